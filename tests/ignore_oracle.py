"""Ignore regions (ignore.py, csrc/crops.hip: target_ignore_kernel, and the *_ignore entry points of csrc/caller.hip,
csrc/topk_loss.hip, csrc/pr_focal.hip) restated in numpy.  Shared by tests/test_ignore_host.py and
tests/test_gpu_ignore.py (test infrastructure; no GPU here).

  * the mark rule: which elements of a window's target become -1, with float32 arithmetic for the source position;
  * ``contains``: the same comparisons on points;
  * "the loss over the non-ignored elements", built on the existing oracles (tests/loss_oracle.py, topk_oracle.py,
    prfocal_oracle.py, imported unchanged): the ignored elements are replaced by elements whose term is exactly 0
    (focal, top-k: pred == target == 0, an exact hit with key 0; penalty-reduced: the term and its interval are set to 0),
    the number of elements -- and with it every reduction depth -- stays;
  * float32 restatements of the three kernels with the mutations the host tests plant.

An element is ignored iff t < 0.0f as an IEEE comparison: -0.0, +0.0 and a NaN are not; -inf and a negative denormal are.
"""
import numpy as np

from tests import loss_oracle, prfocal_oracle, topk_oracle
from tests.helpers import gamma as higham_gamma

F32, F64, U32 = np.float32, np.float64, np.uint32

MUTATIONS = ("ignored_term_counted", "ignored_gradient_stale", "zero_target_ignored", "nan_target_ignored",
             "negative_zero_ignored", "ignored_ranked_first", "ignored_counted_positive", "outside_uses_strict_bounds",
             "class_filter_dropped")


def ignored(target32, mutation=None):
    """bool mask of the ignored elements: t < 0 (and what a mutation makes of it)"""
    t = np.asarray(target32)
    assert t.dtype == F32
    with np.errstate(invalid="ignore"):
        if mutation == "zero_target_ignored":
            return t <= 0
        if mutation == "nan_target_ignored":
            return ~(t >= 0)
        if mutation == "negative_zero_ignored":
            return np.signbit(t) & ~np.isnan(t)
        return t < 0


# ---------------------------------------------------------------------------------------------------------------------
# regions: contains and the mark rule
def _in_rects(rects, rect_class, C, cls, x, y, mutation=None):
    """rects [R, 4] float32, rect_class [R]; cls / x / y arrays of one shape -> bool of that shape: inside some
    rectangle whose class is -1 or cls (a class outside 0..C-1 other than -1 matches nothing; C None: any c >= 0)"""
    out = np.zeros(np.shape(x), bool)
    with np.errstate(invalid="ignore"):
        for (x0, y0, x1, y1), k in zip(np.asarray(rects, F32), np.asarray(rect_class)):
            k = int(k)
            live = k == -1 or (k >= 0 and (C is None or k < C))
            if not live:
                continue
            inside = (x0 <= x) & (x <= x1) & (y0 <= y) & (y <= y1)
            applies = np.ones(np.shape(x), bool) if (k == -1 or mutation == "class_filter_dropped") else (cls == k)
            out |= inside & applies
    return out


def contains(rects, rect_class, frame, cls, xy, mutation=None):
    """IgnoreRegions.contains: rects [S, R, 4], rect_class [S, R], frame / cls integer arrays broadcastable to
    xy[..., 0] -> bool"""
    rects, rect_class = np.asarray(rects, F32), np.asarray(rect_class)
    xy = np.asarray(xy, F32)
    x, y = xy[..., 0], xy[..., 1]
    frame = np.broadcast_to(np.asarray(frame), x.shape)
    cls = np.broadcast_to(np.asarray(cls), x.shape)
    out = np.zeros(x.shape, bool)
    for s in range(rects.shape[0]):
        at = frame == s
        if at.any():
            out |= at & _in_rects(rects[s], rect_class[s], None, cls, x, y, mutation)
    return out


def source_positions(row32, Ho, Wo):
    """(xs, ys) float32 [Ho, Wo]: the warp's own expression, rounded after every operation (csrc/loader.hip)"""
    P = np.asarray(row32, F32)
    x = np.arange(Wo, dtype=F32)[None, :]
    y = np.arange(Ho, dtype=F32)[:, None]
    return ((P[0] * x + P[1] * y) + P[2]).astype(F32), ((P[3] * x + P[4] * y) + P[5]).astype(F32)


def mark_mask(rects, rect_class, index, rows, C, out_size, src_size, outside, mutation=None):
    """bool [N, C, Ho, Wo]: the elements unetpp_target_ignore sets to -1.  rects [M, R, 4] float32 (R may be 0),
    rect_class [M, R], index [N], rows [N, 16]."""
    rects, rect_class = np.asarray(rects, F32), np.asarray(rect_class)
    M = rects.shape[0]
    (Ho, Wo), (Hs, Ws) = out_size, src_size
    N = len(index)
    out = np.zeros((N, C, Ho, Wo), bool)
    cls = np.broadcast_to(np.arange(C).reshape(C, 1, 1), (C, Ho, Wo))
    for n in range(N):
        idx = int(index[n])
        live = 0 <= idx < M
        xs, ys = source_positions(np.asarray(rows, F32)[n], Ho, Wo)
        if live and rects.shape[1] > 0:
            out[n] |= _in_rects(rects[idx], rect_class[idx], C, cls, np.broadcast_to(xs, (C, Ho, Wo)),
                                np.broadcast_to(ys, (C, Ho, Wo)), mutation)
        if outside:
            with np.errstate(invalid="ignore"):
                if mutation == "outside_uses_strict_bounds":
                    inside = (0 < xs) & (xs < F32(Ws - 1)) & (0 < ys) & (ys < F32(Hs - 1))
                else:
                    inside = (0 <= xs) & (xs <= F32(Ws - 1)) & (0 <= ys) & (ys <= F32(Hs - 1))
            out[n] |= ~(inside & live)[None]
    return out


KINDS = {"identity": (False, False, 0, 0.0, 1.0), "flip": (True, False, 0, 0.0, 1.0), "flip_y": (False, True, 0, 0.0, 1.0),
         "quarter": (False, False, 1, 0.0, 1.0), "three_quarters": (True, False, 3, 0.0, 1.0),
         "general": (False, True, 0, 0.6, 1.3)}     # crops_oracle.KINDS and two more of the dihedral group


def window_row(kind, origin, out_size):
    """float64 row [16] of a window whose top-left pixel under the identity is source pixel origin = (ox, oy), under the
    transform KINDS[kind] about the window's centre (crops_oracle.window_row at any origin)"""
    from tests import loader_oracle as lo
    Ho, Wo = out_size
    centre = (origin[0] + (Wo - 1) / 2.0, origin[1] + (Ho - 1) / 2.0)
    row = np.zeros(16)
    row[:6] = lo.inverse_map(*KINDS[kind], centre, (1, 1), out_size).reshape(6)
    row[6:12] = lo.forward_map(*KINDS[kind], centre, (1, 1), out_size).reshape(6)
    row[12] = 1.0
    return row


def cut_window(full, kind, origin, out_size, pad_value):
    """full [..., Hs, Ws] -> [..., Ho, Wo]: the window of a dihedral KINDS[kind] by slice / rot90 / flip on a frame
    padded with pad_value, the construction tests/test_gpu_crops.py uses for the images"""
    import torch
    fx, fy, q, theta, s = KINDS[kind]
    assert theta == 0.0 and s == 1.0
    Ho, Wo = out_size
    assert q % 2 == 0 or Ho == Wo
    pad = max(Ho, Wo) + max(abs(int(origin[0])), abs(int(origin[1])))
    canvas = torch.nn.functional.pad(torch.as_tensor(np.asarray(full)), (pad, pad, pad, pad), value=pad_value)
    w = canvas[..., origin[1] + pad:origin[1] + pad + Ho, origin[0] + pad:origin[0] + pad + Wo]
    w = torch.rot90(w, -q, dims=(-2, -1))
    w = torch.flip(w, dims=(-1,)) if fx else w
    w = torch.flip(w, dims=(-2,)) if fy else w
    return w.numpy()


def apply_mark(target32, mask):
    """the target after the mark launch: exactly -1.0 where the mask is set, untouched elsewhere"""
    out = np.array(target32, dtype=F32)
    out[mask] = F32(-1.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the loss over the non-ignored elements
def sanitise(pred32, target32):
    """-> (pred, target, ignored): copies in which every ignored element is pred == target == +0.0 -- an exact hit of
    FocalLoss_BCE_2d (term 0, gradient 0) with top-k key 0"""
    p, t = np.array(pred32, dtype=F32), np.array(target32, dtype=F32)
    ign = ignored(t)
    p[ign], t[ign] = 0.0, 0.0
    return p, t, ign


def plus_zero(grad32, ign):
    """-> complaints: every gradient at an ignored element is +0.0, sign bit clear"""
    bits = np.asarray(grad32, F32).ravel().view(U32)
    wrong = np.flatnonzero((bits != 0) & np.asarray(ign).ravel())
    if wrong.size:
        i = int(wrong[0])
        return ["%d ignored gradients are not +0.0; first at %d: bits %#x" % (wrong.size, i, int(bits[i]))]
    return []


def check_focal(preds, target, gamma, rows, loss, grads):
    """unetpp_focal_bce_heads_ignore's result (loss [1 + heads], grads or None) against the plain oracle on the masked
    terms -> complaints"""
    heads, bad, bounds = len(preds), [], []
    for h, p in enumerate(preds):
        ps, ts, ign = sanitise(p, target)
        iv = loss_oracle.focal_interval(ps.ravel(), ts.ravel(), gamma, rows * heads)
        if grads is not None:
            more, _ = loss_oracle.check_grad(grads[h], iv)
            bad += ["head %d: %s" % (h, m) for m in more + plus_zero(grads[h], ign)]
        b = loss_oracle.loss_bound(iv._replace(rows=rows))
        bounds.append(b)
        ratio = loss_oracle.loss_ratio(loss[1 + h], b)
        if not ratio <= 1.0:
            bad.append("head %d: loss %r outside [%r, %r] (ratio %.3g)" % (h, float(loss[1 + h]), b[1], b[2], ratio))
    gm = higham_gamma(heads + 2)
    mean = (sum(b[0] for b in bounds) / heads, sum(b[1] for b in bounds) / heads * (1 - gm),
            sum(b[2] for b in bounds) / heads * (1 + gm))
    if not loss_oracle.loss_ratio(loss[0], mean) <= 1.0:
        bad.append("mean over heads %r outside %r" % (float(loss[0]), mean))
    return bad


def topk_expected(pred, target, k, gamma, denom, heads=1):
    """topk_oracle.expected on the sanitised pair: an ignored element has key 0 and, selected or not, the term 0"""
    ps, ts, ign = sanitise(pred, target)
    return topk_oracle.expected(ps, ts, k, gamma, denom, heads), ign


def check_topk(preds, target, k, gamma, denom, loss, grads, kth):
    """unetpp_topk_focal_heads_ignore's result against the oracle -> complaints (kth is exact)"""
    bad = []
    for h, p in enumerate(preds):
        want, ign = topk_expected(p, target, k, gamma, denom, len(preds))
        g = None if grads is None else grads[h]
        bad += ["head %d: %s" % (h, m) for m in topk_oracle.check(want, g, kth[h], loss[1 + h])]
        if g is not None:
            bad += ["head %d: %s" % (h, m) for m in plus_zero(g, ign)]
    return bad


def prfocal_expected(pred, target, heads=1, **params):
    """prfocal_oracle.expected with the ignored elements' terms, gradients and intervals set to 0 (their gradient is
    due as exactly +0.0, as behind a closed gate); n_pos and every reduction depth unchanged"""
    p, t = np.array(pred, dtype=F32).ravel(), np.array(target, dtype=F32).ravel()
    ign = ignored(t)
    p[ign], t[ign] = 0.5, 0.0                         # any finite pair: its numbers are overwritten below
    e = prfocal_oracle.expected(p, t, heads=heads, **params)
    z = lambda a: np.where(ign, 0.0, a)               # noqa: E731
    l, l_lo, l_hi = z(e.l_want), z(e.l_lo), z(e.l_hi)
    gm = higham_gamma(prfocal_oracle.loss_depth(p.size))
    loss = (float(l.sum()) / e.denom, float(l_lo.sum()) / e.denom * (1.0 - gm), float(l_hi.sum()) / e.denom * (1.0 + gm))
    return e._replace(want=z(e.want), lo=z(e.lo), hi=z(e.hi), closed=e.closed | ign, l_want=l, l_lo=l_lo, l_hi=l_hi,
                      loss=loss), ign


def check_prfocal(preds, target, result, **params):
    """unetpp_pr_focal_heads_ignore's (loss, grads or None, n_pos) against the oracle -> complaints (n_pos is exact)"""
    loss, grads, n_pos = result
    bad, exps = [], []
    for h, p in enumerate(preds):
        e, _ = prfocal_expected(p, target, heads=len(preds), **params)
        exps.append(e)
        bad += ["head %d: %s" % (h, m)
                for m in prfocal_oracle.check(e, None if grads is None else grads[h], n_pos, loss[1 + h])]
    ratio = prfocal_oracle.loss_ratio(loss[0], prfocal_oracle.mean_bound(exps))
    if not ratio <= 1.0:
        bad.append("mean over heads %r outside its bound %r" % (float(loss[0]), prfocal_oracle.mean_bound(exps)))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# the kernels restated in float32 torch, with the planted mutations (the order inside a block sum and the finish is
# torch's, which the loss bounds cover)
def _mean(losses, heads):
    import torch
    inv_heads = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(heads), dtype=torch.float32)
    avg = torch.tensor(0.0, dtype=torch.float32)
    for v in losses:
        avg = avg + v
    return torch.stack([(1.0 * avg) * inv_heads] + losses).numpy(), inv_heads


def _mask(le, g, ign, mutation):
    import torch
    m = torch.from_numpy(np.ascontiguousarray(ign))
    if mutation != "ignored_term_counted":
        le = torch.where(m, torch.zeros_like(le), le)
    if mutation != "ignored_gradient_stale":
        g = torch.where(m, torch.zeros_like(g), g)
    return le, g


def restate_focal_f32(preds32, target32, gamma, rows, mutation=None):
    """focal_bce_heads_kernel<., true> and its finish -> (loss float32 [1 + heads], [grad float32 [n]])"""
    import torch
    assert mutation is None or mutation in MUTATIONS
    heads = len(preds32)
    t_np = np.array(target32, dtype=F32).ravel()
    n = t_np.size
    ign = ignored(t_np, mutation)
    t = torch.from_numpy(t_np)
    inv_rows = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(rows), dtype=torch.float32)
    _, inv_heads = _mean([], heads)
    losses, grads = [], []
    for p_np in preds32:
        p = torch.from_numpy(np.array(p_np, dtype=F32).ravel())
        le, g = _mask(*topk_oracle._element_f32(p, t, gamma, inv_rows, inv_heads), ign, mutation)
        padded = torch.zeros(loss_oracle.loss_blocks(n) * loss_oracle.BLOCK, dtype=torch.float32)
        padded[:n] = le
        losses.append((padded.view(-1, loss_oracle.BLOCK).sum(1) * inv_rows).sum())
        grads.append(g.numpy())
    return _mean(losses, heads)[0], grads


def restate_topk_f32(preds32, target32, k, gamma, denom, mutation=None):
    """topk_focal_kernel<., true> and its finish -> (loss [1 + heads], [grad [R, P]], kth float32 [heads, R])"""
    import torch
    assert mutation is None or mutation in MUTATIONS
    heads = len(preds32)
    t_np = np.array(target32, dtype=F32)
    rows, pixels = t_np.shape
    k_eff = min(int(k), pixels)
    ign = ignored(t_np, mutation)
    t = torch.from_numpy(t_np)
    inv_denom = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(denom), dtype=torch.float32)
    _, inv_heads = _mean([], heads)
    losses, grads, kth = [], [], np.zeros((heads, rows), U32)
    for h, p_np in enumerate(preds32):
        p_np = np.array(p_np, dtype=F32)
        with np.errstate(invalid="ignore"):
            key = np.abs(p_np - t_np).view(U32).copy()
        key[ign] = 0x7FFFFFFF if mutation == "ignored_ranked_first" else 0
        sel = np.zeros((rows, pixels), bool)
        for r in range(rows):
            idx = topk_oracle.select(key[r], k_eff)
            sel[r, idx] = True
            kth[h, r] = key[r, idx[-1]]
        le, g = topk_oracle._element_f32(torch.from_numpy(p_np), t, gamma, inv_denom, inv_heads)
        s = torch.from_numpy(sel)
        le, g = torch.where(s, le, torch.zeros_like(le)), torch.where(s, g, torch.zeros_like(g))
        g = torch.where(torch.from_numpy(key == 0) & s, torch.zeros_like(g), g)      # a selected exact hit: +0.0
        le, g = _mask(le, g, ign, mutation)
        losses.append((le.sum(1) * inv_denom).sum())
        grads.append(g.numpy())
    return _mean(losses, heads)[0], grads, kth.view(F32)


def restate_prfocal_f32(preds32, target32, alpha=2.0, beta=4.0, eps=1e-4, positive=1.0, mutation=None):
    """pr_count_kernel, pr_focal_kernel<true> and the finish -> (loss [1 + heads], [grad [n]], n_pos)"""
    import torch
    po = prfocal_oracle
    assert mutation is None or mutation in MUTATIONS
    heads = len(preds32)
    t_np = np.array(target32, dtype=F32).ravel()
    n = t_np.size
    ign = ignored(t_np, mutation)
    t = torch.from_numpy(t_np)
    lo32, hi32 = po.bounds(eps)
    lo, hi = torch.tensor(float(lo32)), torch.tensor(float(hi32))
    alpha32 = torch.tensor(float(alpha), dtype=torch.float32)
    pos = t >= torch.tensor(float(positive), dtype=torch.float32)
    if mutation == "ignored_counted_positive":
        pos = pos | torch.from_numpy(ign)
    n_pos = int(pos.sum())
    inv_denom = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(max(n_pos, 1)), dtype=torch.float32)
    _, inv_heads = _mean([], heads)
    w = torch.where(pos, torch.ones_like(t), po._pow_f32(1.0 - t, po._mode(beta), float(beta), pair=False))
    losses, grads = [], []
    for p_np in preds32:
        p = torch.from_numpy(np.array(p_np, dtype=F32).ravel())
        q = torch.where(p < lo, lo, torch.where(p > hi, hi, p))
        opened = (p >= lo) & (p <= hi)
        omq = 1.0 - q
        lg = torch.where(pos, torch.log(q), torch.log1p(-q))
        a, b = torch.where(pos, omq, q), torch.where(pos, q, omq)
        a1, aa = po._pow_f32(a, po._mode(alpha), float(alpha), pair=True)
        wa = w * aa
        mag = wa / b - (alpha32 * (w * a1)) * lg
        g = torch.where(opened, (torch.where(pos, -mag, mag) * inv_denom) * inv_heads, torch.zeros_like(p))
        le, g = _mask(-wa * lg, g, ign, mutation)
        padded = torch.zeros(po.blocks_of(n) * po.BLOCK, dtype=torch.float32)
        padded[:n] = le
        losses.append(padded.view(-1, po.BLOCK).sum(1).sum() * inv_denom)
        grads.append(g.numpy())
    return _mean(losses, heads)[0], grads, n_pos


# ---------------------------------------------------------------------------------------------------------------------
# input sets: the existing generators' pairs with a share of the target made negative
NEGATIVES = (F32(-1.0), F32(-np.inf), F32(-1e-45), F32(-0.5))     # -1, -inf, a negative denormal, a plain negative


def plant_negatives(preds, target, share=0.25, seed=0, poison=True):
    """In place on float32 arrays of one shape.  A `share` (between 5 % and 50 %) of the target, at least one element
    where there are two, becomes negative, the values of NEGATIVES in turn; where room allows two non-ignored elements
    next to them become -0.0 and +0.0 (pred 0.25).  poison: NaN, +-inf, +-3e38 and 0.5 preds sit under the ignored
    elements.  -> the mask."""
    assert 0.05 <= share <= 0.5
    flat = target.reshape(-1)
    n = flat.size
    rng = np.random.default_rng(9100 + 17 * seed + n)
    count = max(1, int(round(share * n))) if n >= 2 else 0
    idx = np.sort(rng.choice(n, count, replace=False))
    flat[idx] = np.asarray(NEGATIVES)[np.arange(count) % len(NEGATIVES)]
    free = np.setdiff1d(np.arange(n), idx)
    if free.size >= 2:
        j = free[free.size // 2]
        flat[j] = F32(-0.0)                               # not ignored: behaves as a target of 0
        for p in preds:
            p.reshape(-1)[j] = F32(0.25)
    if free.size >= 3:
        j = free[free.size // 2 + 1]
        flat[j] = F32(0.0)                                # +0.0 is not ignored either
        for p in preds:
            p.reshape(-1)[j] = F32(0.25)
    if poison:
        bad = np.asarray([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.5], dtype=F32)     # (0.5: inside every gate)
        for h, p in enumerate(preds):
            p.reshape(-1)[idx] = bad[(np.arange(count) + h) % bad.size]
    mask = np.zeros(n, bool)
    mask[idx] = True
    assert np.array_equal(mask, ignored(flat))
    return mask.reshape(target.shape)


# ---------------------------------------------------------------------------------------------------------------------
# input sets of the mark tests
MARK_SHAPES = [(3, 4, 40, 48), (2, 2, 33, 70), (1, 3, 129, 257)]
MARK_SRC = (2400, 2600)       # (Hs, Ws) of the frames: crops_oracle's window at (X0, Y0) lies well inside


def mark_case(N, C, Ho, Wo, R, first_kind=0, seed=0):
    """-> dict(rects [M, R, 4] f32, rect_class [M, R] i32, index [N] i64, rows [N, 16] f32, kinds, src_size).  M = N
    frames; sample n reads frame n under crops_oracle.KINDS[(first_kind + n) % 4] with the window at (X0, Y0), except
    that with N >= 3 sample 1 has an index outside [0, M).  Planted as R allows (under the identity row):
      0  wholly inside the window, every class        1  across the window's right edge and a tile row, class 0
      2  wholly outside the window                    3  a single pixel, class min(1, C - 1)
      4  x1 < x0: padding                             5  a NaN corner: padding
      6  the whole window with class C: padding       7  the whole window with class -2: padding
      8  overlaps rectangle 0, class C - 1            9  edges at half-integers, every class
      10 across the tile edge at x = 64 (wide windows)
    the rest small and random about the window, of classes -1 .. C; the LAST row (in the second chunk of 256 when
    R = 300) is the window's bottom-left 3 x 3 pixels, every class."""
    from tests import crops_oracle as co
    rng = np.random.default_rng(2300 + 1000 * seed + 7 * R + Ho)
    M, X0, Y0 = N, co.X0, co.Y0
    rects = np.zeros((M, R, 4), dtype=F32)
    classes = np.full((M, R), -1, dtype=np.int32)
    nan = float("nan")
    for m in range(M):
        x0 = rng.uniform(X0 - 60, X0 + Wo + 60, R)
        y0 = rng.uniform(Y0 - 60, Y0 + Ho + 60, R)
        r = np.stack([x0, y0, x0 + rng.uniform(0, 6, R), y0 + rng.uniform(0, 6, R)], axis=1)
        cls = rng.integers(-1, C + 1, R)
        plant = [((X0 + 5 + m, Y0 + 4, X0 + 12 + m, Y0 + 9), -1), ((X0 + Wo - 6, Y0 + 10, X0 + Wo + 20, Y0 + 20), 0),
                 ((X0 - 300, Y0 - 300, X0 - 200, Y0 - 250), -1), ((X0 + 20, Y0 + 20, X0 + 20, Y0 + 20), min(1, C - 1)),
                 ((X0 + 30, Y0 + 5, X0 + 25, Y0 + 30), -1), ((nan, Y0, X0 + 40, Y0 + 40), -1),
                 ((X0, Y0, X0 + Wo, Y0 + Ho), C), ((X0, Y0, X0 + Wo, Y0 + Ho), -2),
                 ((X0 + 10, Y0 + 7, X0 + 18, Y0 + 13), C - 1), ((X0 + 30.5, Y0 + 2.5, X0 + 33.5, Y0 + 4.5), -1),
                 ((X0 + 60, Y0 + 14, X0 + 70, Y0 + 18), -1)]
        for i, (rc, k) in enumerate(plant[:R]):
            r[i], cls[i] = rc, k
        if R > len(plant):
            r[R - 1], cls[R - 1] = (X0 + 0, Y0 + Ho - 3, X0 + 2, Y0 + Ho - 1), -1
        rects[m], classes[m] = r, cls
    index = np.arange(N, dtype=np.int64)
    if N >= 3:
        index[1] = M + 2
    kinds = [co.KINDS[(first_kind + n) % 4] for n in range(N)]
    rows = np.stack([co.window_row(k, (Ho, Wo)) for k in kinds]).astype(F32)
    return dict(rects=rects, rect_class=classes, index=index, rows=rows, kinds=kinds, src_size=MARK_SRC)


def outside_case():
    """A frame of 50 x 30 (Hs x Ws) under windows of 40 x 48: a centred pad in x (ox = -9).  Samples: identity, flip,
    general, identity with index -1 (an all-fill sample), identity shifted so the window also overhangs the bottom.
    One rectangle per frame inside the frame.  -> dict as mark_case, C = 2."""
    Ho, Wo, Hs, Ws = 40, 48, 50, 30
    spec = [("identity", (-9, 4), 0), ("flip", (-9, 10), 1), ("general", (-9, 5), 0), ("identity", (-9, 4), -1),
            ("identity", (-9, 25), 1)]
    rows = np.stack([window_row(k, o, (Ho, Wo)) for k, o, _ in spec]).astype(F32)
    rects = np.asarray([[[3, 8, 9, 15]], [[10, 20, 40, 60]]], dtype=F32)
    classes = np.asarray([[-1], [1]], dtype=np.int32)
    return dict(rects=rects, rect_class=classes, index=np.asarray([s[2] for s in spec], dtype=np.int64), rows=rows,
                kinds=[s[0] for s in spec], src_size=(Hs, Ws), C=2, out_size=(Ho, Wo))


def check_topk_nan_target(preds, target, k, gamma, denom, loss, grads, kth, row, j):
    """A NaN target at [row, j] is NOT ignored: its key is the bits of a NaN, above every number, so it ranks first and
    is selected for every k >= 1 -- the loss of every head and their mean are NaN, the element's gradient is a NaN, kth
    of that row is a NaN for k = 1 and otherwise the (k - 1)-th largest of the row's other keys, the rest of the row's
    selection are those k - 1 elements, and every other row is what the oracle says.  -> complaints.  k < P."""
    t = np.asarray(target, F32)
    rows, pixels = t.shape
    assert np.isnan(t[row, j]) and int(np.isnan(t).sum()) == 1 and 1 <= k < pixels
    bad = []
    if not np.isnan(np.asarray(loss, F32)).all():
        bad.append("a NaN target is hidden: losses %r" % (np.asarray(loss),))
    others = np.arange(rows) != row
    for h, p in enumerate(preds):
        p = np.asarray(p, F32)
        finite_t = t.copy()
        finite_t[row, j] = p[row, j]                  # any finite stand-in: that row is not checked through it
        want, ign = topk_expected(p, finite_t, k, gamma, denom, len(preds))
        g = np.asarray(grads[h], F32).reshape(rows, pixels)
        got_kth = np.asarray(kth[h], F32)
        bad += ["head %d, other rows: %s" % (h, m) for m in topk_oracle.check(want, g, got_kth, 0.0, rows=others)]
        bad += ["head %d: %s" % (h, m) for m in plus_zero(g, ign)]
        if not np.isnan(g[row, j]):
            bad.append("head %d: the gradient at the NaN target is %r, not a NaN: the element was not selected" % (h, g[row, j]))
        ps, ts, _ = sanitise(p[row:row + 1], finite_t[row:row + 1])
        rest_keys = np.delete(topk_oracle.keys(ps, ts)[0], j)
        rest_idx = np.delete(np.arange(pixels), j)
        chosen = rest_idx[topk_oracle.select(rest_keys, k - 1)] if k > 1 else np.zeros(0, np.int64)
        if k == 1:
            if not np.isnan(got_kth[row]):
                bad.append("head %d: kth of the NaN row is %r at k = 1, not a NaN" % (h, got_kth[row]))
        else:
            want_kth = np.sort(rest_keys)[::-1][k - 2]
            if got_kth[row:row + 1].view(U32)[0] != want_kth:
                bad.append("head %d: kth of the NaN row is %r, want %r" % (h, got_kth[row], want_kth.view(F32)))
        unselected = np.ones(pixels, bool)
        unselected[chosen] = False
        unselected[j] = False
        stale = np.flatnonzero((g[row].view(U32) != 0) & unselected)
        if stale.size:
            bad.append("head %d: %d unselected gradients of the NaN row are not +0.0; first at %d" % (h, stale.size, stale[0]))
        live = [i for i in chosen if topk_oracle.keys(ps, ts)[0][i] != 0]
        if any(g[row, i] == 0 for i in live):
            bad.append("head %d: a selected element of the NaN row has no gradient" % h)
    return bad
