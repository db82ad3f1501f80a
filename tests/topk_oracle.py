"""Top-k focal loss (csrc/topk_loss.hip, losses.TopKFocalLoss_BCE_2d) as numpy: the selection rule, the a-priori
acceptance intervals of what the kernel returns, the float32 restatement the host tests mutate, and the input sets.
Shared by tests/test_topk_host.py and tests/test_gpu_topk.py (test infrastructure; no GPU here).

The rule, per head and row (one (n, c) map of P pixels) of pred / target [R, P] float32:
    d = fl32(p - t);  key = the bits of |d| as uint32 (numeric order for non-negative floats, a NaN above everything);
    selected = the k_eff = min(k, P) largest keys, the lowest index first among equal keys
             = np.argsort(~key, kind="stable")[:k_eff];
    kth = |d| at the last of them;  loss = sum over selected of l(p, t) / denom;
    gradient = the focal gradient (tests/loss_oracle.py) on the selected elements, exactly +0.0 on every other.
The per-element error model is loss_oracle.focal_interval's (imported, not copied).  The loss sum: the kernel adds the
selected terms only (an unselected element adds nothing), all of them non-negative, along a fixed path whose length
loss_depth() writes out; [sum lo_i, sum hi_i] / denom widened by gamma(depth) (tests/helpers.gamma) is the bound.
"""
from collections import namedtuple

import numpy as np

from tests import loss_oracle
from tests.helpers import gamma as higham_gamma

F32, F64, U32 = np.float32, np.float64, np.uint32
THREADS = 256            # kTopkThreads: a thread takes 4 consecutive elements per stride of 1024
FINISH_THREADS = 1024    # loss_heads_finish_kernel: partial[h * R + i], i += 1024, then a 10-level tree
DIGIT_BITS = (11, 10, 10)   # bits 30..20, 19..10, 9..0 of the key, most significant first


def keys(pred32, target32):
    """[R, P] float32 -> the uint32 keys"""
    p, t = np.asarray(pred32), np.asarray(target32)
    assert p.dtype == F32 and t.dtype == F32 and p.shape == t.shape and p.ndim == 2
    return np.abs(p - t).view(U32)     # (one float32 subtraction)


def select(key_row, k):
    """the selected indices of one row, in rank order (largest key first, lowest index first among equals)"""
    k_eff = min(int(k), key_row.size)
    return np.argsort(~key_row, kind="stable")[:k_eff]


def selection(pred32, target32, k):
    """-> (selected [R, P] bool, kth [R] float32)"""
    key = keys(pred32, target32)
    sel = np.zeros(key.shape, bool)
    kth = np.zeros(key.shape[0], U32)
    for r in range(key.shape[0]):
        idx = select(key[r], k)
        sel[r, idx] = True
        kth[r] = key[r, idx[-1]]
    return sel, kth.view(F32)


def loss_depth(pixels, k_eff, rows, heads=0):
    """fp32 additions on the longest path from a selected loss term to the loss, written out from csrc/topk_loss.hip:
    a thread adds its selected terms only -- at most k_eff, and at most the 4 elements of each of its strides (the row
    may start up to 3 elements into its first aligned chunk: ceil((P + 3) / 4) chunks, 256 per stride) --, 6 wave
    shuffles, 3 for the workgroup ((w0 + w1) + (w2 + w3), then the product with 1 / denom), ceil(rows / 1024) strided
    additions per finish thread, 10 levels of the LDS tree, and `heads` for the mean over heads.
    k_eff == P is computed by the focal kernels of csrc/caller.hip: loss_oracle.loss_depth."""
    if k_eff >= pixels:
        return loss_oracle.loss_depth(rows * pixels, heads)
    strides = -(-((pixels + 3 + 3) // 4) // THREADS)
    return min(k_eff, 4 * strides) + 6 + 3 + -(-rows // FINISH_THREADS) + 10 + heads


Expected = namedtuple("Expected", "k_eff selected kth iv loss denom")


def expected(pred32, target32, k, gamma, denom, heads=1):
    """What one head must give.  pred / target [R, P] float32, every |d| <= 1.  iv: loss_oracle's intervals of the
    gradient d (mean over `heads` heads) / d pred = g / (denom * heads); loss: (want, lo, hi) of the head's own value."""
    sel, kth = selection(pred32, target32, k)
    rows, pixels = sel.shape
    k_eff = min(int(k), pixels)
    iv = loss_oracle.focal_interval(np.asarray(pred32).ravel(), np.asarray(target32).ravel(), gamma, denom * heads)
    s = sel.ravel()
    gm = higham_gamma(loss_depth(pixels, k_eff, rows))
    loss = (float(iv.l_want[s].sum()) / denom, float(iv.l_lo[s].sum()) / denom * (1.0 - gm),
            float(iv.l_hi[s].sum()) / denom * (1.0 + gm))
    return Expected(k_eff, sel, kth, iv, loss, denom)


def check(want, grad32, kth32, loss, rows=None):
    """-> list of complaints about one head's result (empty: everything holds).  grad32 [R, P] float32 or None, kth32
    [R], loss a number.  rows: boolean [R], the rows to check (default all; the loss is checked only with all rows)."""
    bad = []
    shape = want.selected.shape
    keep_rows = np.ones(shape[0], bool) if rows is None else np.asarray(rows, bool)
    keep = np.broadcast_to(keep_rows[:, None], shape)
    got_kth = np.asarray(kth32, F32).ravel()
    wrong = np.flatnonzero((got_kth.view(U32) != want.kth.view(U32)) & keep_rows)
    if wrong.size:
        r = int(wrong[0])
        bad.append("kth differs in %d rows; first row %d: got %r, want %r" % (wrong.size, r, got_kth[r], want.kth[r]))
    if grad32 is not None:
        g = np.asarray(grad32, F32).reshape(shape)
        stale = np.flatnonzero((g.view(U32) != 0) & ~want.selected & keep)
        if stale.size:
            i = int(stale[0])
            bad.append("%d unselected gradients are not +0.0; first at row %d index %d: %r (bits %#x)"
                       % (stale.size, i // shape[1], i % shape[1], g.ravel()[i], int(g.view(U32).ravel()[i])))
        more, _ = loss_oracle.check_grad(g.ravel(), want.iv, where=(want.selected & keep).ravel())
        bad += ["selected: " + m for m in more]
    if rows is None:
        ratio = loss_oracle.loss_ratio(loss, want.loss)
        if not ratio <= 1.0:
            bad.append("loss %r outside [%r, %r] (want %r, ratio %.3g)" % (float(loss), want.loss[1], want.loss[2],
                                                                           want.loss[0], ratio))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# The kernel restated in float32 torch (the digit passes on integer keys, the index-ordered tie ranks, focal_element's
# arithmetic, the row partials and the finish), with the mutations the host tests plant.  Same operations on the same
# float32 values; the order inside a row sum and inside the finish is torch's, which the loss bound covers.
MUTATIONS = ("ties_to_highest_index", "ties_dropped", "one_more_selected", "unselected_gradient_stale",
             "lowest_digit_skipped", "inv_heads_twice")


def _element_f32(p, t, gamma, inv_denom, scale):
    """focal_element (csrc/focal_element.h) on float32 torch tensors -> (le, g)"""
    import torch
    gm = torch.tensor(float(gamma), dtype=torch.float32)
    d = p - t
    err = (1.0 - d.abs()) + torch.tensor(1e-20, dtype=torch.float32)
    u = 1.0 - err
    lg = torch.log(err)
    ug1 = u * u if float(gamma) == 3.0 else torch.pow(u, gm - 1.0)
    ug = ug1 * u
    le = -ug * lg
    dl_de = gm * ug1 * lg - ug / err
    if float(gamma) < 1.0:
        zero = u == 0
        le = torch.where(zero, torch.zeros_like(le), le)
        dl_de = torch.where(zero, -torch.full_like(u, 1.0 if float(gamma) == 0.0 else 0.0) / err, dl_de)
    return le, (-dl_de * torch.sign(d) * inv_denom) * scale


def _digit_select(key_row, k_eff, passes):
    """the digit passes of the kernel on one row of uint32 keys -> (tau, above, need): after `passes` of the three
    passes, the prefix found so far (lower bits 0), the keys above its bin and the elements still to take from it"""
    prefix, mask, kr, above, shift = 0, 0, int(k_eff), 0, 31
    key = key_row.astype(np.int64)
    for bits in DIGIT_BITS[:passes]:
        shift -= bits
        live = key[(key & mask) == prefix]
        hist = np.bincount((live >> shift) & ((1 << bits) - 1), minlength=1 << bits)
        over = np.cumsum(hist[::-1])[::-1] - hist          # elements in the bins above each bin
        b = int(np.flatnonzero((over < kr) & (kr <= over + hist))[0])
        prefix |= b << shift
        mask |= ((1 << bits) - 1) << shift
        above += int(over[b])
        kr -= int(over[b])
    return prefix, above, kr


def restate_f32(preds32, target32, k, gamma, denom, mutation=None):
    """-> (loss float32 [1 + heads], [grad float32 [R, P]] per head, kth float32 [heads, R]) as the kernel forms them"""
    import torch
    assert mutation is None or mutation in MUTATIONS
    heads = len(preds32)
    t_np = np.asarray(target32, F32)
    rows, pixels = t_np.shape
    k_eff = min(int(k), pixels)
    t = torch.from_numpy(t_np.copy())
    inv_denom = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(denom), dtype=torch.float32)
    inv_heads = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(heads), dtype=torch.float32)
    losses, grads, kth = [], [], np.zeros((heads, rows), U32)
    for h, p_np in enumerate(preds32):
        p_np = np.asarray(p_np, F32)
        key = keys(p_np, t_np)
        sel = np.zeros((rows, pixels), bool)
        for r in range(rows):
            tau, above, need = _digit_select(key[r], k_eff, 2 if mutation == "lowest_digit_skipped" else 3)
            kth[h, r] = tau
            big, tie = key[r] > tau, key[r] == tau
            rank = np.cumsum(tie) - 1                       # index order
            if mutation == "ties_to_highest_index":
                rank = np.cumsum(tie[::-1])[::-1] - 1
            if mutation == "one_more_selected":
                need += 1
            sel[r] = big if mutation == "ties_dropped" else (big | (tie & (rank < need)))
        p = torch.from_numpy(p_np.copy())
        le, g = _element_f32(p, t, gamma, inv_denom, inv_heads)
        if mutation == "inv_heads_twice":
            g = g * inv_heads
        s = torch.from_numpy(sel)
        if mutation != "unselected_gradient_stale":
            g = torch.where(s, g, torch.zeros_like(g))
        partial = torch.where(s, le, torch.zeros_like(le)).sum(1) * inv_denom
        losses.append(partial.sum())
        grads.append(g.numpy())
    avg = torch.tensor(0.0, dtype=torch.float32)
    for v in losses:
        avg = avg + v
    loss = torch.stack([(1.0 * avg) * inv_heads] + losses)
    return loss.numpy(), grads, kth.view(F32)


# ---------------------------------------------------------------------------------------------------------------------
# Input sets.  Every |d| is an exact hit, exactly 1, exactly 0.25 (the planted ties) or at most loss_oracle.MAX_D.
def random_inputs(rows, pixels, seed=0, heads=1):
    """([pred_h [R, P]], target [R, P]) float32: loss_oracle.heads_inputs (random elements, planted hits and |d| = 1)"""
    preds, t = loss_oracle.heads_inputs(heads, rows * pixels, seed)
    return [p.reshape(rows, pixels) for p in preds], t.reshape(rows, pixels)


def tie_inputs(rows, pixels, runs, seed=0, background=None):
    """(pred, target) [R, P] float32 with planted ties: targets are multiples of 2^-10 in [0.25, 0.75], and on every
    index range (lo, hi) of `runs` (in every row) pred = target +- 0.25 with alternating sign, so |d| is exactly 0.25
    there.  Elsewhere |d| is random in (0, 1) and never 0.25 -- or `background` (a float below 0.25) everywhere."""
    rng = np.random.default_rng(4200 + 31 * seed + pixels)
    t = (rng.integers(256, 769, size=(rows, pixels)) / 1024.0).astype(F32)
    if background is None:
        p = loss_oracle._random_pred(rng, t.ravel()).reshape(rows, pixels)
        same = np.abs(p - t) == F32(0.25)
        p[same] = t[same] + F32(0.125)
    else:
        p = (t + F32(background)).astype(F32)
    sign = np.where(np.arange(pixels) % 2 == 0, F32(0.25), F32(-0.25))
    for lo, hi in runs:
        p[:, lo:hi] = t[:, lo:hi] + sign[lo:hi]
    assert np.all(np.abs(p[:, [i for lo, hi in runs for i in range(lo, hi)]] - t[:, [i for lo, hi in runs for i in range(lo, hi)]])
                  == F32(0.25))
    return p, t


def cut_inputs(heads=2, rows=3):
    """([pred_h], target, k): rows of 300 pixels with tie runs of |d| = 0.25 at 62..66 and 290..299; exactly 40 other
    elements of every row are above 0.25 and the rest below 0.2, so k = 43 cuts the first run in the middle and k = 49
    the second (both checked here)"""
    target = tie_inputs(rows, 300, [], seed=5)[1]
    preds = []
    quarter = F32(0.25).view(U32)
    for h in range(heads):
        rng = np.random.default_rng(900 + h)
        p = target + (rng.integers(1, 200, size=target.shape) / 1024.0).astype(F32)     # |d| < 0.2, never a hit
        for r in range(rows):
            idx = rng.choice(np.setdiff1d(np.arange(300), np.r_[62:67, 290:300]), 40, replace=False)
            p[r, idx] = target[r, idx] - (rng.integers(300, 700, size=40) / 2048.0).astype(F32) - F32(0.25)
        p[:, 62:67] = target[:, 62:67] + np.where(np.arange(62, 67) % 2 == 0, F32(0.25), F32(-0.25))
        p[:, 290:300] = target[:, 290:300] + np.where(np.arange(290, 300) % 2 == 0, F32(0.25), F32(-0.25))
        key = keys(p, target)
        assert np.all((key > quarter).sum(1) == 40) and np.all((key == quarter).sum(1) == 15)
        preds.append(p)
    return preds, target, 43


def bit_pattern_inputs(patterns):
    """uint32 [R, P] -> (pred, target): target = 0, pred = the float32 of every pattern, so key == pattern"""
    pat = np.asarray(patterns, U32)
    assert np.all(pat < 0x3F800000), "keys of |d| < 1 only"
    return pat.view(F32).copy(), np.zeros(pat.shape, F32)
