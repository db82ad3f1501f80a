"""Distillation from an external map (csrc/distill.hip: unetpp_teacher_heads, ops.teacher_heads,
losses.TeacherDistillLoss) as plain float64 numpy over tests/loss_oracle.py and tests/distill_oracle.py: the three masks
(void, gate, ignore), an a-priori acceptance interval per gradient element, bounds on S_h, D_h, L_h and the mean, the
float32 restatement of the kernel that the host tests mutate, and the input sets.  Shared by tests/test_teacher_host.py
and tests/test_gpu_teacher.py (test infrastructure; no GPU here).

The rule, for heads p_0 .. p_{J-1}, target t, ONE teacher map q of the target's shape and weight w (a float32), with l
and g of loss_oracle:
    S_h = sum over the elements that are not ignored of l(p_h, t) / rows;
    D_h = sum over the admitted elements of l(p_h, q) / rows -- for every head, the deepest included;
    L_h = S_h + w D_h;   loss = mean_h L_h;
    gradient of head h = [g(p_h, t) off the ignored elements + w g(p_h, q) on the admitted ones] / (rows J).
Void: q < 0 (float32; -0.0 and a NaN are not).  Ignored (ignore on): t < 0.  Admitted: not void, and the gate
|q - t| < |p - t| (gate on; every element otherwise), except that an ignored element counts as having passed the gate and
is admitted iff distill_ignored and it is not void.  All three decisions are numpy float32 operations on the float32
inputs -- the IEEE operations the kernel performs -- so no near-tie can fall differently here and there.

Error model: distill_oracle's, unchanged (the kernel runs the same element function and the same two combinations): the
stored element is fl(g_s + fl(w g_d)), each end of [lo_s + w lo_d, hi_s + w hi_d] moves out by
2^-24 (max |w g_d| + max |g_s + w g_d|); S_h, D_h and L_h are sums of depth loss_depth(n) + 2, + heads for the mean.
What the kernel adds to that is exact: L_h is fl(S_h + fl(w D_h)) of the S_h and D_h it reports and the mean is the
trainer's sum of the L_h it reports times float32(1 / heads), which `check` holds bit for bit.
"""
from collections import namedtuple

import numpy as np

from tests import distill_oracle as DO
from tests import loss_oracle as LO
from tests.helpers import gamma as higham_gamma

F32, F64, U32 = np.float32, np.float64, np.uint32
U = 2.0 ** -24
GATES = DO.GATES
IGNORED_SHARE = 0.24     # with a third of the teacher void: 8 % of the elements ignored and void, 16 % ignored with a teacher
VOID_SHARE = 1.0 / 3.0
CLASSES = ("admitted", "gated_out", "void", "ignored_admitted", "ignored_kept_out")
MIN_SHARE = 0.05
MIN_SHARE_N = 2047       # below this a share of 5 % is a handful of elements: the classes are asserted from here on


def inputs(heads, n, seed=0, ignore=False, void=False):
    """-> ([pred_h], target, teacher) float32 [n].  preds and target: loss_oracle.heads_inputs(heads, n, seed); ignore:
    IGNORED_SHARE of the targets, at positions seeded as distill_oracle.inputs seeds them, are -1.  The teacher is random
    in [0, 1] from its own generator; where n allows, planted: exact +0.0 and -0.0 (a teacher that exists), exact ties of
    the gate (t = 0.5, every p_h = 0.25, q = 0.75: |q - t| == |p - t| with p != q) and elements equal to head 0 (an exact
    hit of the distillation term); void: VOID_SHARE of the elements are negative, half of them -1, half random in
    (-1, 0).  No |p_h - q| of an element with a teacher exceeds loss_oracle.MAX_D, planted |d| = 1 elements excepted."""
    preds, t = LO.heads_inputs(heads, n, seed)
    preds, t = [p.copy() for p in preds], t.copy()
    rng = np.random.default_rng(9000 + 31 * seed + n)
    q = rng.random(n).astype(F32)
    planted = np.zeros(n, bool)
    planted[[i for i in (0, 1, n - 1, n // 2, n - 2) if 0 <= i < n]] = True      # (loss_oracle._plant's places)
    free = np.flatnonzero(~planted)
    if free.size >= 16:
        pick = rng.permutation(free)
        k = max(1, free.size // 100)
        zeros, negzeros, ties, hits = pick[:k], pick[k:2 * k], pick[2 * k:3 * k], pick[3 * k:4 * k]
        q[zeros], q[negzeros] = F32(0.0), F32(-0.0)
        t[ties], q[ties] = F32(0.5), F32(0.75)
        for p in preds:
            p[ties] = F32(0.25)
        q[hits] = preds[0][hits]
        planted[pick[:4 * k]] = True
    far = np.zeros(n, bool)
    for p in preds:
        far |= np.abs(p.astype(F64) - q.astype(F64)) > LO.MAX_D
    q[far] = F32(0.5)
    if ignore:
        r = np.random.default_rng(5000 + 31 * seed + n)
        mask = (r.random(n) < IGNORED_SHARE) & ~planted
        if n >= 3 and not mask.any():
            mask[int(free[int(r.integers(free.size))]) if free.size else 0] = True
        t[mask] = F32(-1.0)
    if void:
        r = np.random.default_rng(7000 + 31 * seed + n)
        mask = (r.random(n) < VOID_SHARE * n / max(int((~planted).sum()), 1)) & ~planted    # (a third of all n)
        if n >= 3 and not mask.any() and free.size:
            mask[int(free[int(r.integers(free.size))])] = True
        neg = -(r.random(n).astype(F32) * F32(0.98) + F32(0.01))
        neg[r.random(n) < 0.5] = F32(-1.0)
        q[mask] = neg[mask]
    return preds, t, q


def masks(p32, q32, t32, gate, ignore, distill_ignored):
    """-> (ignored, void, admitted) boolean arrays, decided in float32 as the kernel decides them"""
    p, q, t = (np.asarray(a, dtype=F32).ravel() for a in (p32, q32, t32))
    ignored, admitted = DO.masks(p, q, t, gate, ignore, distill_ignored)
    with np.errstate(invalid="ignore"):
        void = q < F32(0.0)
    return ignored, void, admitted & ~void


Head = namedtuple("Head", "want lo hi zero_s zero_d ignored void admitted S D L")   # S, D, L: (want, lo, hi)
Expected = namedtuple("Expected", "heads mean w")


def expected(preds, target, teacher, rows, gamma, weight, gate="none", ignore=False, distill_ignored=True):
    """float32 inputs -> Expected: per head the float64 gradient with its interval, which of its two terms are exact
    zeros, the masks, and the bounds of S_h, D_h, L_h; the bound of the mean; w as the float32 the kernel reads"""
    heads = len(preds)
    t = np.asarray(target, dtype=F32).ravel()
    q = np.asarray(teacher, dtype=F32).ravel()
    n = t.size
    w = float(F32(weight))
    depth = LO.loss_depth(n) + 2
    gm = higham_gamma(depth)
    out, mean = [], [0.0, 0.0, 0.0]
    for j in range(heads):
        p = np.asarray(preds[j], dtype=F32).ravel()
        ignored, void, admitted = masks(p, q, t, gate, ignore, distill_ignored)
        iv_s = LO.focal_interval(p, np.where(ignored, p, t), gamma, rows * heads)     # (an ignored element: a hit, dropped below)
        iv_d = LO.focal_interval(p, np.where(admitted, q, p), gamma, rows * heads)
        zero_s = ignored | iv_s.hit
        zero_d = ~admitted | iv_d.hit

        def off(a, zero):
            return np.where(zero, 0.0, a)

        want = off(iv_s.want, zero_s) + w * off(iv_d.want, zero_d)
        lo = off(iv_s.lo, zero_s) + w * off(iv_d.lo, zero_d)
        hi = off(iv_s.hi, zero_s) + w * off(iv_d.hi, zero_d)
        big_d = w * np.maximum(np.abs(off(iv_d.lo, zero_d)), np.abs(off(iv_d.hi, zero_d)))
        widen = U * (big_d + np.maximum(np.abs(lo), np.abs(hi)))
        S = DO._sum_bound(iv_s.l_want, iv_s.l_lo, iv_s.l_hi, ~ignored, rows, depth)
        D = DO._sum_bound(iv_d.l_want, iv_d.l_lo, iv_d.l_hi, admitted, rows, depth)
        L = (S[0] + w * D[0], (S[1] + w * D[1]) * (1.0 - gm), (S[2] + w * D[2]) * (1.0 + gm))
        out.append(Head(want, lo - widen, hi + widen, zero_s, zero_d, ignored, void, admitted, S, D, L))
        for k in range(3):
            mean[k] += L[k] / heads
    gm = higham_gamma(depth + heads)
    return Expected(out, (mean[0], mean[1] * (1.0 - gm), mean[2] * (1.0 + gm)), w)


def class_shares(exp):
    """per head {class: share of the n elements}, from the oracle's masks: admitted (not ignored), gated_out (has a
    teacher, not ignored, kept out by the gate), void, ignored_admitted, ignored_kept_out"""
    out = []
    for h in exp.heads:
        n = float(h.void.size)
        out.append({"admitted": (h.admitted & ~h.ignored).sum() / n,
                    "gated_out": (~h.admitted & ~h.ignored & ~h.void).sum() / n,
                    "void": h.void.sum() / n,
                    "ignored_admitted": (h.ignored & h.admitted).sum() / n,
                    "ignored_kept_out": (h.ignored & ~h.admitted).sum() / n})
    return out


def classes_of(gate, ignore, distill_ignored, void):
    """the classes a configuration exercises"""
    c = ["admitted"]
    if gate == "teacher_better":
        c.append("gated_out")
    if void:
        c.append("void")
    if ignore and distill_ignored:
        c.append("ignored_admitted")
    if ignore and (void or not distill_ignored):
        c.append("ignored_kept_out")
    return c


def thin_classes(exp, gate, ignore, distill_ignored, void):
    """the (head, class, share) of every exercised class below MIN_SHARE; for n >= MIN_SHARE_N"""
    want = classes_of(gate, ignore, distill_ignored, void)
    return [(j, c, float(s[c])) for j, s in enumerate(class_shares(exp)) for c in want if not s[c] >= MIN_SHARE]


def _f32_bits(x):
    return np.asarray(x, dtype=F32).reshape(()).view(U32)


def combine_f32(s, w, d):
    """fl(s + fl(w d)) in float32"""
    return F32(F32(s) + F32(F32(w) * F32(d)))


def mean_f32(L):
    """the trainer's mean in float32: avg = 0; avg = avg + L_h; (1.0 avg) float32(1 / heads)"""
    avg = F32(0.0)
    for l in L:
        avg = F32(avg + F32(l))
    return F32(F32(F32(1.0) * avg) * F32(F32(1.0) / F32(len(L))))


def check(exp, loss, grads, supervised, distill, exact=True):
    """-> (complaints, worst err / room).  loss [1 + heads], grads (a list, or None), supervised and distill [heads] as
    float32 numpy.  Every gradient inside its interval; where exactly one term is an exact zero the sign of the other;
    where both are, 0.0 -- with the sign bit clear where the zero is by rule (an ignored element whose distillation term
    is kept out); every loss value inside its bound.  exact: also L_h == fl(S_h + fl(w D_h)) of the reported S_h and D_h
    and loss[0] == the trainer's float32 mean of the reported L_h, bit for bit (the kernel's two combinations; a path
    that divides by the number of heads instead of multiplying by its float32 inverse passes exact=False)."""
    bad, worst = [], 0.0
    loss, supervised, distill = (np.asarray(a, dtype=F32) for a in (loss, supervised, distill))
    for j, h in enumerate(exp.heads):
        for name, got, bound in (("S", supervised[j], h.S), ("D", distill[j], h.D), ("L", loss[1 + j], h.L)):
            r = LO.loss_ratio(got, bound)
            worst = max(worst, r)
            if not r <= 1.0:
                bad.append("head %d: %s = %r outside [%r, %r] (want %r)" % (j, name, float(got), bound[1], bound[2], bound[0]))
        if not h.admitted.any() and distill[j].view(U32) != 0:
            bad.append("head %d: D = %r with no element admitted, not +0.0" % (j, float(distill[j])))
        if exact:
            with np.errstate(all="ignore"):
                want = combine_f32(supervised[j], exp.w, distill[j])
            if _f32_bits(want) != _f32_bits(loss[1 + j]):
                bad.append("head %d: L = %r is not fl(S + fl(w D)) = %r" % (j, float(loss[1 + j]), float(want)))
        if grads is None:
            continue
        got = np.asarray(grads[j], dtype=F32).ravel()
        g64 = got.astype(F64)
        with np.errstate(all="ignore"):
            room = np.where(g64 >= h.want, h.hi - h.want, h.want - h.lo)
            err = np.abs(g64 - h.want)
            r = np.where(err == 0.0, 0.0, err / room)
        r[~np.isfinite(g64) | np.isnan(r)] = np.inf
        worst = max(worst, float(r.max(initial=0.0)))
        outside = np.flatnonzero(r > 1.0)
        if outside.size:
            i = int(outside[np.argmax(r[outside])])
            bad.append("head %d: %d of %d gradients outside their interval; worst at %d: got %r, want %r in [%r, %r]"
                       % (j, outside.size, got.size, i, g64[i], h.want[i], h.lo[i], h.hi[i]))
        one = h.zero_s ^ h.zero_d
        with np.errstate(invalid="ignore"):
            wrong = np.flatnonzero(one & (np.sign(g64) != np.sign(h.want)))
        if wrong.size:
            bad.append("head %d: %d gradients with the wrong sign; first at %d: got %r, want %r"
                       % (j, wrong.size, int(wrong[0]), g64[wrong[0]], h.want[wrong[0]]))
        both = h.zero_s & h.zero_d
        nz = np.flatnonzero(both & (g64 != 0.0))
        if nz.size:
            bad.append("head %d: %d elements whose two terms are exact zeros hold something else; first at %d: %r"
                       % (j, nz.size, int(nz[0]), g64[nz[0]]))
        by_rule = h.ignored & ~h.admitted
        neg = np.flatnonzero(by_rule & (got.view(U32) != 0))
        if neg.size:
            bad.append("head %d: %d ignored elements without a distillation term are not +0.0; first at %d" % (j, neg.size, int(neg[0])))
    r = LO.loss_ratio(loss[0], exp.mean)
    worst = max(worst, r)
    if not r <= 1.0:
        bad.append("loss = %r outside [%r, %r] (want %r)" % (float(loss[0]), exp.mean[1], exp.mean[2], exp.mean[0]))
    if exact:
        with np.errstate(all="ignore"):
            want = mean_f32(loss[1:])
        if _f32_bits(want) != _f32_bits(loss[0]):
            bad.append("loss = %r is not the float32 mean of the L_h = %r" % (float(loss[0]), float(want)))
    return bad, worst


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's arithmetic restated in float32 torch, operation for operation (distill_oracle's focal_element, the three
# masks, the two combinations), with the mutations the host tests plant.  The order inside a block sum and inside the
# finish differs from the kernel's (torch's sum) and torch's log is not the device's, which the bounds cover; the masks
# and the two combinations are IEEE operations and the same bits everywhere.
MUTATIONS = ("void_rule_le", "void_ignored_under_distill_ignored", "gate_le", "ignored_element_fails_gate",
             "deepest_head_without_teacher", "weight_applied_to_supervised", "fused_combine", "divisor_n",
             "gate_inverted", "weight_twice")


def restate_f32(preds, target, teacher, rows, gamma, weight, gate="none", ignore=False, distill_ignored=True,
                mutation=None):
    """-> (loss [1 + heads], [grad], S [heads], D [heads], [admitted]) float32 / bool numpy as the kernel forms them"""
    import torch
    assert mutation is None or mutation in MUTATIONS
    heads = len(preds)
    P = [torch.from_numpy(np.array(p, dtype=F32).ravel()) for p in preds]
    t = torch.from_numpy(np.array(target, dtype=F32).ravel())
    q = torch.from_numpy(np.array(teacher, dtype=F32).ravel())
    one = torch.tensor(1.0, dtype=torch.float32)
    divisor = float(t.numel()) if mutation == "divisor_n" else float(rows)
    inv_rows = one / torch.tensor(divisor, dtype=torch.float32)
    scale = one / torch.tensor(float(heads), dtype=torch.float32)
    w = torch.tensor(float(weight), dtype=torch.float32)
    ignored = (t < 0) if ignore else torch.zeros_like(t, dtype=torch.bool)
    void = (q <= 0) if mutation == "void_rule_le" else (q < 0)
    grads, admits, L, S, D = [], [], [], [], []
    for j in range(heads):
        p = P[j]
        ls, gs = DO._element_f32(p, t, gamma, inv_rows, scale)
        gs = torch.where(ignored, torch.zeros_like(gs), gs)
        s = DO._block_sum(ls, ~ignored, inv_rows)
        ld, gd = DO._element_f32(p, q, gamma, inv_rows, scale)
        admit = torch.ones_like(ignored)
        if gate == "teacher_better":
            admit = ((q - t).abs() <= (p - t).abs()) if mutation == "gate_le" else ((q - t).abs() < (p - t).abs())
            if mutation == "gate_inverted":
                admit = ~admit
        on_ignored = torch.full_like(admit, bool(distill_ignored))
        if mutation == "ignored_element_fails_gate":
            on_ignored = on_ignored & admit
        if mutation == "void_ignored_under_distill_ignored":
            admit = torch.where(ignored, on_ignored, admit & ~void)        # (the void rule applied before the ignore rule)
        else:
            admit = torch.where(ignored, on_ignored, admit) & ~void
        if mutation == "deepest_head_without_teacher" and j == heads - 1:
            admit = torch.zeros_like(admit)
        wgd = w * gd
        if mutation == "weight_twice":
            wgd = w * wgd
        if mutation == "weight_applied_to_supervised":
            gs = w * gs
        grads.append(torch.where(admit & (wgd != 0), gs + wgd, gs))      # (a zero product: g_s keeps its bits)
        d = DO._block_sum(ld, admit, inv_rows)
        wd = w * d
        if mutation == "weight_twice":
            wd = w * wd
        if mutation == "fused_combine":      # one rounding: the float64 product is exact, its sum rounded once more
            l = (s.double() + w.double() * d.double()).float()
        elif mutation == "weight_applied_to_supervised":
            l = w * s + wd
        else:
            l = s + wd
        admits.append(admit.numpy())
        S.append(s)
        D.append(d)
        L.append(l)
    avg = torch.zeros((), dtype=torch.float32)
    for l in L:
        avg = avg + l
    avg = (1.0 * avg) * scale
    return (torch.stack([avg] + L).numpy(), [g.numpy() for g in grads], torch.stack(S).numpy(), torch.stack(D).numpy(),
            admits)
