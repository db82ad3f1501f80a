"""Self-distillation across the heads (csrc/distill.hip, ops.distill_heads, losses.HeadDistillLoss) as plain float64
numpy over tests/loss_oracle.py, with an a-priori acceptance interval per gradient element, bounds on S_j, D_j, L_j and
the mean, the float32 restatement of the kernel that the host tests mutate, and the input sets.  Shared by
tests/test_distill_host.py and tests/test_gpu_distill.py (test infrastructure; no GPU here).

The rule, for heads p_0 .. p_{J-1} (shallow to deep), target t, weight w (a float32), with l and g of loss_oracle:
    teacher T(j) = J - 1 ("last") or j + 1 ("next") for j < J - 1; the deepest head has none; q = p_T(j) as data;
    S_j = sum over the elements that are not ignored of l(p_j, t) / rows;
    D_j = sum over the admitted elements of l(p_j, q) / rows,  D_{J-1} = +0.0;   L_j = S_j + w D_j;   loss = mean_j L_j;
    gradient of head j = [g(p_j, t) off the ignored elements + w g(p_j, q) on the admitted ones] / (rows J).
Ignored (ignore on): t < 0.  Admitted: the gate |q - t| < |p - t| (gate on; every element otherwise), except that an
ignored element is admitted iff distill_ignored.  Both decisions are numpy float32 operations on the float32 inputs --
the IEEE operations the kernel performs -- so no near-tie can fall differently here and there.

Error model.  g_s and g_d each lie in loss_oracle.focal_interval's interval (the kernel runs the same focal_element for
both).  The stored element is fl(g_s + fl(w g_d)): two more roundings, each at most 2^-24 relative to its own result, so
each end of [lo_s + w lo_d, hi_s + w hi_d] moves out by 2^-24 (max |w g_d| + max |g_s + w g_d|) over the interval --
absolute, because the two terms may cancel.  Where both terms are exact zeros the interval is the point 0.
S_j and D_j are sums in focal_bce_kernel's order (loss_oracle.loss_depth); L_j adds one product and one sum: depth + 2
for all of them (all terms are non-negative, so the bound is relative), + heads for the mean.
"""
from collections import namedtuple

import numpy as np

from tests import loss_oracle as LO
from tests.helpers import gamma as higham_gamma

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TEACHERS = ("last", "next")
GATES = ("none", "teacher_better")
IGNORED_SHARE = 0.10


def inputs(heads, n, seed=0, ignore=False):
    """loss_oracle.heads_inputs(heads, n, seed) (every value in [0, 1], so |p - q| <= 1 as well); ignore: 10 % of the
    targets at seeded positions (at least one when n >= 3) are -1"""
    preds, t = LO.heads_inputs(heads, n, seed)
    if ignore:
        rng = np.random.default_rng(5000 + 31 * seed + n)
        mask = rng.random(n) < IGNORED_SHARE
        if n >= 3 and not mask.any():
            mask[int(rng.integers(n))] = True
        t = t.copy()
        t[mask] = F32(-1.0)
    return preds, t


def teacher_of(j, heads, teacher):
    assert teacher in TEACHERS and 0 <= j < heads - 1
    return heads - 1 if teacher == "last" else j + 1


def masks(p32, q32, t32, gate, ignore, distill_ignored):
    """-> (ignored, admitted) boolean arrays, decided in float32 as the kernel decides them"""
    p, q, t = (np.asarray(a, dtype=F32).ravel() for a in (p32, q32, t32))
    ignored = (t < F32(0.0)) if ignore else np.zeros(t.shape, bool)
    if gate == "teacher_better":
        with np.errstate(invalid="ignore"):
            admitted = np.abs(q - t) < np.abs(p - t)
    else:
        assert gate == "none"
        admitted = np.ones(t.shape, bool)
    admitted = np.where(ignored, bool(distill_ignored), admitted)
    return ignored, admitted


Head = namedtuple("Head", "want lo hi zero_s zero_d ignored admitted S D L")   # S, D, L: (want, lo, hi)
Expected = namedtuple("Expected", "heads mean w")


def _sum_bound(l_want, l_lo, l_hi, keep, rows, depth):
    gm = higham_gamma(depth)
    return (float(l_want[keep].sum()) / rows, float(l_lo[keep].sum()) / rows * (1.0 - gm),
            float(l_hi[keep].sum()) / rows * (1.0 + gm))


def expected(preds, target, rows, gamma, weight, teacher="last", gate="none", ignore=False, distill_ignored=True):
    """float32 inputs -> Expected: per head the float64 gradient with its interval, which of its two terms are exact
    zeros, and the bounds of S_j, D_j, L_j; the bound of the mean; w as the float32 the kernel reads"""
    heads = len(preds)
    t = np.asarray(target, dtype=F32).ravel()
    n = t.size
    w = float(F32(weight))
    depth = LO.loss_depth(n) + 2
    out, mean = [], [0.0, 0.0, 0.0]
    for j in range(heads):
        p = np.asarray(preds[j], dtype=F32).ravel()
        student = j < heads - 1
        q = np.asarray(preds[teacher_of(j, heads, teacher)], dtype=F32).ravel() if student else p
        ignored, admitted = masks(p, q, t, gate, ignore, distill_ignored)
        if not student:
            admitted = np.zeros(n, bool)
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
        S = _sum_bound(iv_s.l_want, iv_s.l_lo, iv_s.l_hi, ~ignored, rows, depth)
        D = _sum_bound(iv_d.l_want, iv_d.l_lo, iv_d.l_hi, admitted, rows, depth)
        gm = higham_gamma(depth)
        L = (S[0] + w * D[0], (S[1] + w * D[1]) * (1.0 - gm), (S[2] + w * D[2]) * (1.0 + gm))
        out.append(Head(want, lo - widen, hi + widen, zero_s, zero_d, ignored, admitted, S, D, L))
        for k in range(3):
            mean[k] += L[k] / heads
    gm = higham_gamma(depth + heads)
    return Expected(out, (mean[0], mean[1] * (1.0 - gm), mean[2] * (1.0 + gm)), w)


def loss_f64(students, teachers, target, rows, gamma, weight, ignored, admitted):
    """the loss in float64 with the teachers' maps and the masks held fixed: what the oracle's gradient differentiates"""
    heads = len(students)
    t = np.asarray(target, dtype=F64).ravel()
    total = 0.0
    for j in range(heads):
        p = np.asarray(students[j], dtype=F64).ravel()
        u = np.maximum(np.abs(p - t) - 1e-20, 0.0)
        total += float(LO._l_and_g(np.where(ignored[j], 0.0, u), gamma)[0][~ignored[j]].sum()) / rows
        if j < heads - 1:
            q = np.asarray(teachers[j], dtype=F64).ravel()
            u = np.maximum(np.abs(p - q) - 1e-20, 0.0)
            total += float(F32(weight)) * float(LO._l_and_g(np.where(admitted[j], u, 0.0), gamma)[0][admitted[j]].sum()) / rows
    return total / heads


def check(exp, loss, grads, supervised, distill):
    """-> (complaints, worst err / room).  loss [1 + heads], grads (a list, or None), supervised and distill [heads] as
    float32 numpy.  Every gradient inside its interval; where exactly one term is an exact zero the sign of the other;
    where both are, 0.0 -- with the sign bit clear where the zero is by rule (an ignored element whose distillation term is
    kept out or that belongs to the deepest head); every loss value inside its bound; D of the deepest head +0.0."""
    bad, worst = [], 0.0
    heads = len(exp.heads)
    loss, supervised, distill = (np.asarray(a, dtype=F32) for a in (loss, supervised, distill))
    for j, h in enumerate(exp.heads):
        for name, got, bound in (("S", supervised[j], h.S), ("D", distill[j], h.D), ("L", loss[1 + j], h.L)):
            r = LO.loss_ratio(got, bound)
            worst = max(worst, r)
            if not r <= 1.0:
                bad.append("head %d: %s = %r outside [%r, %r] (want %r)" % (j, name, float(got), bound[1], bound[2], bound[0]))
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
        neg = np.flatnonzero(by_rule & (got.view(np.uint32) != 0))
        if neg.size:
            bad.append("head %d: %d ignored elements without a distillation term are not +0.0; first at %d" % (j, neg.size, int(neg[0])))
    if distill[heads - 1].view(np.uint32) != 0:
        bad.append("D of the deepest head is %r, not +0.0" % float(distill[heads - 1]))
    r = LO.loss_ratio(loss[0], exp.mean)
    worst = max(worst, r)
    if not r <= 1.0:
        bad.append("loss = %r outside [%r, %r] (want %r)" % (float(loss[0]), exp.mean[1], exp.mean[2], exp.mean[0]))
    return bad, worst


def gated_share(preds, target, teacher="last", ignore=False):
    """the share of the student elements (ignored ones left out) that the gate admits"""
    heads, admitted, total = len(preds), 0, 0
    for j in range(heads - 1):
        ign, adm = masks(preds[j], preds[teacher_of(j, heads, teacher)], target, "teacher_better", ignore, True)
        admitted += int((adm & ~ign).sum())
        total += int((~ign).sum())
    return admitted / max(total, 1)


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's arithmetic restated in float32 torch (focal_element, the two masks, the two combinations), with the
# mutations the host tests plant.  The order inside a block sum and inside the finish differs from the kernel's
# (torch's sum), which the loss bounds cover.
MUTATIONS = ("teacher_gets_gradient", "gate_inverted", "gate_applied_to_ignored", "weight_twice", "weight_read_as_one",
             "next_uses_last", "distill_dropped_on_ignored", "distill_kept_when_distill_ignored_false",
             "loss_misses_distill_sum")


def _element_f32(p, t, gamma, inv_rows, scale):
    """focal_element in float32 torch -> (loss term, gradient)"""
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
    return le, (-dl_de * torch.sign(d) * inv_rows) * scale


def _block_sum(le, keep, inv_rows):
    import torch
    n = le.numel()
    blocks = LO.loss_blocks(n)
    padded = torch.zeros(blocks * LO.BLOCK, dtype=torch.float32)
    padded[:n] = torch.where(keep, le, torch.zeros_like(le))
    return (padded.view(blocks, LO.BLOCK).sum(1) * inv_rows).sum()


def restate_f32(preds, target, rows, gamma, weight, teacher="last", gate="none", ignore=False, distill_ignored=True,
                mutation=None):
    """-> (loss [1 + heads], [grad], S [heads], D [heads]) float32 numpy as the kernel forms them"""
    import torch
    assert mutation is None or mutation in MUTATIONS
    heads = len(preds)
    P = [torch.from_numpy(np.array(p, dtype=F32).ravel()) for p in preds]
    t = torch.from_numpy(np.array(target, dtype=F32).ravel())
    one = torch.tensor(1.0, dtype=torch.float32)
    inv_rows = one / torch.tensor(float(rows), dtype=torch.float32)
    scale = one / torch.tensor(float(heads), dtype=torch.float32)
    w = torch.tensor(1.0 if mutation == "weight_read_as_one" else float(weight), dtype=torch.float32)
    ignored = (t < 0) if ignore else torch.zeros_like(t, dtype=torch.bool)
    zero = torch.zeros((), dtype=torch.float32)
    grads = [None] * heads
    extra = [torch.zeros_like(t) for _ in range(heads)]    # (teacher_gets_gradient)
    L, S, D = [], [], []
    for j in range(heads):
        p = P[j]
        ls, gs = _element_f32(p, t, gamma, inv_rows, scale)
        gs = torch.where(ignored, torch.zeros_like(gs), gs)
        s = _block_sum(ls, ~ignored, inv_rows)
        if j < heads - 1:
            tj = heads - 1 if mutation == "next_uses_last" else teacher_of(j, heads, teacher)
            q = P[tj]
            ld, gd = _element_f32(p, q, gamma, inv_rows, scale)
            admit = torch.ones_like(ignored)
            if gate == "teacher_better":
                admit = (q - t).abs() < (p - t).abs()
                if mutation == "gate_inverted":
                    admit = ~admit
            on_ignored = torch.full_like(admit, bool(distill_ignored))
            if mutation == "gate_applied_to_ignored":
                on_ignored = on_ignored & admit
            if mutation == "distill_dropped_on_ignored":
                on_ignored = torch.zeros_like(admit)
            if mutation == "distill_kept_when_distill_ignored_false":
                on_ignored = torch.ones_like(admit)
            admit = torch.where(ignored, on_ignored, admit)
            wgd = w * gd
            if mutation == "weight_twice":
                wgd = w * wgd
            grads[j] = torch.where(admit, gs + wgd, gs)
            if mutation == "teacher_gets_gradient":
                extra[tj] = extra[tj] - torch.where(admit, wgd, torch.zeros_like(wgd))
            d = _block_sum(ld, admit, inv_rows)
        else:
            grads[j] = gs
            d = zero
        wd = w * d
        if mutation == "weight_twice":
            wd = w * wd
        S.append(s)
        D.append(d)
        L.append(s if mutation == "loss_misses_distill_sum" else s + wd)
    avg = zero
    for l in L:
        avg = avg + l
    avg = (1.0 * avg) * scale
    grads = [(g + e).numpy() for g, e in zip(grads, extra)]
    return (torch.stack([avg] + L).numpy(), grads, torch.stack(S).numpy(), torch.stack(D).numpy())
