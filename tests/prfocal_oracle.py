"""Penalty-reduced focal loss (csrc/pr_focal.hip, ops.pr_focal_heads, losses.PenaltyReducedFocalLoss) as float64 numpy,
with an a-priori acceptance interval per gradient element and per loss term, a bound on every loss sum, the float32
restatement of the kernel that the host tests mutate, and the input sets.  Shared by tests/test_prfocal_host.py and
tests/test_gpu_prfocal.py (test infrastructure; no GPU here).

The rule, element by element over n float32 values of a head p (in [0, 1]) and the target t (domain [0, 1]), with
float32 parameters alpha >= 0, beta >= 0, eps in (0, 0.5), positive in (0, 1]:
    lo = float32(eps),  hi = float32(1) - lo (one float32 subtraction);  q = min(max(p, lo), hi), a NaN stays a NaN;
    the gradient passes where lo <= p <= hi (torch.clamp's rule) and is exactly 0 elsewhere;
    an element is positive when t >= positive:
        positive:   l = -(1 - q)^alpha log(q)
        otherwise:  l = -(1 - t)^beta q^alpha log(1 - q),  log(1 - q) in its well-conditioned form log1p(-q);
    0^0 = 1;  n_pos = the positive elements of the target (an exact integer),  denom = max(n_pos, 1);
    loss_h = (sum of l over head h) * (1 / denom);
    loss[0] = (0 + loss_1 + ... + loss_n) * (1 / n_heads) in that order, as unetpp_focal_bce_heads forms it;
    grad_h = d loss[0] / d pred_h = ((dl / dq) * (1 / denom)) * (1 / n_heads).
A NaN in pred makes the loss NaN; the gradient at that one element is unspecified (NaN or 0).  A label at a sub-pixel
position never produces a target of exactly 1.0; for such targets positive = exp(-0.5 * 0.7071 / radius).
Here the rule is evaluated in float64 on the float32 operands, with the float32 lo / hi / positive.

With a = 1 - q, b = q (positive) or a = q, b = 1 - q (otherwise), lg = log b, w = 1 or (1 - t)^beta:
    l = -w a^alpha lg,    |dl/dq| = w a^alpha / b - alpha w a^(alpha-1) lg  (both terms >= 0: no cancellation),
    dl/dq = -|dl/dq| (positive) or +|dl/dq| (otherwise).

Error model of the kernel, in units of U = 2^-24 (one float32 rounding to nearest), derived from the operations
pr_element (csrc/pr_focal.hip) performs, not from what it returns.  The device math library is specified to OpenCL's
accuracy: log 3 ulp = 6 U, log1p 2 ulp = 4 U, pow 16 ulp = 32 U, a division 2.5 ulp = 5 U.
  input perturbations: q is p or a parameter, exact.  fl(1 - q) rounds once (1 U on a for a positive, on b otherwise);
      fl(1 - t) rounds once (1 U on the base of the weight).  A base off by d makes x^e off by e d.  log1pf sees -q
      exactly, logf sees q exactly.
  w:   0 for a positive; otherwise beta * 1 + [roundings of the chain: 0, 0, 1, 2, 2 for beta = 0..4, else pow = 32].
  aa = a^alpha:        alpha * (1 if positive) + [0, 0, 1, 2, 3 for alpha = 0..4 (x, x x, (x x) x, ((x x) x) x), else 32].
  a1 = a^(alpha-1):    |alpha - 1| * (1 if positive) + [-, 0, 0, 1, 2]; for a general alpha it is aa / a:
                       E(aa) + (1 if positive) + 5.
  l = -(w aa) lg:      E(w) + E(aa) + 1 (w aa) + LOG + 1 (the product);  LOG = 6 (positive) or 4.
  term1 = (w aa) / b:  E(w) + E(aa) + 1 + (1 if not positive: b is rounded) + 5.
  term2 = (alpha (w a1)) lg:  E(w) + E(a1) + 1 (w a1) + 1 (alpha ..) + LOG + 1;  absent (exactly 0) for alpha = 0.
  |dl/dq| = term1 - term2, terms of one sign:  max(E(term1), E(term2)) + 1.
  grad = (dl/dq * inv_denom) * scale:  + 1 + 2 (inv_denom = 1 / float(denom): the conversion and the division)
                       + 1 + 1 (scale = 1 / n_heads is rounded itself).
Second-order terms are covered by the factor (1 + 2^-10) on the sum; results below the normal range of float32 round
absolutely, which ABS_FLOOR = 2^-140 covers (the input sets stay far above it).
The loss sum: all terms are non-negative; the kernel's fixed path has loss_depth() float32 roundings on its longest
branch, so [sum l_lo, sum l_hi] / denom widened by gamma(depth) (tests/helpers.gamma) is a relative bound.  n_pos is exact.
"""
import functools
from collections import namedtuple

import numpy as np

from tests.helpers import gamma as higham_gamma

F32, F64, U32 = np.float32, np.float64, np.uint32
U = 2.0 ** -24
LOG_U, LOG1P_U, POW_U, DIV_U = 6.0, 4.0, 32.0, 5.0
SECOND_ORDER = 1.0 + 2.0 ** -10
ABS_FLOOR = 2.0 ** -140
# the new kernel's constants (csrc/pr_focal.hip)
THREADS, PER_THREAD = 256, 8          # kPrThreads, kPrPerThread
BLOCK = THREADS * PER_THREAD          # elements of one workgroup of the main pass
FINISH_THREADS = 1024                 # pr_focal_finish_kernel: partial[i], i += 1024, then a 10-level tree
COUNT_CHUNK = 256 * 4 * 4             # kPrCountChunk: elements of one workgroup trip of the count pass
COUNT_BLOCKS = 256                    # kPrCountBlocks: workgroups of the count pass at most

DEFAULTS = dict(alpha=2.0, beta=4.0, eps=1e-4, positive=1.0)
PARAMS = ((2.0, 4.0), (0.0, 0.0), (1.0, 1.0), (2.5, 3.5), (3.0, 0.0))     # (alpha, beta)
POSITIVES = (1.0, 0.85)
TAIL_SIZES = (1, 3, 4, 5, 7, 8, 9, 2047, 2048, 2049, 2051, 4099)


def bounds(eps):
    """-> (lo, hi) as float32: lo = float32(eps), hi = float32(1) - lo"""
    lo = F32(eps)
    return lo, F32(F32(1.0) - lo)


def _mode(e):
    return int(e) if float(e) in (0.0, 1.0, 2.0, 3.0, 4.0) else -1


def terms64(p, t, alpha, beta, lo, hi, positive):
    """the rule in float64 on float64 arrays -> (l, dl/dp, is positive, gate open)"""
    p, t = np.asarray(p, F64), np.asarray(t, F64)
    lo, hi, positive = float(lo), float(hi), float(positive)
    with np.errstate(all="ignore"):
        q = np.where(p < lo, lo, np.where(p > hi, hi, p))        # (a NaN stays)
        opened = (p >= lo) & (p <= hi)
        pos = t >= positive
        a = np.where(pos, 1.0 - q, q)
        b = np.where(pos, q, 1.0 - q)
        lg = np.where(pos, np.log(q), np.log1p(-q))
        w = np.where(pos, 1.0, np.power(np.where(pos, 0.0, 1.0 - t), beta))    # 0^0 = 1
        aa = np.power(a, alpha)
        second = alpha * w * np.power(a, alpha - 1.0) * lg if alpha != 0.0 else 0.0
        mag = w * aa / b - second
        l = -w * aa * lg
    return l, np.where(opened, np.where(pos, -mag, mag), 0.0), pos, opened


def rel_units(pos, alpha, beta):
    """-> (units of U of the loss term, of the gradient) per element, from the tally of the module docstring"""
    pos = np.asarray(pos, bool)
    am, bm = _mode(alpha), _mode(beta)
    pa = pos.astype(F64)                  # a = fl(1 - q) is rounded for a positive
    pb = 1.0 - pa                         # b = fl(1 - q) otherwise
    e_w = np.where(pos, 0.0, beta * 1.0 + ((0, 0, 1, 2, 2)[bm] if bm >= 0 else POW_U))
    e_aa = alpha * pa + ((0, 0, 1, 2, 3)[am] if am >= 0 else POW_U)
    if am >= 0:
        e_a1 = abs(alpha - 1.0) * pa + (0, 0, 0, 1, 2)[am]
    else:
        e_a1 = e_aa + pa + DIV_U
    log_u = np.where(pos, LOG_U, LOG1P_U)
    rel_l = e_w + e_aa + 1 + log_u + 1
    term1 = e_w + e_aa + 1 + pb + DIV_U
    term2 = (e_w + e_a1 + 1 + 1 + log_u + 1) if alpha != 0.0 else np.zeros(pos.shape)
    rel_g = np.maximum(term1, term2) + 1 + 1 + 2 + 1 + 1
    return rel_l, rel_g


def blocks_of(n):
    return (n + BLOCK - 1) // BLOCK


def loss_depth(n, heads=0):
    """float32 roundings on the longest path from a loss term to the loss, written out from csrc/pr_focal.hip:
    8 per thread (sum += le), 6 wave shuffles, 2 for the workgroup ((r0 + r1) + (r2 + r3)), ceil(blocks / 1024) strided
    additions per finish thread, 10 levels of the LDS tree, 1 for the product with 1 / denom and 2 for 1 / denom itself
    (the conversion of the count and the division); for the mean over heads `heads` additions, the product with
    1 / heads and that factor's own rounding."""
    mean = heads + 2 if heads else 0
    return PER_THREAD + 6 + 2 + -(-blocks_of(n) // FINISH_THREADS) + 10 + 1 + 2 + mean


Expected = namedtuple("Expected", "n n_pos denom heads want lo hi closed nan l_want l_lo l_hi loss")


def expected(pred32, target32, alpha=2.0, beta=4.0, eps=1e-4, positive=1.0, heads=1):
    """What one head must give: pred / target float32 of any (equal) shape; the gradient is d (mean over `heads`
    heads) / d pred.  want / lo / hi: the gradient and its interval per element (signed); closed: the gate is shut
    (exactly +0.0 is due); nan: pred is NaN there; loss: (want, lo, hi) of the head's own value."""
    p, t = np.asarray(pred32), np.asarray(target32)
    assert p.dtype == F32 and t.dtype == F32 and p.shape == t.shape
    p, t = p.ravel(), t.ravel()
    alpha, beta, positive = float(F32(alpha)), float(F32(beta)), float(F32(positive))
    lo, hi = bounds(eps)
    l, dq, pos, opened = terms64(p.astype(F64), t.astype(F64), alpha, beta, lo, hi, positive)
    n_pos = int(pos.sum())
    denom = max(n_pos, 1)
    rel_l, rel_g = rel_units(pos, alpha, beta)
    want = dq / denom / heads
    room = np.abs(want) * rel_g * U * SECOND_ORDER + ABS_FLOOR
    room = np.where(opened, room, 0.0)
    l_room = np.abs(l) * rel_l * U * SECOND_ORDER + ABS_FLOOR
    l_lo, l_hi = np.maximum(l - l_room, 0.0), l + l_room
    gm = higham_gamma(loss_depth(p.size))
    loss = (float(l.sum()) / denom, float(l_lo.sum()) / denom * (1.0 - gm), float(l_hi.sum()) / denom * (1.0 + gm))
    return Expected(p.size, n_pos, denom, heads, want, want - room, want + room, ~opened & ~np.isnan(p), np.isnan(p),
                    l, l_lo, l_hi, loss)


def mean_bound(exps):
    """(want, lo, hi) of loss[0] from the heads' own bounds: their sum times 1 / heads, widened by the mean's roundings"""
    heads = len(exps)
    gm = higham_gamma(heads + 2)
    return (sum(e.loss[0] for e in exps) / heads, sum(e.loss[1] for e in exps) / heads * (1.0 - gm),
            sum(e.loss[2] for e in exps) / heads * (1.0 + gm))


def loss_ratio(got, bound):
    """(got - want) / (room on got's side); inside <=> <= 1"""
    want, lo, hi = bound
    got = float(got)
    if not np.isfinite(got):
        return float("inf")
    if got == want:
        return 0.0
    room = (hi - want) if got > want else (want - lo)
    return abs(got - want) / room if room > 0 else float("inf")


def grad_ratio(got32, exp):
    got = np.asarray(got32).astype(F64).ravel()
    assert got.shape == exp.want.shape
    with np.errstate(all="ignore"):
        room = np.where(got >= exp.want, exp.hi - exp.want, exp.want - exp.lo)
        err = np.abs(got - exp.want)
        r = np.where(err == 0.0, 0.0, err / room)
    r[~np.isfinite(got)] = np.inf
    r[np.isnan(r)] = np.inf
    r[exp.nan] = 0.0                   # unspecified there
    return r


def check(exp, grad32, n_pos, loss):
    """-> list of complaints about one head's result (empty: everything holds).  grad32: float32 of n elements or None;
    n_pos: an integer or None (not checked); loss: the head's value or None (not checked)."""
    bad = []
    if n_pos is not None and int(n_pos) != exp.n_pos:
        bad.append("n_pos is %d, want %d" % (int(n_pos), exp.n_pos))
    if grad32 is not None:
        g = np.asarray(grad32)
        assert g.dtype == F32
        g = g.ravel()
        stale = np.flatnonzero((g.view(U32) != 0) & exp.closed)
        if stale.size:
            i = int(stale[0])
            bad.append("%d gradients behind a closed gate are not +0.0; first at %d: %r (bits %#x)"
                       % (stale.size, i, g[i], int(g.view(U32)[i])))
        r = grad_ratio(g, exp)
        out = np.flatnonzero(r > 1.0)
        if out.size:
            i = int(out[np.argmax(r[out])])
            bad.append("%d of %d gradients outside their interval; worst at %d: got %r, want %r in [%r, %r] (ratio %.3g)"
                       % (out.size, g.size, i, float(g[i]), exp.want[i], exp.lo[i], exp.hi[i], r[i]))
    if loss is not None:
        if exp.nan.any():
            if not np.isnan(float(loss)):
                bad.append("a NaN in pred is hidden: loss %r" % float(loss))
        else:
            ratio = loss_ratio(loss, exp.loss)
            if not ratio <= 1.0:
                bad.append("loss %r outside [%r, %r] (want %r, ratio %.3g)" % (float(loss), exp.loss[1], exp.loss[2],
                                                                               exp.loss[0], ratio))
    return bad


def check_all(preds, target, result, **params):
    """every head of (loss [1 + heads], grads or None, n_pos) against the oracle, and loss[0] against the mean's bound"""
    loss, grads, n_pos = result
    bad, exps = [], []
    for h, p in enumerate(preds):
        exp = expected(p, target, heads=len(preds), **params)
        exps.append(exp)
        bad += ["head %d: %s" % (h, m) for m in check(exp, None if grads is None else grads[h], n_pos, loss[1 + h])]
    if not any(e.nan.any() for e in exps):
        ratio = loss_ratio(loss[0], mean_bound(exps))
        if not ratio <= 1.0:
            bad.append("mean over heads %r outside its bound %r (ratio %.3g)" % (float(loss[0]), mean_bound(exps), ratio))
    elif not np.isnan(float(loss[0])):
        bad.append("a NaN in pred is hidden in the mean: %r" % float(loss[0]))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's arithmetic restated in float32 torch (pr_element, the workgroup partials and the finish), with the
# mutations the host tests plant.  Same operations on the same float32 values; the order INSIDE a workgroup sum and
# inside the finish is torch's, which the loss bound covers.
MUTATIONS = ("weight_dropped", "gate_ignored", "denominator_counts_all_pixels", "positive_is_strictly_greater",
             "inv_heads_twice", "zero_positives_divide_by_zero", "plain_log_of_one_minus_q")


def _pow_f32(x, mode, e, pair):
    """pr_pow / pr_pow_pair on a float32 tensor -> x^e, or (x^(e-1), x^e)"""
    import torch
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    if mode == 0:
        xm1, xe = zero, one
    elif mode == 1:
        xm1, xe = one, x
    elif mode == 2:
        xm1, xe = x, x * x
    elif mode == 3:
        xm1 = x * x
        xe = xm1 * x
    elif mode == 4:
        if pair:
            xm1 = (x * x) * x
            xe = xm1 * x
        else:
            xm1, xe = None, (x * x) * (x * x)
    else:
        xe = torch.pow(x, torch.tensor(e, dtype=torch.float32))
        xm1 = xe / x
    return (xm1, xe) if pair else xe


def restate_f32(preds32, target32, alpha=2.0, beta=4.0, eps=1e-4, positive=1.0, mutation=None):
    """-> (loss float32 [1 + heads], [grad float32 [n]] per head, n_pos int) as the kernel forms them"""
    import torch
    assert mutation is None or mutation in MUTATIONS
    heads = len(preds32)
    t = torch.from_numpy(np.array(target32, dtype=F32).ravel())
    n = t.numel()
    lo32, hi32 = bounds(eps)
    lo, hi = torch.tensor(float(lo32)), torch.tensor(float(hi32))
    alpha32 = torch.tensor(float(alpha), dtype=torch.float32)
    positive32 = torch.tensor(float(positive), dtype=torch.float32)
    pos = (t > positive32) if mutation == "positive_is_strictly_greater" else (t >= positive32)
    n_pos = int(pos.sum())
    denom = n if mutation == "denominator_counts_all_pixels" else (n_pos if mutation == "zero_positives_divide_by_zero"
                                                                   else max(n_pos, 1))
    with np.errstate(all="ignore"):
        inv_denom = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(denom), dtype=torch.float32)
    inv_heads = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(heads), dtype=torch.float32)
    w = torch.where(pos, torch.ones_like(t), _pow_f32(1.0 - t, _mode(beta), float(beta), pair=False))
    if mutation == "weight_dropped":
        w = torch.ones_like(t)
    losses, grads = [], []
    for p_np in preds32:
        p = torch.from_numpy(np.array(p_np, dtype=F32).ravel())
        q = torch.where(p < lo, lo, torch.where(p > hi, hi, p))
        opened = (p >= lo) & (p <= hi)
        omq = 1.0 - q
        log_neg = torch.log(omq) if mutation == "plain_log_of_one_minus_q" else torch.log1p(-q)
        lg = torch.where(pos, torch.log(q), log_neg)
        a, b = torch.where(pos, omq, q), torch.where(pos, q, omq)
        a1, aa = _pow_f32(a, _mode(alpha), float(alpha), pair=True)
        wa = w * aa
        mag = wa / b - (alpha32 * (w * a1)) * lg
        g = (torch.where(pos, -mag, mag) * inv_denom) * inv_heads
        if mutation == "inv_heads_twice":
            g = g * inv_heads
        if mutation != "gate_ignored":
            g = torch.where(opened, g, torch.zeros_like(g))
        le = -wa * lg
        padded = torch.zeros(blocks_of(n) * BLOCK, dtype=torch.float32)
        padded[:n] = le
        losses.append(padded.view(-1, BLOCK).sum(1).sum() * inv_denom)
        grads.append(g.numpy())
    avg = torch.tensor(0.0, dtype=torch.float32)
    for v in losses:
        avg = avg + v
    return torch.stack([(1.0 * avg) * inv_heads] + losses).numpy(), grads, n_pos


# ---------------------------------------------------------------------------------------------------------------------
# Input sets.
def just_below(x):
    return np.nextafter(F32(x), F32(0.0))


def planted(eps, positive):
    """the 18 planted (p, t) pairs: p exactly 0, lo, nextafter(lo, 0), hi, nextafter(hi, 1), 1 against t exactly
    `positive`, the float32 just below it, and 0 -- ordered so that a short prefix already holds every p and every t"""
    lo, hi = bounds(eps)
    ps = [F32(0.0), lo, just_below(lo), hi, np.nextafter(hi, F32(1.0)), F32(1.0)]
    ts = [F32(positive), just_below(positive), F32(0.0)]
    return [(ps[(i + r) % 6], ts[i % 3]) for r in range(3) for i in range(6)]


def inputs(n, heads=1, seed=0, eps=1e-4, positive=1.0, positives=0.05, plant=True):
    """([pred_h [n]], target [n]) float32: random p in (0, 1), random t in [0, 1) of which a share `positives` is set to
    exactly `positive` (or above it, up to 1); the planted pairs at the front and, from n = 36 on, mirrored at the end
    (inside the scalar tail when n % 4 != 0), rotated by one per head"""
    rng = np.random.default_rng(5000 + 100 * seed + n)
    t = rng.random(n).astype(F32)
    centre = rng.random(n) < positives
    t[centre] = np.where(rng.random(int(centre.sum())) < 0.5, F32(positive),
                         F32(positive) + (F32(1.0) - F32(positive)) * rng.random(int(centre.sum())).astype(F32)).astype(F32)
    preds = []
    for h in range(heads):
        p = (rng.random(n).astype(F32) * F32(0.998) + F32(0.001)).astype(F32)
        if plant:
            pairs = planted(eps, positive)
            pairs = pairs[h % 18:] + pairs[:h % 18]
            for j, (pv, tv) in enumerate(pairs[:n]):
                p[j] = pv
                if h == 0:
                    t[j] = tv
            if n >= 36:
                for j, (pv, tv) in enumerate(pairs):
                    p[n - 1 - j] = pv
                    if h == 0:
                        t[n - 1 - j] = tv
        preds.append(p)     # (the planted targets are those of head 0; the other heads meet them with their rotated p)
    return preds, t


BIG_N = 1025 * BLOCK + 3    # 1026 workgroups: the finish takes a second trip; 513 count chunks on 256 workgroups: three trips
BIG_REGIONS = {"block0": (0, BLOCK), "block600": (600 * BLOCK, 601 * BLOCK), "block1023": (1023 * BLOCK, 1024 * BLOCK),
               "block1024": (1024 * BLOCK, 1025 * BLOCK), "last3": (BIG_N - 3, BIG_N)}


@functools.lru_cache(maxsize=None)
def region_inputs(region, count=300):
    """(pred, target) float32 [BIG_N]: p = 0 against t = 0 everywhere (a term of lo^alpha |log1p(-lo)|, about 1e-12 for
    the defaults) except `count` random elements (all three for "last3") inside ONE region, a quarter of them positives:
    the loss and every positive come from that region.  Read-only arrays, computed once per process."""
    lo, hi = BIG_REGIONS[region]
    rng = np.random.default_rng(7300 + sorted(BIG_REGIONS).index(region))
    p, t = np.zeros(BIG_N, F32), np.zeros(BIG_N, F32)
    idx = np.arange(lo, hi) if hi - lo <= count else lo + np.sort(rng.choice(hi - lo, count, replace=False))
    p[idx] = (rng.random(idx.size).astype(F32) * F32(0.998) + F32(0.001)).astype(F32)
    t[idx] = rng.random(idx.size).astype(F32)
    t[idx[::4]] = 1.0
    p.flags.writeable = t.flags.writeable = False
    return p, t
