"""FocalLoss_BCE_2d (csrc/caller.hip: focal_thread and its block / finish sums) as plain float64 numpy, with an a-priori
acceptance interval per element, a bound on the loss sum, the float32 restatement of the kernel that the host tests
mutate, and the input sets.  Shared by tests/test_loss_targets_host.py, tests/test_gpu_loss_targets.py and
tests/test_gpu_caller.py (test infrastructure; no GPU here).

The function, per element of (pred, target), with d = p - t:
    u = max(|d| - 1e-20, 0),  e = 1 - u,  loss term l(u) = -(u^gamma) log e,
    g(u) = u^gamma / e - gamma u^(gamma-1) log e,  gradient = sign(d) g(u) / rows,  loss = sum l / rows.
At u = 0: 0^0 = 1 (as torch has it), log e = 0, and gamma u^(gamma-1) log e is taken at its limit 0, so l(0) = 0 and
g(0) = 0^gamma; an exact hit (d = 0) has sign 0 and gradient exactly 0.

Error model of the kernel (the interval is derived from it, not from what the kernel returns):
  * It evaluates the exact formula at a perturbed u: fl(p - t) and fl(1 - |d|) round once each, each by at most half an
    ulp of a number <= 1 (2^-25); the + 1e-20f is absorbed unless 1 - |d| is 0; 1 - err is exact for err >= 0.5 and one
    more relative rounding below.  Hence |u_kernel - u| <= DELTA = 2^-23.
  * Everything after that is a relative rounding: about 14 fp32 operations, logf and powf at their documented accuracy:
    EPS = 16 * 2^-24.
  * l is increasing in u on (0, 1) for every gamma >= 0, g for gamma >= 1: the interval is the function at the ends of
    the u range, widened by EPS.  For gamma < 1, g is bracketed by its minimum and maximum over a 9-point grid.
  * |d| == 1 exactly: d = +-1, err = float32(1e-20), u = 1 are exact in the kernel: EPS only.
  * The loss sum: the kernel's fixed order has at most loss_depth() fp32 additions on its longest path; all terms are
    non-negative, so [sum lo_i, sum hi_i] widened by gamma(depth) (tests/helpers.gamma) is a relative bound.
"""
import functools
from collections import namedtuple

import numpy as np

from tests.helpers import gamma as higham_gamma

F32, F64 = np.float32, np.float64
TINY = F64(F32(1e-20))          # the kernel's 1e-20f
DELTA = 2.0 ** -23
EPS = 16 * 2.0 ** -24
LOSS_THREADS, LOSS_PER_THREAD = 256, 8
BLOCK = LOSS_THREADS * LOSS_PER_THREAD   # elements per block of focal_bce_kernel
FINISH_THREADS = 1024                    # focal_bce_finish_kernel: partial[i], i += 1024, then a 10-level tree
MAX_D = 1.0 - 2.0 ** -10                 # |d| of every random element of the input sets is at most this


def _l_and_g(u, gamma):
    """l(u) and g(u) in float64 for u in [0, 1]; at u = 1 (exactly) e is the kernel's float32(1e-20)"""
    u = np.asarray(u, dtype=F64)
    with np.errstate(all="ignore"):
        e = np.where(u >= 1.0, TINY, 1.0 - u)
        # (log1p for small u, where 1 - u in float64 would lose the low bits of u; plain log above 0.5)
        log_e = np.where(u > 0.5, np.log(e), np.log1p(-np.minimum(u, 0.5)))
        ug = np.power(u, gamma)                              # 0^0 = 1
        second = np.where(u > 0.0, gamma * np.power(np.where(u > 0.0, u, 1.0), gamma - 1.0) * log_e, 0.0)
    return -ug * log_e + 0.0, ug / e - second


Terms = namedtuple("Terms", "d u loss_term grad")
Interval = namedtuple("Interval", "d want lo hi l_want l_lo l_hi hit unit rows")


def _d_and_u(pred32, target32):
    p = np.asarray(pred32)
    t = np.asarray(target32)
    assert p.dtype == F32 and t.dtype == F32 and p.shape == t.shape
    d = p.astype(F64).ravel() - t.astype(F64).ravel()
    assert float(np.abs(d).max(initial=0.0)) <= 1.0, "the loss is defined for |pred - target| <= 1"
    u = np.maximum(np.abs(d) - 1e-20, 0.0)      # (float64 absorbs the 1e-20 except at 0: |d| = 1 gives u = 1.0, e = TINY)
    return d, u


def focal_terms(pred32, target32, gamma, rows):
    """float32 operands -> per element, in float64: d, u, the loss term l(u) and the gradient sign(d) g(u) / rows"""
    d, u = _d_and_u(pred32, target32)
    l, g = _l_and_g(u, float(gamma))
    return Terms(d, u, l, np.sign(d) * g / rows)


def focal_interval(pred32, target32, gamma, rows):
    """The acceptance interval of every gradient element ([lo, hi], signed) and of every loss term ([l_lo, l_hi], not yet
    divided by rows), with the float64 values themselves (want, l_want)."""
    gamma = float(gamma)
    d, u = _d_and_u(pred32, target32)
    hit, unit = d == 0.0, np.abs(d) == 1.0
    l, g = _l_and_g(u, gamma)
    u_lo = np.where(unit, 1.0, np.maximum(u - DELTA, 0.0))
    u_hi = np.where(unit, 1.0, np.minimum(u + DELTA, 1.0))
    l_lo, g_lo = _l_and_g(u_lo, gamma)
    l_hi, g_hi = _l_and_g(u_hi, gamma)
    if gamma < 1.0:     # g need not be monotonic: bracket it over a grid (the ends included)
        grid = np.stack([_l_and_g(u_lo + (u_hi - u_lo) * (k / 8.0), gamma)[1] for k in range(9)])
        g_lo, g_hi = grid.min(0), grid.max(0)
    g_lo, g_hi = g_lo * (1.0 - EPS) / rows, g_hi * (1.0 + EPS) / rows
    sgn = np.sign(d)
    lo = np.where(sgn > 0, g_lo, np.where(sgn < 0, -g_hi, 0.0))
    hi = np.where(sgn > 0, g_hi, np.where(sgn < 0, -g_lo, 0.0))
    return Interval(d, sgn * g / rows, lo, hi, l, l_lo * (1.0 - EPS), l_hi * (1.0 + EPS), hit, unit, rows)


def grad_ratio(got32, iv):
    """per element (got - want) / (distance from want to the end of the interval on got's side): inside <=> <= 1.
    A NaN or an element outside a zero-width interval is infinite."""
    got = np.asarray(got32).astype(F64).ravel()
    assert got.shape == iv.want.shape
    with np.errstate(all="ignore"):
        room = np.where(got >= iv.want, iv.hi - iv.want, iv.want - iv.lo)
        err = np.abs(got - iv.want)
        r = np.where(err == 0.0, 0.0, err / room)
    r[~np.isfinite(got)] = np.inf
    r[np.isnan(r)] = np.inf
    return r


def check_grad(got32, iv, where=None):
    """-> (list of complaints, worst ratio).  Inside the interval, the sign of d exactly, exactly 0.0 at exact hits.
    where: boolean mask of the elements to check (default: all)."""
    got = np.asarray(got32).astype(F64).ravel()
    r = grad_ratio(got32, iv)
    keep = np.ones(r.shape, bool) if where is None else np.asarray(where).ravel()
    bad = []
    out = np.flatnonzero((r > 1.0) & keep)
    if out.size:
        i = int(out[np.argmax(r[out])])
        bad.append("%d of %d gradients outside their interval; worst at %d: got %r, want %r in [%r, %r], d = %r"
                   % (out.size, int(keep.sum()), i, got[i], iv.want[i], iv.lo[i], iv.hi[i], iv.d[i]))
    with np.errstate(invalid="ignore"):
        wrong_sign = np.flatnonzero((np.sign(got) != np.sign(iv.d)) & keep)
    if wrong_sign.size:
        i = int(wrong_sign[0])
        bad.append("%d gradients with a sign other than sign(d); first at %d: got %r, d = %r" % (wrong_sign.size, i, got[i], iv.d[i]))
    nz = np.flatnonzero(iv.hit & keep & (got != 0.0))
    if nz.size:
        bad.append("%d exact hits with a gradient other than 0.0; first at %d: %r" % (nz.size, int(nz[0]), got[nz[0]]))
    return bad, float(r[keep].max(initial=0.0))


def loss_blocks(n):
    return (n + BLOCK - 1) // BLOCK


def loss_depth(n, heads=0):
    """fp32 additions on the longest path from a loss term to the loss, written out from csrc/caller.hip:
    8 per thread (sum += le), 6 wave shuffles, 3 for the block ((r0 + r1) + (r2 + r3), then the product with 1 / rows),
    ceil(blocks / 1024) strided additions per finish thread, 10 levels of the LDS tree, and `heads` for the mean over
    heads (avg = avg + loss_h, then the product with 1 / heads)."""
    return LOSS_PER_THREAD + 6 + 3 + -(-loss_blocks(n) // FINISH_THREADS) + 10 + heads


def loss_bound(iv, heads=0):
    """-> (want, lo, hi) of the loss sum l / rows: the element intervals summed, widened by gamma(depth)"""
    n = iv.want.size
    gm = higham_gamma(loss_depth(n, heads))
    return (float(iv.l_want.sum()) / iv.rows, float(iv.l_lo.sum()) / iv.rows * (1.0 - gm),
            float(iv.l_hi.sum()) / iv.rows * (1.0 + gm))


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


# ---------------------------------------------------------------------------------------------------------------------
# The kernel's arithmetic restated in float32 torch (focal_thread, the block partials and the finish), with the
# mutations the host tests plant.  Same operations on the same float32 values; the order INSIDE a block sum and inside
# the finish differs from the kernel's (torch's sum), which the loss bound covers.
MUTATIONS = ("log_term_dropped", "sign_flipped_for_negative_d", "inv_rows_twice", "tail_gradient_left_zero",
             "loss_misses_one_block", "loss_misses_partials_from_1024")


def restate_f32(pred32, target32, gamma, rows, mutation=None, drop_block=0):
    """-> (loss float32 scalar, gradient float32 [n]) as the kernel forms them; mutation: one of MUTATIONS or None"""
    import torch
    assert mutation is None or mutation in MUTATIONS
    p = torch.from_numpy(np.array(pred32, dtype=F32).ravel())
    t = torch.from_numpy(np.array(target32, dtype=F32).ravel())
    n = p.numel()
    gm = torch.tensor(float(gamma), dtype=torch.float32)
    inv_rows = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(rows), dtype=torch.float32)
    d = p - t
    err = (1.0 - d.abs()) + torch.tensor(1e-20, dtype=torch.float32)
    u = 1.0 - err
    lg = torch.log(err)
    ug1 = u * u if float(gamma) == 3.0 else torch.pow(u, gm - 1.0)
    ug = ug1 * u
    le = -ug * lg
    first = gm * ug1 * lg
    if mutation == "log_term_dropped":
        first = torch.zeros_like(first)
    dl_de = first - ug / err
    if float(gamma) < 1.0:   # u == 0: u^(gamma-1) is inf; 0^0 = 1, the log term at its limit 0
        zero = u == 0
        le = torch.where(zero, torch.zeros_like(le), le)
        dl_de = torch.where(zero, -torch.full_like(u, 1.0 if float(gamma) == 0.0 else 0.0) / err, dl_de)
    sgn = torch.sign(d)
    if mutation == "sign_flipped_for_negative_d":
        sgn = sgn.abs()
    g = (-dl_de * sgn * inv_rows) * 1.0
    if mutation == "inv_rows_twice":
        g = g * inv_rows
    if mutation == "tail_gradient_left_zero" and n % 4:
        g[n - n % 4:] = 0.0
    blocks = loss_blocks(n)
    padded = torch.zeros(blocks * BLOCK, dtype=torch.float32)
    padded[:n] = le
    partial = padded.view(blocks, BLOCK).sum(1) * inv_rows
    if mutation == "loss_misses_one_block":
        partial[drop_block] = 0.0
    if mutation == "loss_misses_partials_from_1024":
        partial = partial[:FINISH_THREADS]
    return partial.sum(), g.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# Input sets.  Every element is an exact hit, an exact |d| = 1, or has |d| <= MAX_D = 1 - 2^-10 (so u + DELTA stays
# clear of the pole at u = 1 and the intervals stay narrow: the host tests assert the median width).
TAIL_SIZES = (1, 3, 4, 5, 7, 8, 9, 2047, 2048, 2049, 2051, 4099)
BIG_N = 1025 * BLOCK + 5                         # 1026 blocks: the finish kernels' strided loop takes a second trip
BIG_REGIONS = {"block0": (0, BLOCK), "block1023": (1023 * BLOCK, 1024 * BLOCK), "block1024": (1024 * BLOCK, 1025 * BLOCK),
               "last5": (BIG_N - 5, BIG_N)}


def _random_pred(rng, t):
    """a random float32 pred for the float32 target t: never an exact hit, |d| <= MAX_D"""
    p = rng.random(t.size).astype(F32)
    p[np.abs(p.astype(F64) - t.astype(F64)) > MAX_D] = F32(0.5)
    same = p == t
    p[same] = np.where(t[same] < 0.5, t[same] + F32(0.25), t[same] - F32(0.25))
    return p


def _plant(p, t):
    """where n allows: d = -1 at 0, an exact hit at 1, d = +1 at n - 1 (inside the scalar tail when n % 4 != 0), further
    hits at n // 2 and n - 2"""
    n = p.size
    if n >= 3:
        t[0], p[0] = 1.0, 0.0
        p[1] = t[1]
        t[n - 1], p[n - 1] = 0.0, 1.0
    if n >= 7:
        p[n // 2] = t[n // 2]
    if n >= 2047:
        p[n - 2] = t[n - 2]
    return p, t


def tail_inputs(n, seed=0):
    """(pred, target) float32 [n]: random elements and the planted ones of _plant"""
    rng = np.random.default_rng(1000 * seed + n)
    t = rng.random(n).astype(F32)
    return _plant(_random_pred(rng, t), t)


def heads_inputs(heads, n, seed=0):
    """([pred_h], target): one target, `heads` different preds, every pair an input set like tail_inputs"""
    preds, t = [], None
    for h in range(heads):
        if t is None:
            p, t = tail_inputs(n, seed)
        else:
            p, _ = _plant(_random_pred(np.random.default_rng(1000 * seed + n + 77 * h), t), t)
        preds.append(p)
    return preds, t


@functools.lru_cache(maxsize=None)
def region_inputs(region, seed=0, count=300):
    """(pred, target) float32 [BIG_N]: pred == target everywhere except `count` random elements (all five for
    "last5") inside ONE region, so the whole loss comes from that region.  The target depends on the seed alone.
    Read-only arrays, computed once per process."""
    lo, hi = BIG_REGIONS[region]
    t = np.random.default_rng(7000 + seed).random(BIG_N).astype(F32)
    rng = np.random.default_rng(7100 + 10 * seed + sorted(BIG_REGIONS).index(region))
    p = t.copy()
    idx = np.arange(lo, hi) if hi - lo <= count else lo + np.sort(rng.choice(hi - lo, count, replace=False))
    p[idx] = _random_pred(rng, t[idx])
    p.flags.writeable = t.flags.writeable = False    # (cached: shared among the tests)
    return p, t


def caller_inputs(shape):
    """the inputs of tests/test_gpu_caller.py::test_focal_loss_value_and_gradient (torch generator, planted hits and one
    |d| = 1), as float32 numpy of that shape"""
    import torch
    g = torch.Generator().manual_seed(3)
    pred = torch.rand(shape, generator=g) * 0.98 + 0.01
    target = torch.rand(shape, generator=g)
    pred[0, 0, 0, :3] = target[0, 0, 0, :3]
    target[0, 1, 1, 0], pred[0, 1, 1, 0] = 1.0, 0.0
    return pred.numpy(), target.numpy()


# ---------------------------------------------------------------------------------------------------------------------
# Heat maps: error in float32 ulps of the oracle's value
def ulps(got32, want32):
    """|got - want| in units of the float32 spacing at |want| (numpy float32 arrays)"""
    got, want = np.asarray(got32), np.asarray(want32)
    assert got.dtype == F32 and want.dtype == F32 and got.shape == want.shape
    with np.errstate(all="ignore"):
        r = np.abs(got.astype(F64) - want.astype(F64)) / np.spacing(np.abs(want)).astype(F64)
    r[~np.isfinite(got)] = np.inf
    return r
