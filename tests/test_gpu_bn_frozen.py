"""The backward of a frozen BatchNorm layer (unetpp_bn_frozen_bwd, unetpp_bn_frozen_bwd_bf16 and the coefficient launch
unetpp_bn_eval_coeffs_stats) against float64, in the manner of tests/test_gpu_streaming.py: every case restates the
launcher's own conditions (C % 4, 16-byte alignment, bn_bwd_pool_ok, octets_ok, the grid formulas), asserts the label the
launcher reports, and the last test checks that every label ran and every capped form ran above its cap with a remainder.

With u = 2^-24, g = d_act (+ the pooled gradient where the pixel won its window), gg = (fma(y, scale, shift) > 0) ? g : 0:
    dy = gg * scale            one add (routed) and one product, each rounded once: |dy - ref| <= gamma_2 |gg scale|;
                               bf16: close_bf16.  In place == out of place, and partial == NULL == with sums, bit for bit
    dbeta  = sum gg            |dbeta - ref|  <= gamma_(n+2) sum |gg|
    dgamma = sum gg xhat       |dgamma - ref| <= gamma_(n+5) sum |gg xhat|, xhat = (y - mean) invstd; n = fp32 additions of a
                               partial row (iterations per thread + threads summed per channel, from the launcher formulas;
                               unetpp_bn_bwd_finalize adds the rows in float64)
No gate argument lies within 8 u of zero (asserted), so the reference alone decides every gate.
(b) exact arithmetic above the grid caps: small-integer operands, power-of-two scale / invstd, integer mean, shift = integer
+ 1/2; every partial sum is exact in fp32 in any order (asserted), so dbeta and dgamma must EQUAL the float64 result.
"""
import ctypes

import pytest
import torch

from tests.helpers import U32, bound_ratio, close_bf16, gamma, report_ratio
from tests.stream_rules import (FROZEN_CAP, K_THREADS, al16, bn_bwd_pool_ok, fin_threads, frozen_blocks, frozen_blocks_bf16,  # noqa: F401
                                frozen_blocks_for, octets_ok, ref_route, shifted, windows)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GATE_MARGIN = 8 * U32
GRID = 2.0 ** 24
EVAL_DIV_SQRT_ULPS = 2.0          # as tests/test_gpu_streaming.py: sqrtf and the fp32 division, in u each (an estimate)

COVERAGE = [
    "bn_eval_coeffs/stats",
    "bn_frozen_bwd<4>", "bn_frozen_bwd<4>/sums", "bn_frozen_bwd<1>", "bn_frozen_bwd<1>/sums",
    "bn_frozen_bwd_pool", "bn_frozen_bwd_pool/sums",
    "bn_frozen_bwd_bf16", "bn_frozen_bwd_bf16/sums", "bn_frozen_bwd_bf16/pool", "bn_frozen_bwd_bf16/pool/sums",
]
FAMILIES = ("bn_frozen_bwd<4>", "bn_frozen_bwd<1>", "bn_frozen_bwd_pool", "bn_frozen_bwd_bf16")
SEEN = set()
ABOVE_CAP = set()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def L():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib.lib()


def ran(expect):
    name = L().unetpp_last_kernel_name().decode()
    assert name == expect, (name, expect)
    SEEN.add(name)
    return name


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------- the launcher's conditions, restated
def plan(n, h, w, c, form):
    """(adds, items or rows of the launch, items or rows one pass of the grid covers) of a form."""
    pixels = n * h * w
    if form == "bf16":
        cg = c // 8
        span = frozen_blocks_bf16(pixels, c) * K_THREADS
        return -(-pixels * cg // span) + K_THREADS // cg, pixels * cg, span
    if form == "pool":
        cg = c // 4
        grid = min(n * h, frozen_blocks(pixels, c))
        return -(-n * h // grid) * -(-w * cg // K_THREADS) + K_THREADS // cg, n * h, grid
    cg = c // 4 if form == "vec" else c
    span = frozen_blocks_for(pixels, c, form == "vec") * K_THREADS
    return -(-pixels * cg // span) + -(-K_THREADS // cg), pixels * cg, span


# ------------------------------------------------------------------------------- one launch through the C ABI
def run_frozen(d_act, y, co, pool=None, in_place=False, sums=True):
    """-> (dgamma, dbeta, dy, form); the label of the launch (and of the finalize) asserted from the restated conditions."""
    lib = L()
    n, h, w, c = y.shape
    pixels = n * h * w
    dev = y.device
    bf = y.dtype == BF
    dy = d_act if in_place else torch.full_like(d_act, float("nan"))
    dp, pi = pool if pool is not None else (None, None)
    if bf:
        assert octets_ok(c)
        blocks = int(lib.unetpp_bn_frozen_bwd_blocks_bf16(pixels, c))
        assert blocks == frozen_blocks_bf16(pixels, c)
        fn, form = lib.unetpp_bn_frozen_bwd_bf16, "bf16"
        label = "bn_frozen_bwd_bf16" + ("/pool" if pool is not None else "")
    else:
        blocks = int(lib.unetpp_bn_frozen_bwd_blocks(pixels, c))
        assert blocks == frozen_blocks(pixels, c)
        assert bool(lib.unetpp_bn_bwd_pool_ok(n, h, w, c)) == bn_bwd_pool_ok(n, h, w, c)
        fn = lib.unetpp_bn_frozen_bwd
        if pool is not None:
            assert bn_bwd_pool_ok(n, h, w, c) and al16(d_act) and al16(y) and al16(dy) and al16(co["scale"]) and al16(co["shift"])
            form, label = "pool", "bn_frozen_bwd_pool"
        else:
            vec = c % 4 == 0 and al16(d_act) and al16(y) and al16(dy)
            form, label = ("vec", "bn_frozen_bwd<4>") if vec else ("scalar", "bn_frozen_bwd<1>")
    partial = torch.full((blocks * c * 2,), float("nan"), device=dev) if sums else None
    rc = fn(ptr(d_act), ptr(y), ptr(co["scale"]), ptr(co["shift"]), ptr(co["mean"]) if sums else None,
            ptr(co["invstd"]) if sums else None, ptr(dp), ptr(pi), n, h, w, c, ptr(dy), ptr(partial), stream())
    assert rc == 0, rc
    ran(label + ("/sums" if sums else ""))
    dgamma = dbeta = None
    if sums:
        dgamma, dbeta = (torch.full((c,), float("nan"), device=dev) for _ in range(2))
        assert lib.unetpp_bn_bwd_finalize(ptr(partial), blocks, c, ptr(dgamma), ptr(dbeta), stream()) == 0
        assert L().unetpp_last_kernel_name().decode() == "bn_bwd_finalize/%d" % fin_threads(blocks)
    torch.cuda.synchronize()
    _, count, span = plan(n, h, w, c, form)
    family = label[:-5] if label.endswith("/pool") else label
    if span >= FROZEN_CAP * (1 if form == "pool" else K_THREADS) and count > span and count % span:
        ABOVE_CAP.add(family)
    return dgamma, dbeta, dy, form


class Ref:
    """float64 statement from the same fp32 / bf16 numbers, on the tensors' device."""

    def __init__(self, grad64, y, co):
        c = y.shape[3]
        y64 = y.double()
        sc, sh, mu, is_ = (co[k].double() for k in ("scale", "shift", "mean", "invstd"))
        arg = y64 * sc + sh
        self.margin = float((arg.abs() / ((y64 * sc).abs() + sh.abs())).min())
        self.gg = torch.where(arg > 0, grad64, torch.zeros_like(grad64))
        prod = self.gg * ((y64 - mu) * is_)
        flat = lambda t: t.reshape(-1, c).sum(0)   # noqa: E731
        self.dbeta, self.dgamma = flat(self.gg), flat(prod)
        self.abs_beta, self.abs_gamma = flat(self.gg.abs()), flat(prod.abs())
        self.dy = self.gg * sc


def operands(g, n, h, w, c, bf):
    """Random operands of a frozen layer (running statistics unrelated to the batch) whose gate arguments all stay
    GATE_MARGIN away from zero (moved by 1/4 where they did not)."""
    y = torch.randn(n, h, w, c, generator=g) * 1.5 + 0.2
    y = y.to(BF) if bf else y
    mean = 0.5 * torch.randn(c, generator=g)
    var = 0.5 + 1.5 * torch.rand(c, generator=g)
    invstd = (1.0 / torch.sqrt(var.double() + 1e-5)).float()
    gam = 1 + 0.1 * torch.randn(c, generator=g)
    bet = 0.1 * torch.randn(c, generator=g)
    scale = (gam * invstd)
    co = {"invstd": invstd, "mean": mean, "scale": scale, "shift": bet - mean * scale}
    arg = y.double() * co["scale"].double() + co["shift"].double()
    near = arg.abs() <= 64 * GATE_MARGIN * ((y.double() * co["scale"].double()).abs() + co["shift"].double().abs())
    y = torch.where(near, (y.float() + 0.25).to(y.dtype), y)
    return y, co


def exact_operands(g, n, h, w, c, bf):
    """Small integers; scale in {1, 2, 4} and shift = integer + 1/2 (every gate argument is a half-integer), integer mean,
    power-of-two invstd: every product and every partial sum is exact in fp32 and in bf16 storage."""
    y = torch.randint(-4, 5, (n, h, w, c), generator=g).float()
    co = {"scale": 2.0 ** torch.randint(0, 3, (c,), generator=g).float(),
          "shift": torch.randint(-3, 3, (c,), generator=g).float() + 0.5,
          "mean": torch.randint(-2, 3, (c,), generator=g).float(),
          "invstd": 2.0 ** torch.randint(-1, 2, (c,), generator=g).float()}
    d_act = torch.randint(-3, 4, (n, h, w, c), generator=g).float() * (torch.rand(n, h, w, c, generator=g) < 0.25)
    return (y.to(BF) if bf else y), co, (d_act.to(BF) if bf else d_act)


def make_pool(g, n, h, w, c, bf, dev, exact=False):
    if exact:
        d_pooled = torch.randint(-3, 4, (n, h // 2, w // 2, c), generator=g).float()
        d_pooled = d_pooled * (torch.rand(d_pooled.shape, generator=g) < 0.25)
    else:
        d_pooled = torch.randn(n, h // 2, w // 2, c, generator=g)
    d_pooled = d_pooled.to(BF) if bf else d_pooled
    idx = torch.randint(0, 4, (n, h // 2, w // 2, c), generator=g).to(torch.uint8)
    return d_pooled.to(dev), idx.to(dev)


CASES = [   # (dtype, N, H, W, C, pool, mode)
    ("fp32", 1, 6, 10, 8, False, ""),              # vector form
    ("fp32", 2, 5, 7, 6, False, ""),               # scalar form, odd W
    ("fp32", 1, 6, 10, 8, False, "shift"),         # 4 bytes off a 16-byte boundary: scalar form
    ("fp32", 2, 9, 7, 4, False, ""),               # odd H and W, vector form
    ("fp32", 4, 64, 64, 32, False, ""),            # 512 workgroups
    ("fp32", 1, 6, 10, 260, False, ""),            # 65 quads per pixel: blocks rounded up to a multiple of 65
    ("fp32", 1, 6, 10, 513, False, ""),            # more channel groups than threads of a workgroup
    ("fp32", 2, 8, 16, 16, True, ""),              # routing
    ("fp32", 2, 8, 12, 4, True, ""), ("fp32", 1, 4, 6, 1024, True, ""),
    ("fp32", 2, 64, 8, 16, True, ""),              # 128 image rows
    ("fp32", 2, 8, 16, 24, True, "fallback"),      # 6 quads per pixel: not a power of two, maxpool_bwd first
    ("fp32", 2, 6, 16, 16, True, "shift_coef"),    # scale not 16-byte aligned: the routing form refuses, fallback
    ("bf16", 2, 8, 12, 8, False, ""), ("bf16", 2, 9, 7, 128, False, ""), ("bf16", 1, 4, 6, 2048, False, ""),
    ("bf16", 2, 8, 12, 8, True, ""), ("bf16", 2, 8, 12, 128, True, ""), ("bf16", 3, 32, 48, 32, True, ""),
]


def _id(c):
    return "%s-%dx%dx%dx%d%s%s" % (c[:5] + ("-pool" if c[5] else "", "-" + c[6] if c[6] else ""))


def check_case(dev, case, y, co, d_act, pool_dev, exact):
    """Runs one geometry out of place with sums, in place with sums, and without sums, and judges all three."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    dt, n, h, w, c, pool, mode = case
    bf = dt == "bf16"
    lib = L()
    y, d_act = y.to(dev), d_act.to(dev)
    cod = {k: v.to(dev) for k, v in co.items()}
    grad64 = d_act.double()
    if pool:
        grad64 = grad64 + ref_route(pool_dev[0], pool_dev[1], y.shape)
    ref = Ref(grad64, y, cod)
    assert ref.margin > GATE_MARGIN, ref.margin
    put = (lambda t: shifted(t)) if mode == "shift" else (lambda t: t.clone())
    if mode == "shift_coef":
        cod["scale"] = shifted(cod["scale"])
    launch_pool = pool_dev
    if mode in ("fallback", "shift_coef"):
        # the routing form does not take this call: EINVAL before anything is launched, and the caller routes the pooled
        # gradient with maxpool_bwd first (ops.bn_frozen_backward does exactly this; checked against it below)
        assert mode == "shift_coef" or not bn_bwd_pool_ok(n, h, w, c)
        probe = torch.zeros_like(d_act)
        rc = lib.unetpp_bn_frozen_bwd(ptr(d_act), ptr(y), ptr(cod["scale"]), ptr(cod["shift"]), None, None, ptr(pool_dev[0]),
                                      ptr(pool_dev[1]), n, h, w, c, ptr(probe), None, stream())
        assert rc == -1 and not bool(probe.any())
        routed = d_act.clone()
        ops.maxpool_bwd(pool_dev[0], pool_dev[1], routed)
        d_act, launch_pool = routed, None
    dgamma, dbeta, dy, form = run_frozen(put(d_act), put(y), cod, launch_pool)
    want_form = {"fp32": "pool" if launch_pool is not None else ("scalar" if c % 4 or mode == "shift" else "vec"),
                 "bf16": "bf16"}[dt]
    assert form == want_form, (form, want_form)
    adds = plan(n, h, w, c, form)[0]
    if exact:
        for s in (ref.abs_beta, ref.abs_gamma):   # in units of 1/2: every partial sum is an exact fp32 number
            assert float(s.max()) * 2 < GRID, float(s.max())
        assert torch.equal(dbeta.double(), ref.dbeta) and torch.equal(dgamma.double(), ref.dgamma), case
    worst = {"dbeta": bound_ratio(dbeta, ref.dbeta, gamma(adds + 2) * ref.abs_beta),
             "dgamma": bound_ratio(dgamma, ref.dgamma, gamma(adds + 5) * ref.abs_gamma)}
    if bf:
        close_bf16(dy, ref.dy, (case, "dy"))
    else:
        worst["dy"] = bound_ratio(dy, ref.dy, gamma(2) * ref.dy.abs())
    report_ratio("bn_frozen %s%s" % (_id(case), " exact" if exact else ""), "worst", max(worst.values()),
                 dict(worst, adds=adds, form=form))
    assert max(worst.values()) <= 1.0, (case, worst)
    # in place (dy aliases d_act), as the engine calls it: bit for bit
    dg2, db2, dy2, _ = run_frozen(put(d_act), put(y), cod, launch_pool, in_place=True)
    assert torch.equal(dy2, dy) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta), case
    # partial == NULL: no sums, the same dy
    _, _, dy3, _ = run_frozen(put(d_act), put(y), cod, launch_pool, sums=False)
    assert torch.equal(dy3, dy), case
    return dgamma, dbeta, dy


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_bn_frozen_backward_vs_float64(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import ops
    dt, n, h, w, c, pool, mode = case
    bf = dt == "bf16"
    g = torch.Generator().manual_seed(900 + CASES.index(case))
    y, co = operands(g, n, h, w, c, bf)
    d_act = torch.randn(n, h, w, c, generator=g)
    d_act = d_act.to(BF) if bf else d_act
    pool_dev = make_pool(g, n, h, w, c, bf, dev) if pool else None
    dgamma, dbeta, dy = check_case(dev, case, y, co, d_act, pool_dev, exact=False)
    if mode == "shift":
        return
    # the package's own call (ops.bn_frozen_backward: routing or its maxpool_bwd fallback, finalize) gives the same bits
    cod = {k: v.to(dev) for k, v in co.items()}
    if mode == "shift_coef":
        cod["scale"] = shifted(cod["scale"])
    buf = d_act.to(dev).clone()
    dg, db = ops.bn_frozen_backward(buf, y.to(dev), cod["scale"], cod["shift"], cod["mean"], cod["invstd"], buf, pool=pool_dev)
    assert torch.equal(buf, dy) and torch.equal(dg, dgamma) and torch.equal(db, dbeta), case
    buf = d_act.to(dev).clone()
    none = ops.bn_frozen_backward(buf, y.to(dev), cod["scale"], cod["shift"], None, None, buf, pool=pool_dev, want_sums=False)
    assert none == (None, None) and torch.equal(buf, dy), case


EXACT_CASES = [   # each puts one capped form above FROZEN_CAP workgroups (image rows for the routing form) with a remainder
    ("fp32", 1, 131, 128, 128, False, ""),         # 536576 quads on 2048 * 256 threads
    ("fp32", 1, 300, 300, 6, False, ""),           # 540000 scalars on 2052 * 256 threads
    ("fp32", 1, 4100, 16, 16, True, ""),           # 4100 image rows on 2048 workgroups
    ("bf16", 1, 131, 128, 256, False, ""),         # 536576 octets on 2048 * 256 threads
    ("bf16", 1, 132, 128, 256, True, ""),
    ("fp32", 2, 8, 16, 16, True, ""), ("fp32", 2, 5, 7, 6, False, ""), ("bf16", 2, 8, 12, 8, True, ""),
]


@pytest.mark.parametrize("case", EXACT_CASES, ids=[_id(c) for c in EXACT_CASES])
def test_bn_frozen_backward_exact_above_the_caps(dev, case):
    dt, n, h, w, c, pool, mode = case
    bf = dt == "bf16"
    g = torch.Generator().manual_seed(950 + EXACT_CASES.index(case))
    y, co, d_act = exact_operands(g, n, h, w, c, bf)
    pool_dev = make_pool(g, n, h, w, c, bf, dev, exact=True) if pool else None
    check_case(dev, case, y, co, d_act, pool_dev, exact=True)


@pytest.mark.parametrize("c", [1, 6, 64, 130])
def test_bn_eval_coeffs_stats_vs_float64(dev, c):
    """scale / shift are bn_eval_coeffs' bits; mean is the running mean itself; invstd = 1/sqrt(var + eps) within the
    bound tests/test_gpu_streaming.py uses for the same fp32 formula."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    g = torch.Generator().manual_seed(990 + c)
    gam, bet = (1 + 0.1 * torch.randn(c, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
    rm, rv = (0.5 * torch.randn(c, generator=g)).to(dev), (0.5 + 1.5 * torch.rand(c, generator=g)).to(dev)
    eps = 1e-5
    scale0, shift0 = ops.bn_eval_coeffs(gam, bet, rm, rv, eps)
    mean, invstd, scale, shift = ops.bn_eval_coeffs_stats(gam, bet, rm, rv, eps)
    ran("bn_eval_coeffs/stats")
    assert torch.equal(scale, scale0) and torch.equal(shift, shift0) and torch.equal(mean, rm)
    assert mean.data_ptr() != rm.data_ptr()   # a snapshot, not a view
    want = 1.0 / torch.sqrt((rv.double() + torch.tensor(eps, dtype=torch.float32).double()))
    rel_is = (0.5 + 2 * EVAL_DIV_SQRT_ULPS) * U32 * 1.01
    assert bound_ratio(invstd, want, want.abs() * rel_is) <= 1.0


def test_every_frozen_kernel_ran(dev):
    """Runs last in this module: every label of COVERAGE was seen, no other, and every capped form ran above its cap."""
    assert SEEN == set(COVERAGE), (sorted(set(COVERAGE) - SEEN), sorted(SEEN - set(COVERAGE)))
    assert ABOVE_CAP == set(FAMILIES), sorted(set(FAMILIES) - ABOVE_CAP)
