"""The streaming kernels between the GEMMs (BatchNorm finalize / apply / backward, the pool passes, bilinear x2, the
layout converters; pointwise.hip and their bf16 twins in pointwise_bf16.hip; the heads are heads.hip's) against float64.

Every launcher names the form it chose (unetpp_last_kernel_name); each case restates the launcher's own conditions
(C % 4, 16-byte alignment, even / odd H and W, (W/2)*(C/4) >= 64, bn_bwd_pool_ok, octets_ok) and asserts the label.
unetpp_sum_partials has one form and carries no label (ops.head_bwd calls it after the head's launch, and the caller reads
the head's label after both): it is compared with float64 here but is not part of COVERAGE.

(a) Dispatch matrix, float64 references from the same fp32 / bf16 operands, u = 2^-24:
        affine_relu*, pool values, argmax bytes, maxpool_bwd*      exact: one fma rounded once, first maximum in scan
                                                                   order (ReLU-zero ties included), one add per element;
                                                                   bf16: then one round-to-nearest-even
        bn_finalize, bn_bwd_finalize, sum_partials                 rows summed in float64, the same formula; per output
                                                                   ONE fp32 cast (u, relative) plus the float64 terms
                                                                   ((rows + 8) 2^-53 of the absolute sums, carried through
                                                                   s2/count - m*m as computed: |mean|/std up to 30)
        bn_bwd_reduce* + bn_bwd_finalize                           |dbeta - ref| <= gamma_(n+2) sum |gg|,
                                                                   |dgamma - ref| <= gamma_(n+5) sum |gg xhat|, n = fp32
                                                                   additions of a partial row (iterations per thread +
                                                                   threads summed per channel, from the launcher formulas);
                                                                   no gate argument within 8 u of zero (asserted)
        bn_bwd_apply*                                              element-wise, from the kernel's own dgamma / dbeta:
                                                                   gamma_8 |gamma invstd| (|gg| + |dbeta|/m + |xhat dgamma|/m);
                                                                   in place == out of place bit for bit; bf16: close_bf16
        bilinear2x_fwd                                             bilinear_src restated in numpy float32 and checked
                                                                   against rational positions (|s32 - s| <= 2 u s,
                                                                   0 <= l1 <= 1), in both forms the compiler may give
                                                                   l1 = s - i0 (rounded product; contracted into an fma,
                                                                   which gfx950 builds are: l1 >= -2 u s there), then
                                                                   gamma_6 sum |w v| against the nearer form; one
                                                                   comparison with F.interpolate at the 1e-4 bar
        bilinear2x_bwd                                             full adjoint (autograd of the float64 statement):
                                                                   gamma_32 sum |w dy| (+ u |old|), nearer form; no
                                                                   contributor further than 2 from 2 * source (asserted)
        bn_eval_coeffs                                             fp32 formula, EVAL_DIV_SQRT_ULPS (an estimate) for the
                                                                   square root and the division
        layout converters                                          exact
(b) Production geometries in exact arithmetic (level 0 and deepest layers of the three benchmarked configurations, a
    tall case with more than 16384 rows, a narrow case for the generic pool forms), batches chosen so that each launch
    exceeds its grid cap unevenly: small-integer y, d_act, d_pooled (gradients mostly zero), integer mean,
    power-of-two invstd / scale / gamma, shift = integer + 1/2.  Every partial sum is exact in fp32 in any order
    (sum |terms| < 2^24 grid units per channel, asserted), so dbeta and dgamma must EQUAL the float64 result; pool
    winners and routed gradients are exact; dy keeps the bound of (a), bf16 dy close_bf16.
(c) Every COVERAGE label ran, and every family of FAMILIES ran above its cap with a remainder.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import U32, bound_ratio, close_bf16, gamma, rel_err, report_ratio
from tests.stream_rules import (GRID_CAP, K_THREADS, REDUCE_CAP, ROW_CAP, al16, bn_bwd_blocks, bn_bwd_blocks_bf16,  # noqa: F401
                                bn_bwd_blocks_for, bn_bwd_pool_ok, expect_affine, expect_maxpool_bwd, fin_threads, octets_ok,
                                ref_route, rows_form_ok, shifted, windows)

pytestmark = pytest.mark.gpu

TOL = 1e-4
BF = torch.bfloat16
U64 = 2.0 ** -53
CAST = U32 * (1 + 2.0 ** -20)     # one float64 -> fp32 cast of a value that differs from the reference by float64 terms
GATE_MARGIN = 8 * U32             # no gate argument closer to zero than this, relative to |y scale| + |shift|
EVAL_DIV_SQRT_ULPS = 2.0          # estimate (not derived): sqrtf and the fp32 division of bn_eval_coeffs, in u each
GRID = 2.0 ** 24

COVERAGE = [
    "bn_finalize/256", "bn_finalize/512", "bn_finalize/1024", "bn_eval_coeffs",
    "bn_bwd_finalize/256", "bn_bwd_finalize/512", "bn_bwd_finalize/1024",
    "affine_relu<4>", "affine_relu<1>", "affine_relu_pool<4>", "affine_relu_pool<1>", "affine_relu_pool_rows",
    "maxpool_bwd<4>", "maxpool_bwd<1>", "maxpool_bwd_rows",
    "bn_bwd_reduce<4>", "bn_bwd_reduce<1>", "bn_bwd_apply<4>", "bn_bwd_apply<1>",
    "bn_bwd_reduce_pool", "bn_bwd_apply_pool",
    "bilinear2x_fwd", "bilinear2x_bwd", "nchw_to_nhwc", "nhwc_to_nchw",
    "affine_relu_bf16", "affine_relu_pool_bf16", "maxpool_bwd_bf16",
    "bn_bwd_reduce_bf16", "bn_bwd_reduce_bf16/pool", "bn_bwd_apply_bf16", "bn_bwd_apply_bf16/pool",
    "bilinear2x_fwd_bf16", "bilinear2x_bwd_bf16",
]
SEEN = set()
FAMILIES = (   # kernels with a grid cap; each must run above it with a remainder
    "affine_relu<4>", "affine_relu_pool<4>", "affine_relu_pool_rows", "maxpool_bwd<4>", "maxpool_bwd_rows",
    "bn_bwd_reduce<4>", "bn_bwd_apply<4>", "bn_bwd_reduce_pool", "bn_bwd_apply_pool", "bilinear2x_fwd", "nchw_to_nhwc",
    "nhwc_to_nchw", "affine_relu_bf16", "affine_relu_pool_bf16", "maxpool_bwd_bf16", "bn_bwd_reduce_bf16",
    "bn_bwd_apply_bf16",
)
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
    """The launcher's label is the one the restated conditions give; record it."""
    name = L().unetpp_last_kernel_name().decode()
    assert name == expect, (name, expect)
    SEEN.add(name)
    return name


def above(family, count, span, into=None):
    """`count` items / rows on a grid that covers `span` per pass: above the cap with a remainder?"""
    if count > span and count % span:
        (ABOVE_CAP if into is None else into).add(family)
        return True
    return False


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    assert rc == 0, (what, rc)


def ratio(got, want, bound):
    """bound_ratio on the tensors' own device (the production cases hold > 1e8 elements)."""
    got, want, bound = got.double(), want.double(), bound.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs() / bound.clamp_min(1e-300)).max())


# --------------------------------------------------------------------------------------------- pool passes
def ref_affine_pool(y, scale, shift, relu):
    """-> (act, pooled, argmax byte) in the storage type of y: one fma rounded once (float64 holds the product exactly),
    ReLU, for bf16 one round-to-nearest-even; the winner is the first maximum of the STORED values in scan order."""
    a = y.double()
    if scale is not None:
        a = a * scale.double() + shift.double()
    a = a.float()
    if relu:
        a = a.clamp_min(0)
    a = a.to(y.dtype)
    cand = windows(a)
    best = cand[0].clone()
    bi = torch.zeros(best.shape, dtype=torch.uint8, device=y.device)
    for q in (1, 2, 3):
        m = cand[q] > best
        best = torch.where(m, cand[q], best)
        bi = torch.where(m, torch.full_like(bi, q), bi)
    return a, best, bi


def run_affine(y, scale, shift, relu, want_act=True, want_pool=True, want_idx=True, mode=""):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, h, w, c = y.shape
    dev = y.device
    act = torch.full_like(y, float("nan")) if want_act else None
    pooled = torch.full((n, h // 2, w // 2, c), float("nan"), dtype=y.dtype, device=dev) if want_pool else None
    idx = torch.full((n, h // 2, w // 2, c), 9, dtype=torch.uint8, device=dev) if want_pool and want_idx else None
    if mode == "shift_idx":
        idx = shifted(idx, 1)
    ops.affine_relu_pool(y, scale, shift, relu, act, pooled, idx)
    name = ran(expect_affine(y, scale, shift, act, pooled, idx))
    return act, pooled, idx, name


def run_maxpool_bwd(d_pooled, idx, d_act, gate=None):
    from unet_nested4tiny_objects_keypoints_amd import ops
    ops.maxpool_bwd(d_pooled, idx, d_act, gate=gate)
    return ran(expect_maxpool_bwd(d_pooled, idx, d_act))


POOL_CASES = [   # (N, H, W, C, mode)
    (2, 6, 10, 3, ""), (2, 6, 10, 4, ""), (2, 6, 10, 8, ""), (2, 6, 10, 20, ""),
    (2, 6, 10, 32, ""),            # (W/2)*(C/4) = 40: generic vector form
    (2, 6, 16, 32, ""),            # = 64: the rows form
    (1, 4, 10, 260, ""),           # rows form with 65 quads per pixel
    (1, 4, 6, 513, ""),            # scalar
    (2, 6, 16, 32, "shift_y"),     # input 4 bytes off a 16-byte boundary: scalar form
    (2, 6, 16, 32, "shift_idx"),   # winners not on a dword boundary: no rows form
    (2, 6, 16, 32, "shift_coef"),  # scale not 16-byte aligned: no rows form
    (2, 6, 16, 32, "noact"), (2, 6, 16, 32, "noidx"), (2, 6, 10, 8, "noact"), (2, 6, 10, 8, "noidx"),
    (2, 6, 10, 3, "noidx"), (1, 4, 128, 64, "noaffine"), (2, 6, 10, 20, "noaffine"),
    (2, 5, 8, 8, ""), (2, 6, 7, 8, ""), (1, 9, 7, 3, ""), (2, 5, 7, 32, "noact"), (1, 7, 33, 32, ""),
    (2, 5, 7, 8, "shift_y"), (1, 7, 9, 12, "noidx"),
]


@pytest.mark.parametrize("case", POOL_CASES, ids=["%dx%dx%dx%d%s" % (c[:4] + ("-" + c[4] if c[4] else "",)) for c in POOL_CASES])
def test_affine_relu_pool_and_routing_exact(dev, case):
    n, h, w, c, mode = case
    g = torch.Generator().manual_seed(100 + POOL_CASES.index(case))
    y = torch.randn(n, h, w, c, generator=g)
    y[0, :2, :2, :] = -3.0            # a window of ReLU zeros: four-way tie, winner 0
    affine = mode != "noaffine"
    scale = (1 + 0.2 * torch.randn(c, generator=g)) if affine else None
    shift = (0.3 * torch.randn(c, generator=g)) if affine else None
    want_act, want_pool, want_idx = ref_affine_pool(y, scale, shift, affine)
    yd = shifted(y.to(dev)) if mode == "shift_y" else y.to(dev)
    sd = None if scale is None else (shifted(scale.to(dev)) if mode == "shift_coef" else scale.to(dev))
    hd = None if shift is None else shift.to(dev)
    act, pooled, idx, name = run_affine(yd, sd, hd, affine, want_act=mode != "noact", want_idx=mode != "noidx", mode=mode)
    if act is not None:
        assert torch.equal(act.cpu(), want_act), (case, name)
    assert torch.equal(pooled.cpu(), want_pool), (case, name)
    if idx is not None:
        assert torch.equal(idx.cpu(), want_idx), (case, name)
    # the activation alone
    act1, _, _, name1 = run_affine(yd, sd, hd, affine, want_pool=False)
    assert torch.equal(act1.cpu(), want_act), (case, name1)
    # the routing, on the reference's winners
    d_pool = torch.randn(want_pool.shape, generator=g)
    base = torch.randn(y.shape, generator=g)
    want = (base.double() + ref_route(d_pool, want_idx, y.shape)).float()
    acc = shifted(base.to(dev)) if mode == "shift_y" else base.to(dev)
    widx = want_idx.to(dev)
    bname = run_maxpool_bwd(d_pool.to(dev), shifted(widx, 1) if mode == "shift_idx" else widx, acc)
    assert torch.equal(acc.cpu(), want), (case, bname)


BF16_POOL_CASES = [(2, 6, 10, 8), (1, 4, 6, 128), (1, 4, 6, 1024), (1, 2, 4, 2048), (2, 8, 12, 32)]


@pytest.mark.parametrize("case", BF16_POOL_CASES, ids=["%dx%dx%dx%d" % c for c in BF16_POOL_CASES])
def test_affine_relu_pool_and_routing_bf16_exact(dev, case):
    n, h, w, c = case
    g = torch.Generator().manual_seed(200 + BF16_POOL_CASES.index(case))
    y = torch.randn(n, h, w, c, generator=g).to(BF)
    y[0, :2, :2, :] = -3.0
    scale, shift = 1 + 0.2 * torch.randn(c, generator=g), 0.3 * torch.randn(c, generator=g)
    want_act, want_pool, want_idx = ref_affine_pool(y, scale, shift, True)
    act, pooled, idx, name = run_affine(y.to(dev), scale.to(dev), shift.to(dev), True)
    assert torch.equal(act.cpu(), want_act) and torch.equal(pooled.cpu(), want_pool), (case, name)
    assert torch.equal(idx.cpu(), want_idx), (case, name)
    act1, _, _, name1 = run_affine(y.to(dev), scale.to(dev), shift.to(dev), True, want_pool=False)
    assert torch.equal(act1.cpu(), want_act), (case, name1)
    d_pool = torch.randn(want_pool.shape, generator=g).to(BF)
    base = torch.randn(y.shape, generator=g).to(BF)
    for use_gate in (False, True):
        want = (base.double() + ref_route(d_pool, want_idx, y.shape)).float()    # the kernel's fp32 add, exactly
        if use_gate:
            want = torch.where(want_act.float() > 0, want, torch.zeros_like(want))
        acc = base.to(dev)
        bname = run_maxpool_bwd(d_pool.to(dev), want_idx.to(dev), acc, gate=act if use_gate else None)
        assert torch.equal(acc.cpu(), want.to(BF)), (case, bname, use_gate)


# --------------------------------------------------------------------------------------------- sums over partial rows
FIN_ROWS = (1, 7, 255, 1027, 4101, 8192)   # the three workgroup sizes; the eight-row loop with and without a tail
RATIOS = (0.0, 0.5, 3.0, 30.0, -30.0)      # mean / std of the channels


def _stat_rows(g, rows, per_row=64):
    """fp32 (sum, sum of squares) rows as a convolution epilogue leaves them, from float64 samples."""
    c = len(RATIOS)
    sd = 0.5 + torch.rand(c, generator=g, dtype=torch.float64)
    x = torch.tensor(RATIOS, dtype=torch.float64) * sd + sd * torch.randn(rows, per_row, c, generator=g, dtype=torch.float64)
    return torch.stack([x.sum(1), (x * x).sum(1)], 2).float().contiguous(), rows * per_row


def ref_finalize(part, count, gam, bet, eps, mom, rm, rv):
    """bn_finalize_kernel in float64 from the fp32 rows -> {name: (value, bound)}.  The kernel adds the same rows in
    float64 in another order: e64 = (rows + 8) 2^-53 of the absolute sums covers that, the divisions, the square root and
    the products; it is carried through var = s2/count - m*m AS COMPUTED (dvar), to first order (x 1.01) through
    1/sqrt(var + eps).  On top, every output takes ONE cast to fp32: CAST, relative."""
    p = part.double()
    rows = part.shape[0]
    eps, mom = float(np.float32(eps)), float(np.float32(mom))
    s1, s2 = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    a1 = p[:, :, 0].abs().sum(0)
    m = s1 / count
    var = (s2 / count - m * m).clamp_min(0)
    is_ = 1.0 / torch.sqrt(var + eps)
    sc = gam.double() * is_
    sh = bet.double() - m * sc
    e64 = (rows + 8) * U64
    dm = e64 * a1 / count
    dvar = e64 * (s2 / count + m * m) + 2 * m.abs() * dm + dm * dm
    rel_is = 1.01 * 0.5 * dvar / (var + eps) + 4 * U64
    out = {
        "mean": (m, CAST * m.abs() + dm),
        "invstd": (is_, is_ * (CAST + rel_is)),
        "scale": (sc, sc.abs() * (CAST + rel_is + U64)),
        "shift": (sh, CAST * sh.abs() + sc.abs() * dm + (m * sc).abs() * (rel_is + 2 * U64) + U64 * (bet.double().abs() + (m * sc).abs())),
    }
    if rm is not None:
        f = count / (count - 1.0) if count > 1 else 1.0
        nrm = (1.0 - mom) * rm.double() + mom * m
        nrv = (1.0 - mom) * rv.double() + mom * var * f
        out["running_mean"] = (nrm, CAST * nrm.abs() + mom * dm + 4 * U64 * (rm.double().abs() + m.abs()))
        out["running_var"] = (nrv, CAST * nrv.abs() + mom * f * dvar + 4 * U64 * (rv.double().abs() + var * f))
    return out


def _check_finalize(dev, part, count, gam, bet, rm, rv, label):
    from unet_nested4tiny_objects_keypoints_amd import ops
    rows, c = part.shape[0], part.shape[1]
    eps, mom = 1e-5, 0.1
    want = ref_finalize(part, count, gam, bet, eps, mom, rm, rv)
    rmd, rvd = (None, None) if rm is None else (rm.to(dev), rv.to(dev))
    mean, invstd, scale, shift = ops.bn_finalize(part.to(dev).view(-1), rows, c, count, gam.to(dev), bet.to(dev), eps, mom, rmd, rvd)
    ran("bn_finalize/%d" % fin_threads(rows))
    got = {"mean": mean, "invstd": invstd, "scale": scale, "shift": shift}
    if rm is not None:
        got.update(running_mean=rmd, running_var=rvd)
    worst = {k: bound_ratio(got[k], want[k][0], want[k][1]) for k in want}
    report_ratio("bn_finalize %s" % label, "worst", max(worst.values()), worst)
    assert max(worst.values()) <= 1.0, (label, worst)
    return (None, None) if rm is None else (rmd.cpu(), rvd.cpu())


@pytest.mark.parametrize("rows", FIN_ROWS)
def test_bn_finalize_vs_float64(dev, rows):
    g = torch.Generator().manual_seed(300 + rows)
    c = len(RATIOS)
    gam, bet = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    part, count = _stat_rows(g, rows)
    _check_finalize(dev, part, count, gam, bet, None, None, "rows %d, no running statistics" % rows)
    rm, rv = 0.1 * torch.randn(c, generator=g), 1 + 0.1 * torch.rand(c, generator=g)
    for step in range(3):   # three momentum updates in a row, each from the kernel's own previous buffers
        part, count = _stat_rows(g, rows)
        rm, rv = _check_finalize(dev, part, count, gam, bet, rm, rv, "rows %d, update %d" % (rows, step))


def test_bn_finalize_single_sample(dev):
    """count = 1: the unbiased-variance branch keeps var (no division by count - 1); var itself is rounding noise of
    s2 - m*m and may be negative before the clamp."""
    g = torch.Generator().manual_seed(310)
    c = len(RATIOS)
    x = torch.randn(c, generator=g) * 3
    part = torch.stack([x, x * x], 1).view(1, c, 2).contiguous()
    gam, bet = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    rm, rv = 0.1 * torch.randn(c, generator=g), 1 + 0.1 * torch.rand(c, generator=g)
    _check_finalize(dev, part, 1, gam, bet, rm, rv, "count 1")


@pytest.mark.parametrize("rows", FIN_ROWS)
def test_partial_row_sums_vs_float64(dev, rows):
    """bn_bwd_finalize and sum_partials: the rows summed in float64 and cast once: CAST |sum| + (rows + 8) 2^-53 sum |row|."""
    lib = L()
    g = torch.Generator().manual_seed(320 + rows)
    e64 = (rows + 8) * U64
    worst = {}
    c = 5
    part = (torch.randn(rows, c, 2, generator=g) + torch.tensor([0.5, -0.25])).contiguous()
    pd = part.to(dev)
    dgamma, dbeta = (torch.full((c,), float("nan"), device=dev) for _ in range(2))
    ok(lib.unetpp_bn_bwd_finalize(ptr(pd), rows, c, ptr(dgamma), ptr(dbeta), stream()), "bn_bwd_finalize")
    ran("bn_bwd_finalize/%d" % fin_threads(rows))
    s, a = part.double().sum(0), part.double().abs().sum(0)
    worst["dbeta"] = bound_ratio(dbeta, s[:, 0], CAST * s[:, 0].abs() + e64 * a[:, 0])
    worst["dgamma"] = bound_ratio(dgamma, s[:, 1], CAST * s[:, 1].abs() + e64 * a[:, 1])
    for ln in (1, 16, 37, 100):
        part = (torch.randn(rows, ln, generator=g) + 0.5).contiguous()
        out = torch.full((ln,), float("nan"), device=dev)
        pd = part.to(dev)
        ok(lib.unetpp_sum_partials(ptr(pd), rows, ln, ptr(out), stream()), "sum_partials")
        s, a = part.double().sum(0), part.double().abs().sum(0)
        worst["sum_partials len %d" % ln] = bound_ratio(out, s, CAST * s.abs() + e64 * a)
    report_ratio("partial rows %d" % rows, "worst", max(worst.values()), worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("c", [1, 63, 64, 65, 1024])
def test_bn_eval_coeffs_vs_float64(dev, c):
    """is = 1 / sqrtf(rv + eps): the sum rounds once (half of it survives the root), the root and the division take
    EVAL_DIV_SQRT_ULPS u each (correctly rounded they take one); scale = gamma * is: one more; shift = beta - rm * scale:
    one more on the product and one on the difference."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    g = torch.Generator().manual_seed(330 + c)
    gam, bet = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    rm, rv = torch.randn(c, generator=g), 0.05 + torch.rand(c, generator=g) * 4
    eps = 1e-5
    scale, shift = ops.bn_eval_coeffs(gam.to(dev), bet.to(dev), rm.to(dev), rv.to(dev), eps)
    ran("bn_eval_coeffs")
    is_ = 1.0 / torch.sqrt(rv.double() + float(np.float32(eps)))
    sc = gam.double() * is_
    sh = bet.double() - rm.double() * sc
    rel_is = (0.5 + 2 * EVAL_DIV_SQRT_ULPS) * U32 * 1.01
    rel_sc = rel_is + U32 * 1.01
    worst = {"scale": bound_ratio(scale, sc, sc.abs() * rel_sc),
             "shift": bound_ratio(shift, sh, (rm.double() * sc).abs() * (rel_sc + U32) + U32 * 1.01 * (bet.double().abs() + (rm.double() * sc).abs()))}
    report_ratio("bn_eval_coeffs C=%d" % c, "worst", max(worst.values()), worst)
    assert max(worst.values()) <= 1.0, worst


# --------------------------------------------------------------------------------------------- BatchNorm backward
def reduce_adds(n, h, w, c, form):
    """fp32 additions a partial row goes through: iterations per thread plus the threads summed per channel."""
    pixels = n * h * w
    if form == "bf16":
        cg = c // 8
        iters = -(-pixels * cg // (bn_bwd_blocks_bf16(pixels, c) * K_THREADS))
        return iters + K_THREADS // cg
    if form == "pool":
        cg = c // 4
        grid = min(n * h, bn_bwd_blocks(pixels, c))
        return -(-n * h // grid) * -(-w * cg // K_THREADS) + K_THREADS // cg
    cg = c // 4 if form == "vec" else c
    iters = -(-pixels * cg // (bn_bwd_blocks_for(pixels, c, form == "vec") * K_THREADS))
    return iters + -(-K_THREADS // cg)


def run_bn_bwd(d_act, y, co, pool=None, in_place=False):
    """reduce, finalize, apply through the C ABI, the label asserted after each -> (dgamma, dbeta, dy, form)."""
    lib = L()
    n, h, w, c = y.shape
    pixels = n * h * w
    dev = y.device
    bf = y.dtype == BF
    if bf:
        assert octets_ok(c)
        blocks = int(lib.unetpp_bn_bwd_blocks_bf16(pixels, c))
        assert blocks == bn_bwd_blocks_bf16(pixels, c)
    else:
        blocks = int(lib.unetpp_bn_bwd_blocks(pixels, c))
        assert blocks == bn_bwd_blocks(pixels, c)
        assert bool(lib.unetpp_bn_bwd_pool_ok(n, h, w, c)) == bn_bwd_pool_ok(n, h, w, c)
    partial = torch.full((blocks * c * 2,), float("nan"), device=dev)
    dgamma, dbeta = (torch.full((c,), float("nan"), device=dev) for _ in range(2))
    dy = d_act if in_place else torch.full_like(d_act, float("nan"))
    dp, pi = pool if pool is not None else (None, None)
    st = stream()
    cf = [ptr(co[k]) for k in ("scale", "shift", "mean", "invstd")]
    if bf:
        form = "bf16"
        ok(lib.unetpp_bn_bwd_reduce_bf16(ptr(d_act), ptr(y), *cf, ptr(dp), ptr(pi), n, h, w, c, ptr(partial), st), "reduce")
        ran("bn_bwd_reduce_bf16/pool" if pool is not None else "bn_bwd_reduce_bf16")
    elif pool is not None:
        form = "pool"
        ok(lib.unetpp_bn_bwd_reduce_pool(ptr(d_act), ptr(y), *cf, ptr(dp), ptr(pi), n, h, w, c, ptr(partial), st), "reduce")
        ran("bn_bwd_reduce_pool")
    else:
        vec = c % 4 == 0 and al16(d_act) and al16(y)
        form = "vec" if vec else "scalar"
        ok(lib.unetpp_bn_bwd_reduce(ptr(d_act), ptr(y), *cf, pixels, c, ptr(partial), st), "reduce")
        ran("bn_bwd_reduce<4>" if vec else "bn_bwd_reduce<1>")
    ok(lib.unetpp_bn_bwd_finalize(ptr(partial), blocks, c, ptr(dgamma), ptr(dbeta), st), "finalize")
    ran("bn_bwd_finalize/%d" % fin_threads(blocks))
    if bf:
        ok(lib.unetpp_bn_bwd_apply_bf16(ptr(d_act), ptr(y), *cf, ptr(co["gamma"]), ptr(dgamma), ptr(dbeta), ptr(dp), ptr(pi),
                                        n, h, w, c, ptr(dy), st), "apply")
        ran("bn_bwd_apply_bf16/pool" if pool is not None else "bn_bwd_apply_bf16")
    elif pool is not None:
        ok(lib.unetpp_bn_bwd_apply_pool(ptr(d_act), ptr(y), *cf, ptr(co["gamma"]), ptr(dgamma), ptr(dbeta), ptr(dp), ptr(pi),
                                        n, h, w, c, ptr(dy), st), "apply")
        ran("bn_bwd_apply_pool")
    else:
        vec = c % 4 == 0 and al16(d_act) and al16(y) and al16(dy)
        ok(lib.unetpp_bn_bwd_apply(ptr(d_act), ptr(y), *cf, ptr(co["gamma"]), ptr(dgamma), ptr(dbeta), pixels, c, ptr(dy), st),
           "apply")
        ran("bn_bwd_apply<4>" if vec else "bn_bwd_apply<1>")
    torch.cuda.synchronize()
    return dgamma, dbeta, dy, form


class BnRef:
    """The float64 statement of BatchNorm + ReLU backward from the same fp32 / bf16 numbers, built once per case."""

    def __init__(self, grad64, y, co):
        c = y.shape[3]
        y64 = y.double()
        sc, sh, mu, is_ = (co[k].double() for k in ("scale", "shift", "mean", "invstd"))
        arg = y64 * sc + sh
        self.margin = float((arg.abs() / ((y64 * sc).abs() + sh.abs())).min())   # the reference alone decides a gate
        self.gg = torch.where(arg > 0, grad64, torch.zeros_like(grad64))
        self.xhat = (y64 - mu) * is_
        self.k = co["gamma"].double() * is_
        self.m = float(y.numel() // c)
        flat = lambda t: t.reshape(-1, c).sum(0)   # noqa: E731
        prod = self.gg * self.xhat
        self.dbeta, self.dgamma = flat(self.gg), flat(prod)
        self.abs_beta, self.abs_gamma = flat(self.gg.abs()), flat(prod.abs())

    def dy(self, dgamma, dbeta):
        """(dy, bound) from the kernel's own dgamma / dbeta: the two passes are judged separately."""
        t2 = dbeta.double() / self.m
        t3 = self.xhat * (dgamma.double() / self.m)
        want = self.k * (self.gg - t2 - t3)
        return want, gamma(8) * self.k.abs() * (self.gg.abs() + t2.abs() + t3.abs())


def _bn_operands(g, n, h, w, c, bf):
    """Random operands whose gate arguments all stay GATE_MARGIN away from zero (moved by 1/4 where they did not)."""
    y = torch.randn(n, h, w, c, generator=g) * 1.5 + 0.2
    y = y.to(BF) if bf else y
    yd = y.double().view(-1, c)
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    gam = 1 + 0.1 * torch.randn(c, generator=g)
    bet = 0.1 * torch.randn(c, generator=g)
    co = {"gamma": gam, "invstd": invstd.float(), "mean": mean.float(), "scale": (gam.double() * invstd).float(),
          "shift": (bet.double() - mean * gam.double() * invstd).float()}
    arg = y.double() * co["scale"].double() + co["shift"].double()
    near = arg.abs() <= 64 * GATE_MARGIN * ((y.double() * co["scale"].double()).abs() + co["shift"].double().abs())
    y = torch.where(near, (y.float() + 0.25).to(y.dtype), y)
    return y, co


BN_CASES = [   # (dtype, N, H, W, C, pool, mode)
    ("fp32", 2, 24, 40, 3, False, ""), ("fp32", 2, 24, 40, 4, False, ""), ("fp32", 2, 24, 40, 8, False, ""),
    ("fp32", 2, 24, 40, 20, False, ""), ("fp32", 2, 24, 40, 32, False, ""), ("fp32", 2, 6, 10, 260, False, ""),
    ("fp32", 1, 6, 10, 513, False, ""),            # more channel groups than threads of a workgroup
    ("fp32", 4, 64, 64, 32, False, ""),            # 32 workgroups, 16 items per thread
    ("fp32", 2, 24, 40, 32, False, "shift"),       # 4 bytes off: scalar forms
    ("fp32", 2, 8, 12, 4, True, ""), ("fp32", 2, 8, 12, 16, True, ""), ("fp32", 2, 8, 12, 128, True, ""),
    ("fp32", 1, 4, 64, 256, True, ""), ("fp32", 1, 4, 6, 1024, True, ""),
    ("fp32", 2, 64, 8, 16, True, ""),              # 128 image rows on 16 partial rows: the row loop iterates
    ("bf16", 2, 8, 12, 8, False, ""), ("bf16", 2, 8, 12, 128, False, ""), ("bf16", 1, 4, 6, 1024, False, ""),
    ("bf16", 1, 4, 6, 2048, False, ""), ("bf16", 2, 8, 12, 8, True, ""), ("bf16", 2, 8, 12, 128, True, ""),
    ("bf16", 1, 4, 6, 1024, True, ""), ("bf16", 1, 4, 6, 2048, True, ""), ("bf16", 3, 32, 48, 32, True, ""),
]


def _bn_id(c):
    return "%s-%dx%dx%dx%d%s%s" % (c[:5] + ("-pool" if c[5] else "", "-" + c[6] if c[6] else ""))


@pytest.mark.parametrize("case", BN_CASES, ids=[_bn_id(c) for c in BN_CASES])
def test_bn_backward_vs_float64(dev, case):
    dt, n, h, w, c, pool, mode = case
    bf = dt == "bf16"
    g = torch.Generator().manual_seed(400 + BN_CASES.index(case))
    y, co = _bn_operands(g, n, h, w, c, bf)
    d_act = torch.randn(n, h, w, c, generator=g)
    d_act = d_act.to(BF) if bf else d_act
    grad64 = d_act.double()
    pool_dev = None
    if pool:
        d_pooled = torch.randn(n, h // 2, w // 2, c, generator=g)
        d_pooled = d_pooled.to(BF) if bf else d_pooled
        idx = torch.randint(0, 4, (n, h // 2, w // 2, c), generator=g).to(torch.uint8)
        grad64 = grad64 + ref_route(d_pooled, idx, y.shape)
        pool_dev = (d_pooled.to(dev), idx.to(dev))
    ref = BnRef(grad64, y, co)
    assert ref.margin > GATE_MARGIN, ref.margin
    cod = {k: v.to(dev) for k, v in co.items()}
    put = (lambda t: shifted(t.to(dev))) if mode == "shift" else (lambda t: t.to(dev))
    dgamma, dbeta, dy, form = run_bn_bwd(put(d_act), put(y), cod, pool_dev)
    assert form == {"fp32": "pool" if pool else ("scalar" if c % 4 or mode == "shift" else "vec"), "bf16": "bf16"}[dt]
    adds = reduce_adds(n, h, w, c, form)
    worst = {"dbeta": bound_ratio(dbeta, ref.dbeta, gamma(adds + 2) * ref.abs_beta),
             "dgamma": bound_ratio(dgamma, ref.dgamma, gamma(adds + 5) * ref.abs_gamma)}
    want_dy, dy_bound = ref.dy(dgamma.cpu(), dbeta.cpu())
    if bf:
        close_bf16(dy, want_dy, (case, "dy"))
    else:
        worst["dy"] = bound_ratio(dy, want_dy, dy_bound)
    report_ratio("bn_bwd %s" % _bn_id(case), "worst", max(worst.values()), dict(worst, adds=adds, form=form))
    assert max(worst.values()) <= 1.0, (case, worst)
    # in place (dy aliases d_act), as the engine calls it: bit for bit
    dg2, db2, dy2, _ = run_bn_bwd(put(d_act), put(y), cod, pool_dev, in_place=True)
    assert torch.equal(dy2, dy) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta), case


# --------------------------------------------------------------------------------------------- bilinear x2
FORMS = ("rounded product", "contracted")


def src_positions(n_in, contracted=False):
    """bilinear_src of both kernel files restated for every destination index of the doubled axis -> (i0, i1, l1, s).
    Two forms of `l1 = s - float(i0)`, both the source's arithmetic under HIP's default -ffp-contract=fast:
      rounded product  numpy float32, same operations in the same order: s = fl(r dst) rounded, the difference exact;
      contracted       what hipcc emits for gfx950 in both files (v_mul_f32 for s and the integer part, v_fma_f32
                       (r, dst, -float(i0)) for l1): r dst is exact in float64 (24 x 12 bits), minus the integer i0 it
                       still is, and one rounding to fp32 is the fma.  l1 can then be about -u s (s rounded up to an
                       integer from a product just below it)."""
    n_out = 2 * n_in
    r = np.float32(n_in - 1) / np.float32(n_out - 1)
    s = r * np.arange(n_out).astype(np.float32)
    assert s.dtype == np.float32
    i0 = np.minimum(s.astype(np.int32), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    if contracted:
        l1 = (np.float64(r) * np.arange(n_out).astype(np.float64) - i0.astype(np.float64)).astype(np.float32)
    else:
        l1 = s - i0.astype(np.float32)
    assert l1.dtype == np.float32
    return i0.astype(np.int64), i1.astype(np.int64), l1, s


def check_positions(n_in):
    """(i) for BOTH forms: the fp32 position i0 + l1 against the exact rational one (|p - s| <= 2 u s: the ratio's
    rounding and one more), the range of l1 ([0, 1]; the contracted form may undershoot zero by 2 u s), and the largest
    |dst - 2 * source| over the contributors the backward kernel's own tests (`1.f - l1`, `l1` non-zero) admit."""
    reach = 0
    n_out = 2 * n_in
    for contracted in (False, True):
        i0, i1, l1, s = src_positions(n_in, contracted)
        for dst in range(n_out):
            exact = Fraction(dst * (n_in - 1), n_out - 1)
            pos = Fraction(int(i0[dst])) + Fraction(float(l1[dst]))
            assert abs(pos - exact) <= Fraction(2.0 * U32) * exact, (n_in, dst, contracted)
        low = -2.0 * U32 * s.astype(np.float64) if contracted else np.zeros(n_out)
        assert bool((l1 >= low).all()) and bool((l1 <= 1).all()), (n_in, contracted)
        dst = np.arange(n_out)
        d0 = np.where(np.float32(1) - l1 != 0, np.abs(dst - 2 * i0), 0)
        d1 = np.where(l1 != 0, np.abs(dst - 2 * i1), 0)
        reach = max(reach, int(d0.max()), int(d1.max()))
    return reach


def interp64(x64, contracted=False, magnitude=False):
    """(ii) the interpolation in float64 with the restated (i0, i1, l1) of one form; x64 NHWC.  magnitude=True: the
    same taps with the absolute weights (x64 >= 0): sum |w v|."""
    _, h, w, _ = x64.shape
    y0, y1, ly, _ = src_positions(h, contracted)
    x0, x1, lx, _ = src_positions(w, contracted)
    ly = torch.from_numpy(ly.astype(np.float64)).view(1, -1, 1, 1)
    lx = torch.from_numpy(lx.astype(np.float64)).view(1, 1, -1, 1)
    y0, y1, x0, x1 = (torch.from_numpy(a) for a in (y0, y1, x0, x1))
    wy0, wy1, wx0, wx1 = 1 - ly, ly, 1 - lx, lx
    if magnitude:
        wy0, wy1, wx0, wx1 = wy0.abs(), wy1.abs(), wx0.abs(), wx1.abs()

    def mix(r):
        return wx0 * r[:, :, x0] + wx1 * r[:, :, x1]
    return wy0 * mix(x64[:, y0]) + wy1 * mix(x64[:, y1])


BILINEAR_CASES = [(2, 1, 1, 3), (1, 2, 3, 4), (2, 5, 7, 5), (2, 64, 48, 6), (2, 192, 320, 20), (1, 256, 256, 4)]


@pytest.mark.parametrize("case", BILINEAR_CASES, ids=["%dx%dx%dx%d" % c for c in BILINEAR_CASES])
def test_bilinear2x_vs_float64(dev, case):
    """Each kernel is judged against the nearer of the two statements of l1 (src_positions) under the bounds
    gamma_6 sum |w v| and gamma_32 sum |w dy| (+ u |old|): a build is one form or the other throughout, and the
    ratios against both are reported.  (Against the rounded-product form the gfx950 build misses them by 5-5000x from
    5x7 up, by the u s between the two weights; it is the contracted form.)"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, h, w, c = case
    accumulate = bool(BILINEAR_CASES.index(case) & 1)
    reach = max(check_positions(h), check_positions(w))
    assert reach <= 2, reach      # the kernel gathers from +-3: one pixel of slack
    g = torch.Generator().manual_seed(500 + BILINEAR_CASES.index(case))
    x = torch.randn(n, h, w, c, generator=g)
    dy = torch.randn(n, 2 * h, 2 * w, c, generator=g)
    old = torch.randn(n, h, w, c, generator=g)
    y = torch.full((n, 2 * h, 2 * w, c), float("nan"), device=dev)
    ops.bilinear2x_fwd(x.to(dev), y)
    ran("bilinear2x_fwd")
    above("bilinear2x_fwd", y.numel(), GRID_CAP * K_THREADS)
    torch_ref = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    assert rel_err(y.cpu().permute(0, 3, 1, 2), torch_ref) < TOL, case     # ties the restatement to torch
    dx = old.to(dev) if accumulate else torch.full((n, h, w, c), float("nan"), device=dev)
    ops.bilinear2x_bwd(dy.to(dev), dx, accumulate)
    ran("bilinear2x_bwd")
    ratios = {}
    for contracted in (False, True):
        x64 = x.double().requires_grad_(True)
        out = interp64(x64, contracted)
        ratios["fwd " + FORMS[contracted]] = bound_ratio(y, out.detach(), gamma(6) * interp64(x.double().abs(), contracted, True))
        (want,) = torch.autograd.grad((out * dy.double()).sum(), x64)
        xa = x.double().abs().requires_grad_(True)      # the adjoint of the absolute weights: sum |w dy|
        (mag,) = torch.autograd.grad((interp64(xa, contracted, True) * dy.double().abs()).sum(), xa)
        bound = gamma(32) * mag
        if accumulate:
            want, bound = want + old.double(), bound + U32 * old.double().abs()
        ratios["bwd " + FORMS[contracted]] = bound_ratio(dx, want, bound)
    worst = {k: min(ratios[k + " " + f] for f in FORMS) for k in ("fwd", "bwd")}
    report_ratio("bilinear2x %dx%dx%dx%d" % case, "worst", max(worst.values()),
                 dict(worst, reach=reach, accumulate=accumulate, **ratios))
    assert max(worst.values()) <= 1.0, (case, worst, ratios)


@pytest.mark.parametrize("case", [(1, 5, 7, 8), (2, 64, 48, 16)], ids=["1x5x7x8", "2x64x48x16"])
def test_bilinear2x_bf16_vs_float64(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, h, w, c = case
    g = torch.Generator().manual_seed(520 + h)
    x = torch.randn(n, h, w, c, generator=g).to(BF)
    y = torch.full((n, 2 * h, 2 * w, c), float("nan"), dtype=BF, device=dev)
    ops.bilinear2x_fwd(x.to(dev), y)
    ran("bilinear2x_fwd_bf16")
    x64 = x.double().requires_grad_(True)
    out = interp64(x64)
    close_bf16(y, out.detach(), (case, "forward"))
    dy = torch.randn(n, 2 * h, 2 * w, c, generator=g).to(BF)
    (adj,) = torch.autograd.grad((out * dy.double()).sum(), x64)
    old = torch.randn(n, h, w, c, generator=g).to(BF)
    gate = torch.randn(n, h, w, c, generator=g).to(BF)
    for accumulate, use_gate in ((False, False), (True, False), (True, True)):
        dx = old.to(dev)
        ops.bilinear2x_bwd(dy.to(dev), dx, accumulate, gate.to(dev) if use_gate else None)
        ran("bilinear2x_bwd_bf16")
        want = adj + (old.double() if accumulate else 0)
        if use_gate:
            want = want * (gate.double() > 0)
        close_bf16(dx, want, (case, "backward", accumulate, use_gate))


# --------------------------------------------------------------------------------------------- layout converters
CONVERTER_CASES = [(2, 2, 8, 12), (2, 3, 8, 12), (1, 5, 7, 9), (2, 32, 6, 10), (3, 5, 700, 401)]


@pytest.mark.parametrize("case", CONVERTER_CASES, ids=["%dx%dx%dx%d" % c for c in CONVERTER_CASES])
def test_layout_converters_exact(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, c, h, w = case
    g = torch.Generator().manual_seed(600 + c)
    src = torch.randn(n, c, h, w, generator=g)
    nhwc = ops.nchw_to_nhwc(src.to(dev))
    ran("nchw_to_nhwc")
    assert torch.equal(nhwc.cpu(), src.permute(0, 2, 3, 1).contiguous()), case
    back = ops.nhwc_to_nchw(nhwc)
    ran("nhwc_to_nchw")
    assert torch.equal(back.cpu(), src), case
    if CONVERTER_CASES.index(case) == len(CONVERTER_CASES) - 1:
        assert above("nchw_to_nhwc", src.numel(), GRID_CAP * K_THREADS) and above("nhwc_to_nchw", src.numel(), GRID_CAP * K_THREADS)


# --------------------------------------------------------------------------------------------- (b)
EXACT_CASES = [   # (label, dtype, N, H, W, C, BatchNorm backward too, families that must run above their cap)
    # (17 x 2^19 quads: 17 passes of bn_bwd_reduce<4>'s 2048 workgroups, no remainder at this geometry; the deepest has one)
    ("fp32 base 32 level 0 (256x256x32)", "fp32", 17, 256, 256, 32, True,
     {"affine_relu<4>", "bn_bwd_apply<4>", "bn_bwd_reduce_pool"}),
    ("fp32 base 32 deepest (16x16x512)", "fp32", 257, 16, 16, 512, True,
     {"affine_relu<4>", "bn_bwd_reduce<4>", "bn_bwd_apply<4>", "bn_bwd_reduce_pool"}),
    ("fp32 tall: 17408 pooled rows (17x2048x16x32)", "fp32", 17, 2048, 16, 32, True,
     {"affine_relu_pool_rows", "maxpool_bwd_rows", "bn_bwd_apply_pool"}),
    ("fp32 narrow: generic pool forms (66x2048x126x4)", "fp32", 66, 2048, 126, 4, False,
     {"affine_relu_pool<4>", "maxpool_bwd<4>", "affine_relu<4>"}),
    ("bf16 base 32 level 0 (512x512x32)", "bf16", 17, 512, 512, 32, True,
     {"affine_relu_bf16", "affine_relu_pool_bf16", "maxpool_bwd_bf16", "bn_bwd_apply_bf16"}),
    ("bf16 depth 5 base 64 level 0 (384x384x64)", "bf16", 5, 384, 384, 64, True,
     {"affine_relu_bf16", "maxpool_bwd_bf16", "bn_bwd_reduce_bf16", "bn_bwd_apply_bf16"}),
    ("bf16 depth 5 base 64 deepest (12x12x2048)", "bf16", 114, 12, 12, 2048, True,
     {"affine_relu_bf16", "maxpool_bwd_bf16", "bn_bwd_reduce_bf16", "bn_bwd_apply_bf16"}),
    ("bf16 base 32 deepest (32x32x512)", "bf16", 65, 32, 32, 512, True,
     {"affine_relu_bf16", "maxpool_bwd_bf16", "bn_bwd_reduce_bf16", "bn_bwd_apply_bf16"}),
]


def _mark_caps(name, y, into):
    """Which family the launch `name` on a tensor shaped like y put above its cap, from the restated grids."""
    n, h, w, c = y.shape
    pixels, span = n * h * w, GRID_CAP * K_THREADS
    win = n * (h // 2) * (w // 2)
    table = {
        "affine_relu<4>": (pixels * (c // 4), span), "bn_bwd_apply<4>": (pixels * (c // 4), span),
        "affine_relu_pool<4>": (win * (c // 4), span), "maxpool_bwd<4>": (win * (c // 4), span),
        "affine_relu_pool_rows": (n * (h // 2), ROW_CAP), "maxpool_bwd_rows": (n * (h // 2), ROW_CAP),
        "bn_bwd_apply_pool": (n * h, ROW_CAP),
        "affine_relu_bf16": (pixels * (c // 8), span), "affine_relu_pool_bf16": (win * (c // 8), span),
        "maxpool_bwd_bf16": (pixels * (c // 8), span), "bn_bwd_apply_bf16": (pixels * (c // 8), span),
        "bn_bwd_apply_bf16/pool": (pixels * (c // 8), span),
    }
    if name == "bn_bwd_reduce<4>":
        blocks = bn_bwd_blocks_for(pixels, c, True)
        if blocks >= REDUCE_CAP:
            above(name, pixels * (c // 4), blocks * K_THREADS, into)
    elif name == "bn_bwd_reduce_pool":
        above(name, n * h, min(n * h, bn_bwd_blocks(pixels, c)), into)
    elif name.startswith("bn_bwd_reduce_bf16"):
        blocks = bn_bwd_blocks_bf16(pixels, c)
        if blocks >= REDUCE_CAP:
            above("bn_bwd_reduce_bf16", pixels * (c // 8), blocks * K_THREADS, into)
    elif name in table:
        above(name.split("/")[0], *table[name], into)


def _exact_operands(g, dev, bf, n, h, w, c):
    def ints(shape, lo, hi, density=None):
        v = torch.randint(lo, hi + 1, shape, generator=g, device=dev).float()
        if density is not None:
            v = v * (torch.rand(shape, generator=g, device=dev) < density)
        return v.to(BF) if bf and len(shape) == 4 else v
    y = ints((n, h, w, c), -6, 6)
    d_act = ints((n, h, w, c), -3, 3, 1.0 / 16)
    d_pooled = ints((n, h // 2, w // 2, c), -3, 3, 1.0 / 16)
    pw2 = lambda lo, hi: torch.pow(2.0, torch.randint(lo, hi + 1, (c,), generator=g, device=dev).float())   # noqa: E731
    invstd = pw2(-1, 1)
    scale = pw2(0, 2) * (1 - 2 * torch.randint(0, 2, (c,), generator=g, device=dev).float())     # +-{1, 2, 4}: y * scale is an integer
    co = {"mean": ints((c,), -2, 2), "invstd": invstd, "scale": scale, "gamma": scale / invstd,
          "shift": ints((c,), -3, 3) + 0.5}
    return y, d_act, d_pooled, co


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0].split(" (")[0].replace(" ", "_").replace(":", "") for c in EXACT_CASES])
def test_production_geometry_exact(dev, case):
    label, dt, n, h, w, c, with_bn, must = case
    bf = dt == "bf16"
    capped = set()                          # families this case itself puts above their cap
    g = torch.Generator(device=dev).manual_seed(700 + EXACT_CASES.index(case))
    y, d_act, d_pooled, co = _exact_operands(g, dev, bf, n, h, w, c)
    # forward: activation, pooled values and winners (ties among the ReLU zeros and among equal integers)
    want_act, want_pool, want_idx = ref_affine_pool(y, co["scale"], co["shift"], True)
    act, pooled, idx, name = run_affine(y, co["scale"], co["shift"], True)
    _mark_caps(name, y, capped)
    assert torch.equal(act, want_act) and torch.equal(pooled, want_pool) and torch.equal(idx, want_idx), (label, name)
    del pooled, want_pool
    act1, _, _, name1 = run_affine(y, co["scale"], co["shift"], True, want_pool=False)
    _mark_caps(name1, y, capped)
    assert torch.equal(act1, want_act), (label, name1)
    del act, act1, want_act
    # routing alone
    routed = ref_route(d_pooled, want_idx, y.shape)
    acc = d_act.clone()
    bname = run_maxpool_bwd(d_pooled, idx, acc)
    _mark_caps(bname, y, capped)
    assert torch.equal(acc.double(), d_act.double() + routed), (label, bname)
    del acc
    worst = {}
    if with_bn:
        for pool in (None, (d_pooled, idx)):
            ref = BnRef(d_act.double() + (0 if pool is None else routed), y, co)
            assert ref.margin >= 0.5 / (6 * 4 + 3.5), ref.margin                 # integer + 1/2: never near zero
            assert float(ref.abs_beta.max()) < GRID and float(ref.abs_gamma.max()) * 2 < GRID   # premise: grids 1 and 1/2
            dgamma, dbeta, dy, form = run_bn_bwd(d_act, y, co, pool)
            names = {"vec": ("bn_bwd_reduce<4>", "bn_bwd_apply<4>"), "pool": ("bn_bwd_reduce_pool", "bn_bwd_apply_pool"),
                     "bf16": ("bn_bwd_reduce_bf16", "bn_bwd_apply_bf16")}[form]
            for nm in names:
                _mark_caps(nm, y, capped)
            assert torch.equal(dbeta.double(), ref.dbeta), (label, form, float((dbeta.double() - ref.dbeta).abs().max()))
            assert torch.equal(dgamma.double(), ref.dgamma), (label, form, float((dgamma.double() - ref.dgamma).abs().max()))
            want_dy, dy_bound = ref.dy(dgamma, dbeta)
            if bf:
                close_bf16(dy, want_dy, (label, form, "dy"))
            else:
                worst["dy " + form] = ratio(dy, want_dy, dy_bound)
                assert worst["dy " + form] <= 1.0, (label, form, worst)
            del want_dy, dy_bound, ref
            inp = d_act.clone()
            dg2, db2, dy2, _ = run_bn_bwd(inp, y, co, pool, in_place=True)
            assert torch.equal(dy2, dy) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta), (label, form, "in place")
            del dy, dy2, inp
    missing = sorted(must - capped)
    assert not missing, (label, missing)
    ABOVE_CAP.update(capped)
    report_ratio("streaming exact %s" % label, "dy", max(worst.values()) if worst else 0.0,
                 dict(worst, pixels=n * h * w, above_cap=sorted(must)))
    del routed
    torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------- (c)
def test_every_streaming_kernel_ran(dev):
    """Runs last in this module: every label of COVERAGE was seen, no other, and every family ran above its cap."""
    missing = [k for k in COVERAGE if k not in SEEN]
    assert not missing, missing
    unknown = sorted(SEEN - set(COVERAGE))
    assert not unknown, unknown
    below = [f for f in FAMILIES if f not in ABOVE_CAP]
    assert not below, below
