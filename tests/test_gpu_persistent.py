"""Persistent-grid kernels with SEVERAL units per workgroup, against float64.

Every hot GEMM of the library runs a persistent grid sized from the usable CUs (common.h device_cu_count); each
workgroup walks a stream of (pixel patch x column tile) units (gemm_units.h).  At the default grid the kernel-level
parity tests mostly give a workgroup one unit, so the code that only runs from the second unit on -- the next unit's
prefetch, epilogues draining under the next unit, the carried cursor, resident weight images, input-patch reuse,
BatchNorm rows summed over several units, uneven tails -- is reached here by shrinking the grid with the data-parallel
knob (unetpp_set_reserved_cus), at 8, 13, 40 and all CUs.

Each case asserts the kernel the dispatcher chose, that the launcher's own unit / worker formulas give more units than
workgroups at the reduced settings, and parity with float64 under a-priori element-wise bounds (tests/helpers.py):
    direct / pointwise GEMM   |got - want| <= gamma_(taps K + 3) * (conv(|x|, |w|) + |b|)
    Winograd F(2x2,3x3)       |got - want| <= WINO_FACTOR * gamma_(K + 16) * (the same through |A^T|, |G|, |B^T|)
    BatchNorm sums per row    |sum got - sum y| <= gamma_(p + 2) * sum |y|   (p = pixels summed into the row)
next to the suite's 1e-4 relative bar; bf16 outputs keep close_bf16 (half an ulp + fp32 accumulation).  The worst
err / bound of every case is printed as one 'err/bound:' JSON line (visible with pytest -s).

Kernels covered (COVERAGE; test_every_kernel_ran_multi_unit checks each ran with more units than workgroups):
    fp32 forward     gemm_wino_kernel modes 0 / 1 / 2, narrow and wide columns, tile widths 8 / 16 / 32, with and
                     without per-workgroup BatchNorm rows, a concat whose workgroups cross image boundaries;
                     gemm_fast_kernel<9>, gemm_fast_kernel<1>, gemm_pw_kernel, small_cin_fwd_kernel (C = 1, 3 with
                     fp32 and bf16 output, C = 4 with bf16)
    fp32 dgrad       the 3x3 input gradient into two views: accumulate + gate of the sum, and a ReLU gate
    weight grads     wgrad_wino / pw / dma<1> / dma<9> / fast<9> / bf16 / bf16_quad at the DEFAULT target_blocks,
                     which ops.wgrad scales by usable / physical CUs
    bf16             gemm_bf16_dma_kernel<9> 8-wave (default dispatch) and 4-wave (statistics, one-chunk dgrad),
                     gemm_bf16_dma_kernel<1> into one and two column tiles, gemm_bf16_kernel<9> / <1> (fold on
                     load), gemm_pw_bf16_kernel, the bf16 head backward over several rounds of tiles
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import (WINO_FACTOR, bound_ratio, conv_magnitude, gamma, rel_err, report_ratio, usable_cus,
                           wino_magnitude)

pytestmark = pytest.mark.gpu

TOL = 1e-4
BF = torch.bfloat16
CU_SETTINGS = [8, 13, 40, None]    # None: every CU of the device
COVERAGE = [
    "gemm_wino_kernel/mode0", "gemm_wino_kernel/mode1", "gemm_wino_kernel/mode2",
    "gemm_wino_kernel/narrow", "gemm_wino_kernel/wide",
    "gemm_wino_kernel/tw8", "gemm_wino_kernel/tw16", "gemm_wino_kernel/tw32",
    "gemm_wino_kernel/bn_in_kernel", "gemm_wino_kernel/bn_per_block", "gemm_wino_kernel/cross_image",
    "gemm_wino_kernel/dgrad",
    "gemm_fast_kernel<9>", "gemm_fast_kernel<1>", "gemm_pw_kernel",
    "small_cin_fwd_kernel/C1", "small_cin_fwd_kernel/C3", "small_cin_fwd_kernel/C4",
    "small_cin_fwd_kernel/fp32", "small_cin_fwd_kernel/bf16",
    "wgrad_wino_kernel", "wgrad_pw_kernel", "wgrad_dma_kernel<1>", "wgrad_dma_kernel<9>", "wgrad_fast_kernel<9>",
    "wgrad_bf16_kernel<9>", "wgrad_bf16_quad_kernel<9>",
    "gemm_bf16_dma_kernel<9>/8wave", "gemm_bf16_dma_kernel<9>/8wave_groups", "gemm_bf16_dma_kernel<9>/4wave_stats",
    "gemm_bf16_dma_kernel<9>/in_reuse", "gemm_bf16_dma_kernel<1>/1tile", "gemm_bf16_dma_kernel<1>/2tiles",
    "gemm_bf16_kernel<9>", "gemm_bf16_kernel<1>", "gemm_pw_bf16_kernel", "head_bwd_bf16",
]
SEEN = set()      # coverage names that ran with more units than workgroups at a reduced grid
UNEVEN = set()    # kernels (name before '/') that ran with units % workgroups != 0 at a reduced grid
_KERNELS_NEED_UNEVEN = {"gemm_wino_kernel", "gemm_fast_kernel<9>", "gemm_fast_kernel<1>", "gemm_pw_kernel",
                        "small_cin_fwd_kernel", "gemm_bf16_dma_kernel<9>", "gemm_bf16_dma_kernel<1>",
                        "gemm_bf16_kernel<9>", "gemm_bf16_kernel<1>", "gemm_pw_bf16_kernel", "head_bwd_bf16"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib
    import ctypes
    phys = ctypes.c_int32(0)
    assert int(_lib.lib().unetpp_usable_cus(ctypes.byref(phys))) == phys.value   # the knob is back at 0


def last_kernel():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib.lib().unetpp_last_kernel_name().decode()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).double().cpu()


# ----------------------------------------------------------------------------------------- the launchers' formulas
def tile_geom(h, w):   # common.h tile_geom: 256-pixel patches, tile width 8 / 16 / 32
    l2 = 3
    while (1 << l2) < w and l2 < 5:
        l2 += 1
    tw, th = 1 << l2, 256 >> l2
    return l2, -(-w // tw), -(-h // th)


def col_tiles(cols, width=32):
    return sum(-(-c // width) for c in cols)


def multi_unit(u, names, units, workers, uneven_ok=True):
    """The launch's grid is min(units, workers); at a reduced setting it must hand some workgroup several units.
    names: coverage entries this launch stands for."""
    grid = min(units, workers)
    if u.cus < u.physical:
        assert units > grid, (names, u.cus, units, workers)
        SEEN.update(names)
        if uneven_ok and units % grid:
            UNEVEN.update(n.split("/")[0] for n in names)
    return grid


def wino_workers(cus):     # gemm_wino.hip launch_gemm_wino: (2 cus) & ~7, at least 8, at most kBnFusedRows
    return min(2048, max(8, (2 * cus) & ~7))


def contiguous_ranges(total, grid):
    """gemm_units.h my_contiguous_unit_range for every workgroup: [(first, count)]"""
    if grid >= total:
        return [(None, 1)] * grid   # one unit each (xcd_remap order; not needed here)
    w8 = grid >> 3
    q, r = total >> 3, total & 7
    out = []
    for bid in range(grid):
        xcd, widx = bid & 7, bid >> 3
        start = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
        cnt = q + (1 if xcd < r else 0)
        per, rem = cnt // w8, cnt % w8
        out.append((start + widx * per + min(widx, rem), per + (1 if widx < rem else 0)))
    return out


# ----------------------------------------------------------------------------------------- checks
def check_gemm(case, cus, got, want, mag, n_terms, wino):
    """got / want / mag NCHW.  The a-priori bound and the suite's 1e-4 bar."""
    g = gamma(n_terms) * (WINO_FACTOR if wino else 1.0)
    bound = (g * mag).clamp_max(TOL * float(want.abs().max()))   # never looser than the suite's 1e-4 bar anywhere
    ratio = bound_ratio(got, want, bound)
    report_ratio(case, "output", ratio, {"cus": cus, "n": n_terms, "factor": WINO_FACTOR if wino else 1.0})
    assert ratio <= 1.0, (case, cus, ratio)
    assert rel_err(got, want) < TOL, (case, cus)


def check_stat_sums(case, cus, rows_got, y, p):
    """rows_got [rows, C, 2] fp32 sums of `y` (float64 NCHW: the STORED tensor); p pixels at most in one row."""
    rows = rows_got.double().cpu()
    assert bool(torch.isfinite(rows).all()), (case, cus, "NaN in a written row")
    tot = rows.sum(0)
    yd = y.double()
    s, s2 = yd.sum((0, 2, 3)), (yd * yd).sum((0, 2, 3))
    a, a2 = yd.abs().sum((0, 2, 3)), s2
    r1 = bound_ratio(tot[:, 0], s, gamma(p + 2) * a)
    r2 = bound_ratio(tot[:, 1], s2, gamma(p + 2) * a2)
    report_ratio(case, "bn_sums", max(r1, r2), {"cus": cus, "p": p})
    assert r1 <= 1.0 and r2 <= 1.0, (case, cus, r1, r2)
    assert rel_err(tot[:, 1], s2) < TOL


def check_bn_finish(case, cus, fin, y, rm0, rv0, momentum, eps):
    yd = y.double().permute(0, 2, 3, 1).reshape(-1, y.shape[1])
    mean, var = yd.mean(0), yd.var(0, unbiased=False)
    cnt = yd.shape[0]
    invstd = 1 / (var + eps).sqrt()
    assert float((fin.mean.double().cpu() - mean).abs().max()) < 1e-5 * max(1.0, float(mean.abs().max())), (case, cus)
    assert rel_err(fin.invstd.cpu(), invstd) < 1e-5, (case, cus)
    assert rel_err(fin.scale.cpu(), fin.gamma.double().cpu() * invstd) < 1e-5, (case, cus)
    rm = (1 - momentum) * rm0 + momentum * mean
    rv = (1 - momentum) * rv0 + momentum * var * cnt / (cnt - 1)
    assert rel_err(fin.running_mean.cpu(), rm) < 1e-5, (case, cus)
    assert rel_err(fin.running_var.cpu(), rv) < 1e-5, (case, cus)


# ----------------------------------------------------------------------------------------- fp32 forward
FWD_CASES = [
    # id, (B, H, W, [cin per view], cout), options
    ("wino-lean-wide-tw32-bnrows", (2, 96, 64, [32], 64), dict(bn=True)),
    ("wino-general-slice-narrow-tw16", (4, 336, 16, [20], 16), dict(slice=(4, 28), relu=True, stats=True)),
    ("wino-fold-narrow-tw8-bnrows", (11, 256, 8, [16], 16), dict(fold=True, bn=True)),
    ("wino-concat-cross-image-gate-acc", (9, 40, 24, [16, 16, 8], 40), dict(gate=True, accumulate=True)),
    ("wino-fold-wide-stats", (2, 96, 64, [32], 48), dict(fold=True, relu=True, stats=True)),
    ("fast9-direct-relu-stats", (3, 96, 64, [32, 16], 48), dict(direct=True, relu=True, stats=True)),
    ("fast1-pointwise-accumulate", (6, 96, 64, [32, 16], 64), dict(taps=1, accumulate=True)),
    ("pw-relu", (3, 64, 112, [64], 64), dict(taps=1, relu=True)),
]


def _fwd_kernel(spec, opt):
    b, h, w, cins, co = spec
    taps = opt.get("taps", 9)
    if taps == 9:
        return "gemm_fast_kernel<9>" if opt.get("direct") else "gemm_wino_kernel"
    return "gemm_pw_kernel" if cins == [64] else "gemm_fast_kernel<1>"


def _fwd_coverage(spec, opt, kernel):
    b, h, w, cins, co = spec
    if kernel != "gemm_wino_kernel":
        return [kernel]
    l2, tx, ty = tile_geom(h, w)
    mode = 0 if "slice" in opt else (2 if opt.get("fold") else 1)
    names = ["mode%d" % mode, "narrow" if co <= 16 else "wide", "tw%d" % (1 << l2)]
    if opt.get("bn"):
        names.append("bn_in_kernel")
    if opt.get("stats"):
        names.append("bn_per_block")
    if len(cins) > 1:
        names.append("cross_image")
    return ["gemm_wino_kernel/" + n for n in names]


def _fwd_grid(spec, opt, cus):
    b, h, w, cins, co = spec
    taps = opt.get("taps", 9)
    kernel = _fwd_kernel(spec, opt)
    l2, tx, ty = tile_geom(h, w)
    stats = opt.get("stats") or opt.get("bn")
    if kernel == "gemm_wino_kernel":   # gemm_units.h fast_args (WNC = 32 columns per unit), gemm_wino.hip workers
        return b * ty * tx * col_tiles([co]), wino_workers(cus)
    if kernel == "gemm_fast_kernel<9>":   # gemm_fast.hip launch_gemm_fast: 3 per CU
        return b * ty * tx * col_tiles([co]), max(8, (3 * cus) & ~7)
    if kernel == "gemm_fast_kernel<1>":   # two column tiles per unit without statistics (fast_args), 3 / 4 per CU
        nt = col_tiles([co])
        ntu = 2 if (not stats and nt % 2 == 0) else 1
        return b * ty * tx * nt // ntu, max(8, ((3 if ntu == 2 else 4) * cus) & ~7)
    # gemm_pw.hip: 16-pixel row tiles, one per wave per turn; at most 16 waves per CU
    return b * h * (w // 16), 16 * cus


def _fwd_data(case, spec, opt):
    b, h, w, cins, co = spec
    taps = opt.get("taps", 9)
    g = torch.Generator().manual_seed(zlib.crc32(case.encode()))
    if "slice" in opt:
        off, width = opt["slice"]
        big = torch.randn(b, width, h, w, generator=g)
        xs_full, xs = [big], [big[:, off:off + cins[0]]]
    else:
        xs = xs_full = [torch.randn(b, c, h, w, generator=g) for c in cins]
    k = sum(cins)
    ks = 3 if taps == 9 else 1
    wt = torch.randn(co, k, ks, ks, generator=g) * (2.0 / (taps * k)) ** 0.5
    bias = 0.1 * torch.randn(co, generator=g)
    d = dict(xs=xs, xs_full=xs_full, wt=wt, bias=bias)
    if opt.get("fold"):
        d["scale"] = 1 + 0.3 * torch.randn(cins[0], generator=g)
        d["scale"][0] = 0.0
        d["shift"] = 0.3 * torch.randn(cins[0], generator=g)
    if opt.get("gate"):
        d["gate"] = torch.randn(b, co, h, w, generator=g)
    if opt.get("accumulate"):
        d["prev"] = torch.randn(b, co, h, w, generator=g)
    # float64 reference and magnitude on the operands the kernel sees (the fold: |x||s| + |h| bounds the fp32 transform)
    ops64 = [x.double() for x in xs]
    mags = [x.double().abs() for x in xs]
    if opt.get("fold"):
        s, t = d["scale"].double().view(1, -1, 1, 1), d["shift"].double().view(1, -1, 1, 1)
        ops64[0] = (ops64[0] * s + t).clamp_min(0)
        mags[0] = mags[0] * s.abs() + t.abs()
    pad = 1 if taps == 9 else 0
    x64, xm = torch.cat(ops64, 1), torch.cat(mags, 1)
    want = F.conv2d(x64, wt.double(), bias.double(), padding=pad)
    wino = taps == 9 and not opt.get("direct")
    mag = (wino_magnitude(xm, wt.abs(), bias.abs()) if wino else conv_magnitude(xm, wt.abs(), bias.abs(), padding=pad))
    n_terms = (k + 16) if wino else taps * k + 3
    if opt.get("relu"):
        want = want.clamp_min(0)
    if opt.get("gate"):
        keep = (d["gate"] > 0).double()
        want, mag = want * keep, mag * keep
    if opt.get("accumulate"):
        want, mag, n_terms = want + d["prev"].double(), mag + d["prev"].double().abs(), n_terms + 1
    d.update(want=want, mag=mag, n_terms=n_terms, wino=wino)
    return d


@pytest.mark.parametrize("case,spec,opt", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_fp32_forward_multi_unit(dev, case, spec, opt):
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    b, h, w, cins, co = spec
    taps = opt.get("taps", 9)
    d = _fwd_data(case, spec, opt)
    kernel = _fwd_kernel(spec, opt)
    xs_dev = [nhwc(x).to(dev) for x in d["xs_full"]]
    if "slice" in opt:
        ins = [V(xs_dev[0], c_off=opt["slice"][0], c_len=cins[0])]
    elif opt.get("fold"):
        ins = [V(xs_dev[0], scale=d["scale"].to(dev), shift=d["shift"].to(dev), relu=True)]
    else:
        ins = [V(x) for x in xs_dev]
    wp = engine.pack_conv_fwd(d["wt"].to(dev))
    bias = d["bias"].to(dev)
    for n in CU_SETTINGS:
        with usable_cus(n) as u:
            units, workers = _fwd_grid(spec, opt, u.cus)
            grid = multi_unit(u, [kernel] + _fwd_coverage(spec, opt, kernel), units, workers)
            if opt.get("accumulate"):
                out = nhwc(d["prev"]).to(dev)
            else:
                out = torch.full((b, h, w, co), float("nan"), device=dev)
            ov = V(out, relu=bool(opt.get("relu")), accumulate=bool(opt.get("accumulate")),
                   gate=nhwc(d["gate"]).to(dev) if opt.get("gate") else None)
            part, fin = None, None
            if opt.get("bn"):
                rows = ops.gemm_stats_rows(b, h, w)
                part = torch.full((rows * co * 2,), float("nan"), device=dev)
                gm, bt = 1 + 0.1 * torch.randn(co), 0.1 * torch.randn(co)
                rm0, rv0 = 0.1 * torch.randn(co), 1 + 0.1 * torch.rand(co)
                fin = ops.BatchNormFinish(gm.to(dev), bt.to(dev), rm0.to(dev), rv0.to(dev), 1e-5, 0.1, b * h * w)
            elif opt.get("stats"):
                part = torch.full((ops.gemm_pixel_blocks(b, h, w) * co * 2,), float("nan"), device=dev)
            ops.gemm_fwd(b, h, w, taps, ins, [ov], wp, bias, part, direct=bool(opt.get("direct")), bn=fin)
            torch.cuda.synchronize()
            assert last_kernel() == kernel, (case, u.cus, last_kernel())
            got = nchw(out)
            check_gemm(case, u.cus, got, d["want"], d["mag"], d["n_terms"], d["wino"])
            if opt.get("stats"):
                check_stat_sums(case, u.cus, part.view(-1, co, 2), got, 256)
            if opt.get("bn"):
                # per-workgroup rows: the first `grid` rows, each the sum over that workgroup's contiguous units
                # (gemm_units.h my_contiguous_unit_range), every unit 256 pixels of one 32-column group
                rows_got = part.view(-1, co, 2)[:grid].double().cpu()
                per = max(c for _, c in contiguous_ranges(units, grid))
                check_stat_sums(case, u.cus, rows_got, got, 256 * per)
                if units > grid:
                    _check_rows_per_workgroup(case, u.cus, rows_got, got, units, grid, h, w, co)
                check_bn_finish(case, u.cus, fin, got, rm0.double(), rv0.double(), 0.1, 1e-5)


def _check_rows_per_workgroup(case, cus, rows_got, y, units, grid, h, w, co):
    """Row r = the sums over the units workgroup r walked (decode_unit: column group fastest, then patch x, y, image)."""
    l2, tx, ty = tile_geom(h, w)
    tw, th = 1 << l2, 256 >> l2
    n_groups = col_tiles([co])
    yd = y.double()
    want = torch.zeros(grid, co, 2, dtype=torch.float64)
    mag = torch.zeros(grid, co, 2, dtype=torch.float64)
    for r, (first, cnt) in enumerate(contiguous_ranges(units, grid)):
        for unit in range(first, first + cnt):
            grp, patch = unit % n_groups, unit // n_groups
            txi, tyi, img = patch % tx, (patch // tx) % ty, patch // (tx * ty)
            c0, c1 = grp * 32, min(co, grp * 32 + 32)
            blk = yd[img, c0:c1, tyi * th:(tyi + 1) * th, txi * tw:(txi + 1) * tw]
            want[r, c0:c1, 0] += blk.sum((1, 2))
            want[r, c0:c1, 1] += (blk * blk).sum((1, 2))
            mag[r, c0:c1, 0] += blk.abs().sum((1, 2))
            mag[r, c0:c1, 1] += (blk * blk).sum((1, 2))
    per = max(c for _, c in contiguous_ranges(units, grid))
    ratio = bound_ratio(rows_got, want, gamma(256 * per + 2) * mag + 1e-30)
    report_ratio(case, "bn_rows_per_workgroup", ratio, {"cus": cus})
    assert ratio <= 1.0, (case, cus, ratio)


# ----------------------------------------------------------------------------------------- fp32 input gradient
def test_fp32_conv3x3_dgrad_multi_unit(dev):
    """engine.pack_conv_dgrad into two views as _pair_bwd issues them: accumulate + gate of the sum (in_targets of a
    concat input) and a plain ReLU gate (d_a1), against autograd in float64."""
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    case = "wino-dgrad-two-views"
    b, h, w, ci, co = 2, 96, 64, 48, 32
    g = torch.Generator().manual_seed(21)
    x = torch.randn(b, ci, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    wt = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
    dy = torch.randn(b, co, h, w, generator=g)
    F.conv2d(x, wt.double(), None, padding=1).backward(dy.double())
    gate = torch.randn(b, ci, h, w, generator=g)
    prev = torch.randn(b, 24, h, w, generator=g)
    keep = (gate > 0).double()
    want = x.grad.clone()
    want[:, :24] += prev.double()
    want = want * keep
    wd = wt.double().flip(2, 3).transpose(0, 1)          # the input gradient as a convolution of dy
    mag = wino_magnitude(dy.double().abs(), wd.abs())
    mag[:, :24] += prev.double().abs()
    mag = mag * keep
    wp = engine.pack_conv_dgrad(wt.to(dev))
    dyd = nhwc(dy).to(dev)
    for n in CU_SETTINGS:
        with usable_cus(n) as u:
            l2, tx, ty = tile_geom(h, w)
            multi_unit(u, ["gemm_wino_kernel", "gemm_wino_kernel/dgrad"], b * ty * tx * 2, wino_workers(u.cus))
            d0 = nhwc(prev).to(dev)
            d1 = torch.full((b, h, w, 24), float("nan"), device=dev)
            gd = nhwc(gate).to(dev)
            ops.gemm_fwd(b, h, w, 9, [V(dyd)], [V(d0, accumulate=True, gate=gd[..., :24].contiguous(), gate_sum=True),
                                                V(d1, gate=gd[..., 24:].contiguous())], wp)
            torch.cuda.synchronize()
            assert last_kernel() == "gemm_wino_kernel", last_kernel()
            got = torch.cat([nchw(d0), nchw(d1)], 1)
            check_gemm(case, u.cus, got, want, mag, co + 16 + 1, True)


# ----------------------------------------------------------------------------------------- first layer
# (C = 4 with an fp32 output is aligned: it takes the Winograd kernel, so four channels run with the bf16 output only)
SMALL_CASES = [(1, "fp32", True), (3, "fp32", True), (1, "bf16", False), (3, "bf16", False), (4, "bf16", False)]


@pytest.mark.parametrize("cin,out_dtype,bn", SMALL_CASES, ids=["C%d-%s%s" % (c, d, "-bnrows" if s else "") for c, d, s in SMALL_CASES])
def test_first_layer_multi_unit(dev, cin, out_dtype, bn):
    from tests.test_gpu_bf16 import close_bf16
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    case = "small-cin-C%d-%s" % (cin, out_dtype)
    b, h, w, co = 3, 128, 120, 32
    g = torch.Generator().manual_seed(30 + cin)
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(co, cin, 3, 3, generator=g) * 0.3
    bias = 0.1 * torch.randn(co, generator=g)
    want = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    mag = conv_magnitude(x.abs(), wt.abs(), bias.abs())
    dt = torch.float32 if out_dtype == "fp32" else BF
    xd = nhwc(x).to(dev)
    for n in CU_SETTINGS:
        with usable_cus(n) as u:
            l2, tx, ty = tile_geom(h, w)
            # first_layer.hip launch_small_cin_fwd: n_patches = N tiles_y tiles_x, workers = cus * (3 | 4)
            grid = multi_unit(u, ["small_cin_fwd_kernel", "small_cin_fwd_kernel/C%d" % cin,
                                  "small_cin_fwd_kernel/" + out_dtype], b * ty * tx, min(2048, u.cus * (3 if cin >= 3 else 4)))
            y = torch.full((b, h, w, co), float("nan"), dtype=dt, device=dev)
            fin, part = None, None
            if bn:
                part = torch.full((ops.gemm_stats_rows(b, h, w) * co * 2,), float("nan"), device=dev)
                fin = ops.BatchNormFinish(torch.ones(co, device=dev), torch.zeros(co, device=dev), torch.zeros(co, device=dev),
                                          torch.ones(co, device=dev), 1e-5, 0.1, b * h * w)
            ops.gemm_fwd(b, h, w, 9, [V(xd)], [V(y)], engine.pack_conv_fwd(wt.to(dev)), bias.to(dev), part, bn=fin)
            torch.cuda.synchronize()
            assert last_kernel() == "small_cin_fwd_kernel", last_kernel()
            got = nchw(y)
            if out_dtype == "fp32":
                check_gemm(case, u.cus, got, want, mag, 9 * cin + 3, False)
            else:
                close_bf16(got, want, case)
            if bn:
                rows_got = part.view(-1, co, 2)[:grid]
                per = -(-(b * ty * tx) // grid)
                check_stat_sums(case, u.cus, rows_got, got, 256 * per)
                check_bn_finish(case, u.cus, fin, got, torch.zeros(co, dtype=torch.float64),
                                torch.ones(co, dtype=torch.float64), 0.1, 1e-5)


# ----------------------------------------------------------------------------------------- weight gradients
WGRAD_CASES = [
    # id, kernel, (B, H, W, cin, cout), form
    ("wgrad-wino", "wgrad_wino_kernel", (2, 32, 48, 32, 32), "plain"),
    ("wgrad-dma9", "wgrad_dma_kernel<9>", (2, 32, 48, 16, 16), "direct"),
    ("wgrad-fast9", "wgrad_fast_kernel<9>", (2, 32, 32, 32, 32), "fold-direct"),
    ("wgrad-pw", "wgrad_pw_kernel", (2, 16, 32, 64, 32), "deconv"),
    ("wgrad-dma1", "wgrad_dma_kernel<1>", (1, 8, 8, 64, 16), "deconv"),
    ("wgrad-bf16", "wgrad_bf16_kernel<9>", (2, 32, 32, 32, 32), "bf16"),
    ("wgrad-bf16-quad", "wgrad_bf16_quad_kernel<9>", (2, 32, 64, 64, 64), "bf16"),
]
# case -> (pairs_per_workgroup, max_split) as commit 83ca35a's unetpp_wgrad_pairs_per_workgroup / unetpp_wgrad_max_split
# answered for the descriptors of WGRAD_CASES (recorded on the CPU from that commit's library)
WGRAD_RECORDED = {"wgrad-wino": (1, 16), "wgrad-dma9": (1, 16), "wgrad-fast9": (1, 8), "wgrad-pw": (8, 4), "wgrad-dma1": (1, 1),
                  "wgrad-bf16": (1, 8), "wgrad-bf16-quad": (4, 16)}


def split_before_the_plan(target, pairs, pairs_per_workgroup, max_split, usable, physical, bf16, one_narrow_x=False):
    """n_split as ops.wgrad of commit 83ca35a computed it in Python, rule for rule"""
    if one_narrow_x:
        target = 1024
    if 0 < usable < physical:
        target = max(8, target * usable // physical)
    if bf16 and target == 256 and pairs_per_workgroup == 1:
        target = 512
    return max(1, min(max_split, target // max(1, pairs // max(1, pairs_per_workgroup))))


@pytest.mark.parametrize("case,kernel,spec,form", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad_default_split_at_reduced_grids(dev, case, kernel, spec, form):
    """ops.wgrad's DEFAULT target_blocks, which it scales by usable / physical CUs (and, for bf16, no longer doubles
    from 256 to 512 once scaled), against autograd in float64 on the operands the kernel reads."""
    from tests.test_gpu_bf16 import rb
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    b, h, w, ci, co = spec
    g = torch.Generator().manual_seed(40)
    x = torch.randn(b, ci, h, w, generator=g)
    if form == "deconv":
        wt = torch.randn(ci, co, 2, 2, generator=g, dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(co, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(b, co, 2 * h, 2 * w, generator=g)
        F.conv_transpose2d(x.double(), wt, bias, stride=2).backward(dy.double())
    else:
        xin = x.double()
        scale = shift = None
        if form == "fold-direct":
            scale, shift = torch.randn(ci, generator=g), torch.randn(ci, generator=g)
            xin = (xin * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).clamp_min(0)
        if form == "bf16":
            xin = rb(x)
        wt = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(co, dtype=torch.float64, requires_grad=True)
        dy = torch.randn(b, co, h, w, generator=g)
        F.conv2d(xin, wt, bias, padding=1).backward(rb(dy) if form == "bf16" else dy.double())
    for n in CU_SETTINGS:
        with usable_cus(n) as u:
            dw = torch.full(tuple(wt.shape), float("nan"), device=dev)
            db = torch.full((co,), float("nan"), device=dev)
            if form == "deconv":
                plan = ops.wgrad(b, h, w, 1, [V(nhwc(x).to(dev))], engine._phase_views(nhwc(dy).to(dev)), dw, (0, 4 * co, 4, 1),
                                 db, n_inner=co)
            elif form == "bf16":
                plan = ops.wgrad(b, h, w, 9, [V(nhwc(x).to(BF).to(dev))], [V(nhwc(dy).to(BF).to(dev))], dw, (1, 9, ci * 9, 0), db)
            else:
                xv = V(nhwc(x).to(dev)) if scale is None else V(nhwc(x).to(dev), scale=scale.to(dev), shift=shift.to(dev), relu=True)
                plan = ops.wgrad(b, h, w, 9, [xv], [V(nhwc(dy).to(dev))], dw, (1, 9, ci * 9, 0), db, direct=form != "plain")
            torch.cuda.synchronize()
            assert last_kernel() == kernel, (case, u.cus, last_kernel())
            assert plan.kernel.decode() == last_kernel(), (case, u.cus, plan.kernel)   # the plan names the kernel that ran
            pairs = -(-ci // 32) * -(-co // 32) * (4 if form == "deconv" else 1)
            want_split = split_before_the_plan(256, pairs, *WGRAD_RECORDED[case], u.cus, u.physical, form == "bf16")
            assert plan.n_split == want_split, (case, u.cus, plan.n_split, want_split)
            assert plan.pairs_per_workgroup == WGRAD_RECORDED[case][0]
            if u.cus < u.physical:
                SEEN.add(kernel)
            r1, r2 = rel_err(dw.cpu(), wt.grad), rel_err(db.cpu(), bias.grad)
            report_ratio(case, "rel_err/1e-4", max(r1, r2) / TOL, {"cus": u.cus})
            assert r1 < TOL and r2 < TOL, (case, u.cus, r1, r2)


# ----------------------------------------------------------------------------------------- bf16 GEMMs
def bf16_dma8_units(b, h, w, nt):
    l2, tx, _ = tile_geom(h, w)
    return b * -(-h // 16) * tx * (nt // 2 if nt % 2 == 0 else nt)


BF16_CASES = [
    # id, coverage names, (B, H, W, [cin per view], cout), form
    ("dma9-8wave", ["gemm_bf16_dma_kernel<9>/8wave"], (4, 96, 128, [64], 32), "plain"),
    ("dma9-8wave-groups", ["gemm_bf16_dma_kernel<9>/8wave_groups"], (2, 80, 128, [32], 128), "plain"),
    ("dma9-4wave-stats", ["gemm_bf16_dma_kernel<9>/4wave_stats"], (3, 96, 64, [32], 64), "stats"),
    ("dma9-in-reuse-dgrad", ["gemm_bf16_dma_kernel<9>/in_reuse"], (2, 96, 64, [32], 64), "dgrad"),
    ("dma1-one-tile", ["gemm_bf16_dma_kernel<1>/1tile"], (4, 128, 120, [32, 32, 32], 32), "pointwise"),
    ("dma1-two-tiles", ["gemm_bf16_dma_kernel<1>/2tiles"], (4, 128, 120, [32, 32, 32], 64), "pointwise"),
    ("reg9-fold", ["gemm_bf16_kernel<9>"], (4, 96, 64, [32], 64), "fold"),
    ("reg1-fold", ["gemm_bf16_kernel<1>"], (4, 128, 120, [64], 64), "fold1"),
    ("pw-bf16-deconv", ["gemm_pw_bf16_kernel"], (4, 64, 80, [64], 32), "deconv"),
]


def _bf16_kernel_and_grid(form, spec, cus):
    """(kernel name, units, workers) by gemm_bf16_dma.hip launch_gemm_bf16_dma / gemm_bf16.hip launch_gemm_bf16 /
    gemm_pw_bf16.hip"""
    b, h, w, cins, co = spec
    l2, tx, ty = tile_geom(h, w)
    if form == "deconv":
        return "gemm_pw_bf16_kernel", b * h * (w // 16), 16 * cus
    if form in ("fold", "fold1"):
        taps = 1 if form == "fold1" else 9
        nt = col_tiles([co])
        ntu = 2 if nt % 2 == 0 else 1          # no statistics: bf16_gemm_args / fast_args take two tiles per unit
        return "gemm_bf16_kernel<%d>" % taps, b * ty * tx * nt // ntu, max(8, (2 * cus) & ~7)
    if form == "pointwise":
        nt = col_tiles([co])
        ntu = 2 if nt % 2 == 0 else 1
        return "gemm_bf16_dma_kernel<1>", b * ty * tx * nt // ntu, max(8, (3 * cus) & ~7)   # plain outputs: 3 per CU
    nt = col_tiles([co])   # (dgrad: dy has cins channels, dx co)
    chunks = sum(-(-c // 32) for c in cins)
    units8 = bf16_dma8_units(b, h, w, nt)
    if form != "stats" and l2 == 5 and (chunks > 1 or nt > 1) and units8 >= 2 * cus:
        return "gemm_bf16_dma_kernel<9>", units8, max(8, cus & ~7)         # the 8-wave form: one per CU
    return "gemm_bf16_dma_kernel<9>", b * ty * tx * nt, max(8, (2 * cus) & ~7)   # 4-wave: one tile per unit, 2 per CU


@pytest.mark.parametrize("case,names,spec,form", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_bf16_gemm_multi_unit(dev, case, names, spec, form):
    from tests.test_gpu_bf16 import close_bf16, close_f32, rb
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    b, h, w, cins, co = spec
    g = torch.Generator().manual_seed(60)
    k = sum(cins)
    xs = [torch.randn(b, c, h, w, generator=g) for c in cins]
    xin = [rb(x) for x in xs]
    xd = [nhwc(x).to(BF).to(dev) for x in xs]
    views = [V(t) for t in xd]
    if form == "deconv":
        wt = torch.randn(k, co, 2, 2, generator=g) * 0.1
        bias = 0.1 * torch.randn(co, generator=g)
        want = F.conv_transpose2d(xin[0], rb(wt), bias.double(), stride=2)
        wp, bias_d = engine.pack_deconv_fwd(wt.to(dev)), engine.tile_bias4(bias.to(dev))
    else:
        taps = 1 if form in ("pointwise", "fold1") else 9
        if form == "dgrad":   # dgrad of a conv co -> k: w [k, co, 3, 3]; dy has k (= cins) channels, dx co
            wt = torch.randn(k, co, 3, 3, generator=g) * (2.0 / (9 * co)) ** 0.5
            want = F.conv2d(torch.cat(xin, 1), rb(wt).flip(2, 3).transpose(0, 1), None, padding=1)
            wp, bias, bias_d = engine.pack_conv_dgrad(wt.to(dev)), None, None
        else:
            ks = 3 if taps == 9 else 1
            wt = torch.randn(co, k, ks, ks, generator=g) * (2.0 / (taps * k)) ** 0.5
            bias = 0.1 * torch.randn(co, generator=g)
            if form in ("fold", "fold1"):
                scale, shift = 1 + 0.2 * torch.randn(cins[0], generator=g), 0.3 * torch.randn(cins[0], generator=g)
                views[0] = V(xd[0], scale=scale.to(dev), shift=shift.to(dev), relu=True)
                xin[0] = rb((xin[0] * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).clamp_min(0).float())
            want = F.conv2d(torch.cat(xin, 1), rb(wt), bias.double(), padding=1 if taps == 9 else 0)
            wp, bias_d = engine.pack_conv_fwd(wt.to(dev)), bias.to(dev)
    oh, ow = (2 * h, 2 * w) if form == "deconv" else (h, w)
    for n in CU_SETTINGS:
        with usable_cus(n) as u:
            kernel, units, workers = _bf16_kernel_and_grid(form, spec, u.cus)
            grid = multi_unit(u, [kernel] + names, units, workers)
            y = torch.full((b, oh, ow, co), float("nan"), dtype=BF, device=dev)
            part = None
            if form == "stats":
                part = torch.full((ops.gemm_pixel_blocks(b, h, w) * co * 2,), float("nan"), device=dev)
            outs = engine._phase_views(y) if form == "deconv" else [V(y)]
            ops.gemm_fwd(b, h, w, 1 if form in ("deconv", "pointwise", "fold1") else 9, views, outs, wp, bias_d, part)
            torch.cuda.synchronize()
            assert last_kernel() == kernel, (case, u.cus, last_kernel(), units, workers)
            got = nchw(y)
            close_bf16(got, want, "%s cus=%d" % (case, u.cus))
            report_ratio(case, "close_bf16", bound_ratio(got, want, 2.0 ** -8 * want.abs() + 1e-5 * float(want.abs().max())),
                         {"cus": u.cus, "units": units, "grid": grid})
            if form == "stats":
                rows = part.view(-1, co, 2).double().sum(0).cpu()
                close_f32(rows[:, 0], got.sum((0, 2, 3)), 1e-4, "sum")
                close_f32(rows[:, 1], (got * got).sum((0, 2, 3)), 1e-4, "sum of squares")


def test_bf16_head_backward_several_rounds(dev):
    """The bf16 head backward: at most HEAD_WGS_PER_CU (4) workgroups per CU take 256-pixel tiles, so a reduced grid
    walks several rounds of them (heads.hip); dx (accumulate + gate), dW and db against float64."""
    from tests.test_gpu_bf16 import close_bf16, close_f32
    from unet_nested4tiny_objects_keypoints_amd import ops
    b, h, w, c, n_cls = 4, 128, 100, 32, 4
    g = torch.Generator().manual_seed(70)
    x = torch.randn(b, h, w, c, generator=g).to(BF)
    wt = torch.randn(n_cls, c, generator=g) * 0.2
    bias = torch.randn(n_cls, generator=g) * 0.1
    d_out = torch.randn(b, n_cls, h, w, generator=g)
    old = torch.randn(b, h, w, c, generator=g).to(BF)
    logits = torch.einsum("nhwc,kc->nkhw", x.double(), wt.double()) + bias.double().view(1, -1, 1, 1)
    p = torch.sigmoid(logits)
    dl = d_out.double() * p * (1 - p)
    want_dx = (torch.einsum("nkhw,kc->nhwc", dl, wt.double()) + old.double()) * (x.double() > 0)
    want_dw, want_db = torch.einsum("nkhw,nhwc->kc", dl, x.double()), dl.sum((0, 2, 3))
    xd = x.to(dev)
    for n in CU_SETTINGS:
        with usable_cus(n) as u:
            tiles = -(-(b * h * w) // 256)
            multi_unit(u, ["head_bwd_bf16"], tiles, 4 * u.cus)
            out = torch.empty(b, n_cls, h, w, device=dev)
            ops.head_fwd(xd, wt.to(dev), bias.to(dev), 0.0, 1, None, out)
            close_f32(out, p, 2e-5, "head forward")
            dx = old.clone().to(dev)
            dw, db = ops.head_bwd(d_out.to(dev), out, xd, wt.to(dev), 0.0, 1, None, dx, True, True)
            torch.cuda.synchronize()
            close_bf16(dx, want_dx, "head dx cus=%d" % u.cus)
            close_f32(dw.view(n_cls, c), want_dw, 1e-4, "head dW")
            close_f32(db, want_db, 1e-4, "head db")


# ----------------------------------------------------------------------------------------- whole network at 8 CUs
def test_fp32_train_step_vs_oracle_on_eight_cus(dev):
    """test_gpu_model's base-32 ORACLE_CASES entry with every persistent grid sized for 8 CUs (its own bounds)."""
    import tests.test_gpu_model as tgm
    case = next(c for c in tgm.ORACLE_CASES if c[0] == dict(in_channels=1, n_classes=4, feature_scale=1) and c[1:4] == (2, 64, 64))
    with usable_cus(8):
        tgm.test_train_step_vs_oracle(dev, case)


def test_bf16_train_step_vs_oracles_on_eight_cus(dev):
    """test_gpu_bf16's base-32 train step with every persistent grid sized for 8 CUs (its own bounds)."""
    import tests.test_gpu_bf16 as tgb
    with usable_cus(8):
        tgb.test_bf16_train_step_vs_oracles(dev, dict(in_channels=1, n_classes=4, feature_scale=1), 2, 64, 64)


def test_every_kernel_ran_multi_unit(dev):
    """Runs last in this module: every entry of COVERAGE ran with more units than workgroups at a reduced grid, and every
    kernel at least once with units that do not divide evenly among the workgroups."""
    missing = [n for n in COVERAGE if n not in SEEN]
    assert not missing, missing
    uneven = sorted(_KERNELS_NEED_UNEVEN - UNEVEN)
    assert not uneven, uneven
