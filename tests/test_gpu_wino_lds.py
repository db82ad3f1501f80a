"""Winograd GEMM (gemm_wino.hip): exact per-element tests on integer data, at the smallest shapes at which the LDS side of
its chunk loop can go wrong -- the channel-planar input patch of the lean instantiations and its staging (halo, dummy
items behind the patch), the 16-byte weight-fragment reads of the repacked image, the one-instruction floor of the fold
and of the epilogue (profiles/wino_lds/).

Data on which F(2x2,3x3) in fp32 is exact: inputs are integers in -4..4, weights multiples of 4 in -8..8, so U = G g G^T
is integral (|U| <= 18), a transformed window element is at most 4 * 11 = 44 in magnitude (11 = the largest folded
input, 2 * 4 + 3), and a whole output is below 9 * 24 * 11 * 8 < 2^15: every product, partial sum and transform step is
an integer far below 2^24, whatever the order.  The outputs are therefore compared BIT FOR BIT with a float64 direct
convolution computed on the CPU (once per shape and channel list, shared by the variants).

Shapes: a patch is 32 x 8 pixels.  8x32 = one patch, every halo pixel outside the image; 16x64 (two images) = border
patches only; 24x96 = one interior patch among eight border ones; 10x40 = ragged patches, run through the lean kernels
(general epilogue) and, with the lean forms switched off, through the general kernel, whose pixel-major patch is as it was.
Channels: one chunk (8), two (16), a chunk walk across two views (8 + 16); 16 columns (half tile), 32, and 40 (a second,
partial column tile).

BatchNorm partial sums: per 256-pixel block the plain sum is at most 256 * 6912 < 2^24 in magnitude, so it is exact in
any order and compared exactly.  The sum of squares is not (a square reaches 4.8e7): each of its at most 258 additions /
fused multiply-adds rounds once, relative error 2^-24 each on non-negative terms, so it is held to 258 * 2^-24 of the
float64 value.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 32), (2, 16, 64), (1, 24, 96), (1, 10, 40)]
CHANNELS = [([8], 16), ([16], 32), ([8, 16], 40), ([8], 40), ([8, 16], 16), ([16], 16), ([8, 16], 32)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def nhwc(t):  # NCHW cpu -> NHWC gpu
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def nchw(t):  # NHWC gpu -> NCHW cpu
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def case(shape, cins, co):
    """Integer data and the float64 references of one (shape, channel list): computed once, never modified."""
    b, h, w = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * sum(cins) + co)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    d = {}
    d["xs"] = [ri(-4, 4, b, c, h, w) for c in cins]
    d["wt"] = ri(-2, 2, co, sum(cins), 3, 3) * 4
    d["bias"] = ri(-5, 5, co)
    # fold: integer scale in -2..2 with a negative one in channel 1, integer shift in 1..3 (so that a padding pixel that
    # went through the fold would read max(shift, 0) > 0 instead of zero)
    d["scale"] = [ri(-2, 2, c) for c in cins]
    d["shift"] = [ri(1, 3, c) for c in cins]
    for s in d["scale"]:
        s[1] = -2.0
    d["gate"] = ri(-1, 1, b, co, h, w)
    d["prev"] = ri(-9, 9, b, co, h, w)
    x = torch.cat(d["xs"], 1)
    xf = torch.cat([F.relu(xx * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
                    for xx, sc, sh in zip(d["xs"], d["scale"], d["shift"])], 1)
    d["plain"] = F.conv2d(x, d["wt"], d["bias"], padding=1)
    d["fold"] = F.relu(F.conv2d(xf, d["wt"], d["bias"], padding=1))
    d["gated"] = d["prev"] + F.conv2d(x, d["wt"], None, padding=1) * (d["gate"] > 0)
    return d


def gpu_inputs(d):
    from unet_nested4tiny_objects_keypoints_amd import engine
    xs = [nhwc(x.float()) for x in d["xs"]]
    wp = engine.pack_conv_fwd(d["wt"].float().cuda())
    return xs, wp, d["bias"].float().cuda()


def run_variants(dev, shape, cins, co, label):
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    b, h, w = shape
    d = case(shape, tuple(cins), co)
    xs, wp, bias = gpu_inputs(d)
    # plain (mode 1), with the per-block BatchNorm partial sums
    out = torch.full((b, h, w, co), float("nan"), device=dev)
    blocks = ops.gemm_pixel_blocks(b, h, w)
    part = torch.full((blocks * co * 2,), float("nan"), device=dev)
    ops.gemm_fwd(b, h, w, 9, [V(x) for x in xs], [V(out)], wp, bias, part)
    assert _lib.lib().unetpp_last_kernel_name().decode() == "gemm_wino_kernel"
    assert same_bits(nchw(out), d["plain"].float()), label + " plain"
    sums = part.view(blocks, co, 2).cpu()
    s1, s2 = sums[:, :, 0].double().sum(0), sums[:, :, 1].double()
    assert torch.equal(s1, d["plain"].sum((0, 2, 3))), label + " partial sums"
    # per block the sum of squares rounds at most 258 times (module docstring); summed over blocks in float64 here
    ref2 = (d["plain"] ** 2).sum((0, 2, 3))
    assert bool(((s2.sum(0) - ref2).abs() <= 258 * 2.0 ** -24 * ref2).all()), label + " sums of squares"
    # BatchNorm fold on load with a negative scale and ReLU (mode 2), ReLU in the epilogue
    out = torch.full((b, h, w, co), float("nan"), device=dev)
    ins = [V(x, scale=sc.float().cuda(), shift=sh.float().cuda(), relu=True) for x, sc, sh in zip(xs, d["scale"], d["shift"])]
    ops.gemm_fwd(b, h, w, 9, ins, [V(out, relu=True)], wp, bias)
    assert same_bits(nchw(out), d["fold"].float()), label + " fold"
    # gate + accumulate (input-gradient form)
    acc = nhwc(d["prev"].float())
    ops.gemm_fwd(b, h, w, 9, [V(x) for x in xs], [V(acc, gate=nhwc(d["gate"].float()), accumulate=True)], wp)
    assert same_bits(nchw(acc), d["gated"].float()), label + " gate + accumulate"
    # BatchNorm sums as one row per workgroup (the BNF instantiations), finished by the library: the stored tensor is the
    # same bits; mean and 1/std against float64 within the fp32 finalize's 1e-5 (tests/test_gpu_kernels.py)
    out = torch.full((b, h, w, co), float("nan"), device=dev)
    gamma, beta = torch.ones(co, device=dev), torch.zeros(co, device=dev)
    fin = ops.BatchNormFinish(gamma, beta, torch.zeros(co, device=dev), torch.ones(co, device=dev), 1e-5, 0.1, b * h * w)
    work = torch.full((ops.gemm_stats_rows(b, h, w) * co * 2,), float("nan"), device=dev)
    ops.gemm_fwd(b, h, w, 9, [V(x) for x in xs], [V(out)], wp, bias, work, bn=fin)
    assert same_bits(nchw(out), d["plain"].float()), label + " BNF output"
    mean, var = d["plain"].mean((0, 2, 3)), d["plain"].var((0, 2, 3), unbiased=False)
    assert float((fin.mean.cpu().double() - mean).abs().max()) <= 1e-5 * max(1.0, float(mean.abs().max())), label + " BNF mean"
    inv = 1 / (var + 1e-5).sqrt()
    assert float((fin.invstd.cpu().double() - inv).abs().max()) <= 1e-5 * float(inv.max()), label + " BNF invstd"


@pytest.mark.parametrize("cins,co", CHANNELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_wino_exact_on_integer_data(dev, shape, cins, co):
    run_variants(dev, shape, cins, co, "lean")


@pytest.mark.parametrize("cins,co", CHANNELS[:3])
def test_wino_general_kernel_exact(dev, cins, co):
    """10x40 with the lean forms switched off: the general instantiation (pixel-major patch) reads the repacked weight
    image too."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    with ops._lib.debug_switch("WINO_NO_LEAN", 1):
        run_variants(dev, SHAPES[3], cins, co, "general")


@pytest.mark.parametrize("fold", [False, True])
def test_wino_nan_and_negative_zero(dev, fold):
    """A NaN and a -0.0 in the input: NaN in exactly the output elements in which the direct kernel has one, with and
    without the fold + ReLU on load and with the ReLU in the epilogue (both go through the one-instruction floor); every
    other element is the same bits as the direct kernel's, zeros included.  With the fold (scale 1, shift -0.0, ReLU) the
    -0.0 inputs are staged as max(-0.0, +0) = +0.0, and the result equals that of the same input with +0.0 in their place."""
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    b, h, w, c, co = 1, 24, 96, 16, 32
    d = case((b, h, w), (c,), co)
    x = d["xs"][0].float().clone()
    x[0, 3, 9, 40] = float("nan")      # interior patch
    x[0, 10, 0, 0] = float("nan")      # image corner, second chunk
    x[0, :, 12:14, 50:60] = -0.0
    x[0, 5, 20, :] = -0.0
    wp = engine.pack_conv_fwd(d["wt"].float().cuda())
    bias = d["bias"].float().cuda()
    kw = dict(scale=torch.ones(c, device=dev), shift=torch.full((c,), -0.0, device=dev), relu=True) if fold else {}

    def run(xin, direct):
        out = torch.full((b, h, w, co), 7.0, device=dev)
        ops.gemm_fwd(b, h, w, 9, [V(nhwc(xin), **kw)], [V(out, relu=True)], wp, bias, direct=direct)
        return nchw(out)

    wino, direct = run(x, False), run(x, True)
    assert torch.equal(wino.isnan(), direct.isnan())
    assert 0 < int(wino.isnan().sum()) <= 2 * 9 * co
    keep = ~direct.isnan()
    assert same_bits(wino[keep], direct[keep])
    xpos = torch.where(x == 0, torch.zeros_like(x), x)   # -0.0 -> +0.0
    assert same_bits(run(xpos, False)[keep], wino[keep])
    # against float64, away from the NaNs
    xin = F.relu(xpos.double()) if fold else xpos.double()
    ref = F.relu(F.conv2d(torch.nan_to_num(xin), d["wt"], d["bias"], padding=1)).float()
    assert same_bits(wino[keep], ref[keep])
