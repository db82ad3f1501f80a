"""Weight-gradient kernels and their finish kernels, every element of dW and db, against tests/wgrad_oracle.py.

Tier A (TIER_A): small-integer operands.  Every product, partial sum, Winograd transform and the finish's multiples of
1/4 are exact in fp32 as long as wgrad_oracle.exactness_margin < 2^22 (asserted for every row on the CPU, in
tests/test_wgrad_oracle_host.py), so the kernels must EQUAL the float64 oracle in any summation order and for any
split: a dropped, duplicated, stale or misplaced term fails, whatever its size.
Tier B (TIER_B): impulses in dy against full-mantissa x.  dW[:, k, i] is the 3x3 window of x around impulse pixel i: a
copy for every direct-sum kernel (equality), and for wgrad_wino_kernel within gamma(WINO_ROUNDINGS) of the window's
magnitude through the transforms.  This is the tier that sees a lost mantissa bit, which integers cannot.
Tier C (FINISH_*): unetpp_wgrad_finish on integer slabs made on the host, n_split in FINISH_SPLITS.

Every case: dw and db live inside larger buffers with sentinels on both sides and start as NaN; the call is repeated
with dw=None and with db=None; channels outside a sliced view and dy pixels outside every phase are NaN; the plan's
kernel, the kernel that ran and the row's label agree, and the plan's n_split is the split the row asks for.

Reachability (csrc/wgrad.hip wgrad_select, precedence first layer, bf16, pointwise, Winograd, LDS-DMA, fast, generic):
every label of the family is reachable through ops.wgrad and appears in TIER_A.  The two that no earlier test ran:
  wgrad_fast_kernel<1>  taps 1 with a folded x view: wgrad_pw_applies and wgrad_dma_applies want plain views
                        (pw_plain / plain_aligned refuse a scale), wgrad_fast_applies allows the affine on x;
  wgrad_kernel<1>       taps 1 with a ReLU gate on dy or a channel count that is no multiple of 4: every *_applies
                        above refuses a gate (and plain_aligned / aligned_view the alignment).

Loops of the kernels the splits and shapes are aimed at.  wgrad_dma / wgrad_wino walk their tiles two per iteration
(buffer A, buffer B): a workgroup with 1, 2, 3 and more tiles, odd and even, comes from n_split 32, 11 / 31, 5, 3, 2, 1
on the 32 patches of (2, 25, 97); wgrad_fast / wgrad_bf16 (prefetch distance two) take the same counts.  wgrad_bf16.hip
has no shape-dependent loop constant besides the tile width (LOG2TW 3 / 4 / 5: W 5 / 8, 12 / 16, >= 17) and that tile
count; wgrad_pw.hip keeps kDepth = 3 steps of four pixels in flight per wave and gives each of its 8 waves
rows * part / parts image rows: the PW_STEPS rows give waves with 0 / 1, 1 / 2, 2 / 3, 3 / 4 and 4 / 5 steps, and its
workgroup renumbering switches on when the grid is a multiple of 8 (pw-remap rows).
"""
import ctypes
import zlib

import pytest
import torch

from tests import wgrad_oracle as wo
from tests.wgrad_oracle import case

pytestmark = pytest.mark.gpu

S25 = (2, 25, 97)   # 4 x 4 patches per image, 2 x 2 of them interior at both limits of the test, ragged row and column
S24 = (2, 24, 96)   # exact multiples of the patch, one interior patch per image
S40 = (5, 40, 96)   # 75 patches
ALL25 = (1, 2, 3, 5, 11, 31, 32)
CORE25 = (1, 3, 31, 32)
BIG40 = (64, 65, 75)

WINO, DMA9, DMA1 = "wgrad_wino_kernel", "wgrad_dma_kernel<9>", "wgrad_dma_kernel<1>"
FAST9, FAST1, GEN9, GEN1 = "wgrad_fast_kernel<9>", "wgrad_fast_kernel<1>", "wgrad_kernel<9>", "wgrad_kernel<1>"
PW, FIRST = "wgrad_pw_kernel", "small_cin_wgrad_kernel"
PAIR9, PAIR1 = "wgrad_bf16_kernel<9>", "wgrad_bf16_kernel<1>"
QUAD9, QUAD1 = "wgrad_bf16_quad_kernel<9>", "wgrad_bf16_quad_kernel<1>"

# every tile width a kernel is instantiated for, images smaller than a patch, one pixel row, ragged second patches
SMALL_GEOMS = [(3, 33, 5), (2, 40, 8), (2, 17, 12), (1, 33, 16), (1, 17, 33), (2, 9, 40), (1, 1, 20), (1, 3, 4)]


def _ends(shape):
    m = wo.pixel_tiles(*shape)
    return (1, m) if m > 1 else (1,)


def _geometry_rows():
    rows = []
    for shape in SMALL_GEOMS:
        tag = "%dx%dx%d" % shape
        sp = _ends(shape)
        wide = shape[2] > 16
        rows += [
            case("geo-first-c3-" + tag, FIRST, shape, [3], 8, sp),
            case("geo-dma9-" + tag, DMA9, shape, [8], 8, sp, direct=True),
            case("geo-fast9-" + tag, FAST9, shape, [8], 8, sp, fold=True, direct=True),
            case("geo-gen9-" + tag, GEN9, shape, [8], 8, sp, gate=True),
            case("geo-pair9-" + tag, PAIR9, shape, [8], 8, sp, bf16=True),
            case("geo-quad9-" + tag, QUAD9, shape, [64], 64, sp, bf16=True),
            case("geo-dma1-" + tag, DMA1, shape, [8], 8, sp, taps=1),
            case("geo-fast1-" + tag, FAST1, shape, [8], 8, sp, taps=1, fold=True),
            case("geo-gen1-" + tag, GEN1, shape, [8], 8, sp, taps=1, gate=True),
            case("geo-pair1-" + tag, PAIR1, shape, [8], 8, sp, taps=1, bf16=True),
            case("geo-quad1-" + tag, QUAD1, shape, [64], 64, sp, taps=1, bf16=True),
        ]
        if wide:   # the Winograd kernel takes 32-wide patches only; narrower images go to the direct sum undirected
            rows += [case("geo-wino-" + tag, WINO, shape, [8], 8, sp),
                     case("geo-wino-fold-" + tag, WINO, shape, [8], 8, sp, fold=True)]
        else:
            rows.append(case("geo-dma9-undirected-" + tag, DMA9, shape, [8], 8, sp))
    return rows


PW_STEPS = [(1, 6, 4), (1, 12, 4), (1, 20, 4), (1, 28, 4), (1, 36, 4)]   # rows / 8 waves -> steps per wave, W / 4 = 1

TIER_A = _geometry_rows() + [
    # ---- first layer: C = 1..4, fp32 and bf16 dy (steered by SMALL_WGRAD_BLOCKS)
    case("first-c1-f32", FIRST, S25, [1], 8, CORE25),
    case("first-c2-f32", FIRST, S25, [2], 4, (1, 5, 32)),
    case("first-c3-f32", FIRST, S24, [3], 32, (1, 4, 18)),
    case("first-c4-f32", FIRST, S25, [4], 64, (2, 11, 32)),
    case("first-c3-f32-dyslice", FIRST, S25, [3], (20, 4, 8), (3, 32)),
    case("first-c1-f32-big", FIRST, S40, [1], 16, BIG40),
    case("first-c1-bf16", FIRST, S25, [1], 8, CORE25, bf16=True),
    case("first-c2-bf16", FIRST, S24, [2], 16, (1, 18), bf16=True),
    case("first-c3-bf16-dyslice", FIRST, S25, [3], (24, 8, 16), (3, 31), bf16=True),
    case("first-c4-bf16", FIRST, S40, [4], 32, BIG40, bf16=True),
    # ---- Winograd, plain and folded
    case("wino-8-8", WINO, S25, [8], 8, ALL25),
    case("wino-fold-8-8", WINO, S25, [8], 8, ALL25, fold=True),
    case("wino-cat-36", WINO, S25, [32, 8, 12], 36, (1, 3, 32)),
    case("wino-fold-cat-36", WINO, S25, [32, 8, 12], 36, (2, 31), fold=True),
    case("wino-40-64", WINO, S25, [40], 64, (1, 31)),
    case("wino-12-4", WINO, S25, [12], 4, (2, 11)),
    case("wino-slices", WINO, S25, [(20, 4, 8)], (20, 4, 8), (1, 5, 32)),
    case("wino-fold-slice", WINO, S25, [(20, 4, 8)], 8, (3, 32), fold=True),
    case("wino-s24", WINO, S24, [8], 8, (1, 4, 18)),
    case("wino-fold-s24", WINO, S24, [8], 8, (1, 5, 18), fold=True),
    case("wino-s40", WINO, S40, [8], 8, BIG40),
    case("wino-fold-s40", WINO, S40, [12], 8, BIG40, fold=True),
    # ---- LDS-DMA direct sum
    case("dma9-8-8", DMA9, S25, [8], 8, ALL25, direct=True),
    case("dma9-cat-36", DMA9, S25, [32, 8, 12], 36, (1, 3, 32), direct=True),
    case("dma9-40-64", DMA9, S25, [40], 64, (1, 31), direct=True),
    case("dma9-slices", DMA9, S25, [(20, 4, 8)], (20, 4, 8), (1, 5, 32), direct=True),
    case("dma9-narrow-x", DMA9, S25, [4, 8], 4, (3, 11)),   # an x view below 8 channels: not the Winograd kernel
    case("dma9-s24", DMA9, S24, [8], 8, (1, 4, 18), direct=True),
    case("dma9-s40", DMA9, S40, [8], 8, BIG40, direct=True),
    case("dma1-conv-12-36", DMA1, S25, [12], 36, CORE25, taps=1),
    case("dma1-deconv-64-16", DMA1, S25, [64], 16, CORE25, taps=1, deconv=True),
    case("dma1-deconv-pad", DMA1, S25, [8], (12, 4, 4), (1, 2, 32), taps=1, deconv=True, dy_pad=1),
    case("dma1-s40", DMA1, S40, [8], 4, BIG40, taps=1, deconv=True),
    # ---- register-staged fast kernel (a folded x view that is not the Winograd kernel's)
    case("fast9-8-8", FAST9, S25, [8], 8, ALL25, fold=True, direct=True),
    case("fast9-cat-36", FAST9, S25, [32, 8, 12], 36, (1, 3, 32), fold=True, direct=True),
    case("fast9-mixed", FAST9, S25, [8, 8], 8, (2, 5, 31), fold=(True, False)),   # folded and plain x views together
    case("fast9-slices", FAST9, S25, [(20, 4, 8)], (20, 4, 8), (1, 32), fold=True, direct=True),
    case("fast9-s24", FAST9, S24, [8], 8, (1, 4, 18), fold=True, direct=True),
    case("fast9-s40", FAST9, S40, [8], 8, BIG40, fold=True, direct=True),
    case("fast1-conv-40-8", FAST1, S25, [40], 8, CORE25, taps=1, fold=True),
    case("fast1-deconv-8-4", FAST1, S25, [8], 4, (1, 5, 32), taps=1, deconv=True, fold=True),
    # ---- generic kernel (ReLU gate on dy, or channel counts that are no multiple of 4)
    case("gen9-gate-8-8", GEN9, S25, [8], 8, ALL25, gate=True),
    case("gen9-cat-40-5", GEN9, S25, [40, 5], 36, CORE25),
    case("gen9-c30", GEN9, S25, [30], 8, (1, 32)),
    case("gen9-gate-slice", GEN9, S25, [12], (20, 4, 8), (3, 11), gate=True),
    case("gen9-s24", GEN9, S24, [8], 8, (1, 4, 18), gate=True),
    case("gen9-s40", GEN9, S40, [8], 8, BIG40, gate=True),
    case("gen1-conv-gate", GEN1, S25, [12], 8, CORE25, taps=1, gate=True),
    case("gen1-deconv-6-5", GEN1, S25, [6], 5, (1, 2, 32), taps=1, deconv=True),
    case("gen1-conv-cat-40-5", GEN1, S24, [40, 5], 33, (1, 18), taps=1),
    # ---- pointwise kernel at its block shape K = 64, N = 4 x 32
    case("pw-w4", PW, (2, 37, 4), [64], 32, (1, 3, 4), taps=1, deconv=True),
    case("pw-w20", PW, (1, 6, 20), [64], 32, (1,), taps=1, deconv=True),
    case("pw-w32", PW, (2, 16, 32), [64], 32, (1, 3, 4), taps=1, deconv=True),
    case("pw-remap-1block", PW, (4, 16, 32), [64], 32, (5, 8), taps=1, deconv=True),
    case("pw-remap-4blocks", PW, (1, 16, 32), [128], 64, (1, 2), taps=1, deconv=True),
    case("pw-slices", PW, (2, 9, 40), [(72, 8, 64)], (40, 8, 32), (1, 3, 8), taps=1, deconv=True),
    case("pw-conv-cat", PW, (2, 8, 16), [32, 32], 128, (1, 2), taps=1),
] + [case("pw-steps-%d" % s[1], PW, s, [64], 32, (1,), taps=1, deconv=True) for s in PW_STEPS] + [
    # ---- bf16 storage: pair and quad kernels
    case("pair9-8-8", PAIR9, S25, [8], 8, ALL25, bf16=True),
    case("pair9-cat-40", PAIR9, S25, [32, 8, 40], 40, (1, 3, 32), bf16=True),
    case("pair9-96-64", PAIR9, S25, [96, 64], 64, (1, 32), bf16=True),
    case("pair9-fold", PAIR9, S25, [8], 8, CORE25, bf16=True, fold=True),
    case("pair9-slices", PAIR9, S25, [(24, 8, 8)], (24, 8, 8), (1, 31), bf16=True),
    case("pair9-s24", PAIR9, S24, [8], 8, (1, 4, 18), bf16=True),
    case("pair9-s40", PAIR9, S40, [8], 8, BIG40, bf16=True),
    case("pair1-deconv-32-8", PAIR1, S25, [32], 8, CORE25, taps=1, deconv=True, bf16=True),
    case("pair1-conv-40-8", PAIR1, S24, [40], 8, (1, 5, 18), taps=1, bf16=True),
    case("quad9-64-64", QUAD9, S25, [64], 64, ALL25, bf16=True),
    case("quad9-128-64", QUAD9, S25, [128, 64], 64, (1, 32), bf16=True),
    case("quad9-fold", QUAD9, S25, [64], 64, (3, 31), bf16=True, fold=True),
    case("quad9-s24", QUAD9, S24, [64], 64, (1, 4, 18), bf16=True),
    case("quad9-s40", QUAD9, S40, [64], 64, BIG40, bf16=True),
    case("quad1-deconv-128-64", QUAD1, S25, [128], 64, (1, 3, 32), taps=1, deconv=True, bf16=True),
    case("quad1-deconv-small", QUAD1, (1, 12, 16), [128], 64, (1,), taps=1, deconv=True, bf16=True),
    # ---- wide layers: the transposing finish (direct sums) and the Winograd finish at the same width
    case("wide-256-256", DMA9, (1, 8, 8), [256], 256, (1,)),
    case("wide-320-224-direct", DMA9, (1, 16, 24), [128, 192], 224, (1, 2), direct=True),
    case("wide-320-224-wino", WINO, (1, 16, 24), [128, 192], 224, (1, 2)),
]

COVERAGE = (["%s C=%d %s" % (FIRST, c, t) for c in (1, 2, 3, 4) for t in ("fp32", "bf16")] +
            [WINO + " plain", WINO + " folded", DMA9, DMA1, FAST9, FAST1, GEN9, GEN1, PW, PAIR9, PAIR1, QUAD9, QUAD1])

# Tier B: (2, 25, 97) and (1, 12, 16), 8 -> 8 channels (the block shapes of the quad and pointwise kernels where those
# need more), at n_split 1 and max_split
B25, B12 = (2, 25, 97), (1, 12, 16)


def _tier_b_rows():
    rows = []
    for shape in (B25, B12):
        tag = "%dx%dx%d" % shape
        sp = _ends(shape)
        rows += [
            case("imp-first-c3-" + tag, FIRST, shape, [3], 8, sp),
            case("imp-first-c2-bf16-" + tag, FIRST, shape, [2], 8, sp, bf16=True),
            case("imp-dma9-" + tag, DMA9, shape, [8], 8, sp, direct=True),
            case("imp-fast9-" + tag, FAST9, shape, [8], 8, sp, fold=True, direct=True),
            case("imp-gen9-" + tag, GEN9, shape, [8], 8, sp, gate=True),
            case("imp-pair9-" + tag, PAIR9, shape, [8], 8, sp, bf16=True),
            case("imp-pair9-fold-" + tag, PAIR9, shape, [8], 8, sp, bf16=True, fold=True),
            case("imp-quad9-" + tag, QUAD9, shape, [64], 64, sp, bf16=True),
            case("imp-dma1-" + tag, DMA1, shape, [8], 8, sp, taps=1),
            case("imp-fast1-" + tag, FAST1, shape, [8], 8, sp, taps=1, fold=True),
            case("imp-gen1-" + tag, GEN1, shape, [8], 8, sp, taps=1, gate=True),
            case("imp-pair1-" + tag, PAIR1, shape, [8], 8, sp, taps=1, bf16=True),
            case("imp-quad1-" + tag, QUAD1, shape, [64], 64, sp, taps=1, bf16=True),
        ]
    rows += [case("imp-pw-1x12x16", PW, B12, [64], 128, (1,), taps=1),
             case("imp-pw-2x25x96", PW, (2, 25, 96), [64], 128, (1, 24), taps=1),
             case("imp-wino-2x25x97", WINO, B25, [8], 8, _ends(B25)),
             case("imp-wino-fold-2x25x97", WINO, B25, [8], 8, _ends(B25), fold=True)]
    return rows


TIER_B = _tier_b_rows()
# (1, 12, 16) is 16 wide: wgrad_wino_applies wants 32-wide patches (W >= 17), so the issue's second Winograd shape runs
# the direct sum (imp-dma9-1x12x16 above, undirected below) and the Winograd bound is exercised on (2, 25, 97)
TIER_B.append(case("imp-dma9-undirected-1x12x16", DMA9, B12, [8], 8, (1,)))

# Roundings between an x value and a dW element of the Winograd path when dy is a single 1.0 per column
# (csrc/wgrad_wino.hip):  2  the column pass and the row pass of B^T d B (one add / sub each; compute(), column_pass and
#                            pk_sub_add_x / pk_cross_sub);
#                         0  A dY A^T of a single 1.0 is +-1 or 0, the MFMA product by it and the accumulation onto
#                            zeros (other tiles, waves, slabs) are exact;
#                         4  the fmaf chain over bb of the finish (rowsum), 4 the fmaf chain over aa (out).
WINO_ROUNDINGS = 2 + 4 + 4

PAD = 64           # sentinel floats on both sides of dw and db
SENTINEL = -777.25
SEEN = {}          # coverage key -> set of splits that ran and passed


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_REF = {}


def _reference(c, ops, key):
    """the oracle's (dw, db) of a case, computed once"""
    if key not in _REF:
        _REF[key] = wo.reference(c, ops)
    return _REF[key]


def _device_views(c, ops, dev):
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    act = torch.bfloat16 if c.bf16 else torch.float32
    xdt = torch.float32 if c.first_layer else act   # the 1..4-channel network input stays fp32
    cache = {}

    def put(t, dt):
        k = (id(t), dt)
        if k not in cache:
            cache[k] = t.to(dt).to(dev).contiguous()
        return cache[k]

    def conv(v, dt):
        f = (lambda t: None if t is None else t.float().to(dev))
        return V(put(v.t, dt), v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, scale=f(v.scale), shift=f(v.shift),
                 gate=None if v.gate is None else put(v.gate, dt), relu=v.relu)
    return [conv(v, xdt) for v in ops.xs], [conv(v, act) for v in ops.dys]


def _guarded(numel, dev):
    buf = torch.full((numel + 2 * PAD,), SENTINEL, device=dev)
    out = buf[PAD:PAD + numel]
    out.fill_(float("nan"))
    return buf, out


def _intact(buf, numel):
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + numel:] == SENTINEL).all())


def _mismatch(got, want):
    bad = (got != want).nonzero().flatten()
    i = int(bad[0])
    return "%d of %d elements differ, first at %d: got %r want %r" % (bad.numel(), want.numel(), i, float(got[i]), float(want[i]))


def _launch(c, xv, dv, n_split, dw, db):
    """ops.wgrad with the split steered as the row asks; returns the plan"""
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    n, h, w = c.shape
    k_tiles = sum((v[2] + 31) // 32 for v in c.xs)
    n_tiles = ((c.dy[2] + 31) // 32) * (4 if c.deconv else 1)
    ppw = 4 if c.label in (QUAD9, QUAD1) else 8 if c.label == PW else 1
    assert (k_tiles * n_tiles) % ppw == 0
    target = n_split * k_tiles * n_tiles // ppw
    if c.bf16 and ppw == 1 and target == 256:
        target += 1   # (exactly 256 is the plan's "default" that the pair kernel doubles; 257 // workgroups is the same split)
    args = (n, h, w, c.taps, xv, dv, dw, c.dw_strides, db)
    kw = dict(n_inner=c.n_inner, direct=c.direct)
    if c.first_layer:
        with _lib.debug_switch("SMALL_WGRAD_BLOCKS", n_split * k_tiles * n_tiles):
            return ops.wgrad(*args, **kw)
    return ops.wgrad(*args, target_blocks=target, **kw)


def _check_plan(c, plan, n_split):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    ran = _lib.lib().unetpp_last_kernel_name().decode()
    assert plan.kernel.decode() == ran == c.label, (c.id, plan.kernel.decode(), ran, c.label)
    assert plan.n_split == n_split, (c.id, plan.n_split, n_split)
    assert plan.planes == (16 if c.wino else c.taps)


def _run(c, ops, dev, n_split, want, with_partial_calls, compare):
    """One launch into guarded NaN destinations (+ the dw=None and db=None calls), compared by `compare(got_dw, got_db)`"""
    xv, dv = _device_views(c, ops, dev)
    want_dw, want_db = want
    dw_buf, dw = _guarded(want_dw.numel(), dev)
    db_buf, db = _guarded(want_db.numel(), dev)
    _check_plan(c, _launch(c, xv, dv, n_split, dw, db), n_split)
    torch.cuda.synchronize()
    assert _intact(dw_buf, dw.numel()) and _intact(db_buf, db.numel()), "%s split %d: a sentinel was overwritten" % (c.id, n_split)
    got_dw, got_db = dw.cpu().double(), db.cpu().double()
    assert not bool(torch.isnan(got_dw).any()), "%s split %d: dw elements left unwritten" % (c.id, n_split)
    assert not bool(torch.isnan(got_db).any()), "%s split %d: db elements left unwritten" % (c.id, n_split)
    compare(got_dw, got_db)
    if with_partial_calls:
        db2_buf, db2 = _guarded(want_db.numel(), dev)
        _check_plan(c, _launch(c, xv, dv, n_split, None, db2), n_split)
        dw3_buf, dw3 = _guarded(want_dw.numel(), dev)
        _check_plan(c, _launch(c, xv, dv, n_split, dw3, None), n_split)
        torch.cuda.synchronize()
        assert _intact(db2_buf, db2.numel()) and _intact(dw3_buf, dw3.numel())
        assert _intact(dw_buf, dw.numel()) and _intact(db_buf, db.numel())
        assert torch.equal(dw.cpu().double(), got_dw) and torch.equal(db.cpu().double(), got_db), "an output of the full call changed"
        assert torch.equal(db2.cpu().double(), got_db), "%s split %d: db differs with dw=None" % (c.id, n_split)
        assert torch.equal(dw3.cpu().double(), got_dw), "%s split %d: dw differs with db=None" % (c.id, n_split)


@pytest.mark.parametrize("c", TIER_A, ids=[c.id for c in TIER_A])
def test_integer_operands_every_element_equal(dev, c):
    ops = wo.integer_operands(c)
    want = _reference(c, ops, ("A", c.id))

    for i, n_split in enumerate(c.splits):
        def compare(got_dw, got_db):
            assert torch.equal(got_dw, want[0]), "%s split %d dw: %s" % (c.id, n_split, _mismatch(got_dw, want[0]))
            assert torch.equal(got_db, want[1]), "%s split %d db: %s" % (c.id, n_split, _mismatch(got_db, want[1]))
        _run(c, ops, dev, n_split, want, i == 0, compare)
        SEEN.setdefault(c.cover, set()).add(n_split)


def wino_impulse_bound(c, ops):
    """gamma(WINO_ROUNDINGS) * M per element of dw: M = the window's absolute values through |B^T| . |B| (the planes) and
    |G^T| . |G| (the finish), in the destination layout"""
    from tests.helpers import gamma
    n, h, w = c.shape
    m = wo.wino_finish(wo.wino_planes(wo.concat(ops.xs, h, w).abs(), wo.concat(ops.dys, h, w).abs(), absolute=True), absolute=True)
    return gamma(WINO_ROUNDINGS) * wo.scatter_dw(m, c.dw_strides, c.n_inner)


@pytest.mark.parametrize("c", TIER_B, ids=[c.id for c in TIER_B])
def test_impulses_copy_the_window(dev, c):
    from tests.helpers import bound_ratio, report_ratio
    for chunk in range(wo.impulse_chunks(c)):
        ops, pairs = wo.impulse_operands(c, chunk)
        want = _reference(c, ops, ("B", c.id, chunk))
        assert all(float(want[1][col]) == (0.0 if (c.gate and j == 0) else 1.0) for j, (_, col) in enumerate(pairs))
        assert float(want[1].sum()) == len(pairs) - (1 if c.gate else 0)
        bound = wino_impulse_bound(c, ops) if c.wino else None
        for i, n_split in enumerate(c.splits):
            def compare(got_dw, got_db):
                assert torch.equal(got_db, want[1]), "%s split %d db: %s" % (c.id, n_split, _mismatch(got_db, want[1]))
                if not c.wino:
                    assert torch.equal(got_dw, want[0]), "%s split %d dw: %s" % (c.id, n_split, _mismatch(got_dw, want[0]))
                    return
                ratio = bound_ratio(got_dw, want[0], bound)
                report_ratio("%s chunk %d split %d" % (c.id, chunk, n_split), "dw", ratio, {"roundings": WINO_ROUNDINGS})
                assert ratio <= 1.0, (c.id, n_split, ratio)
                untouched = bound == 0   # columns without an impulse (and taps whose window lies outside): exact zeros
                assert bool((got_dw[untouched] == 0).all())
            _run(c, ops, dev, n_split, want, i == 0 and chunk == 0, compare)


def test_every_label_ran(dev):
    """Runs after the tier A cases of this module: every kernel label of the family (first layer: every channel count
    with fp32 and with bf16 dy; Winograd: plain and folded) passed, each tile-walking kernel at splits 1, 3, 31 and 32
    of the 32 patches of (2, 25, 97)."""
    missing = [k for k in COVERAGE if k not in SEEN]
    assert not missing, missing
    for k in (WINO + " plain", WINO + " folded", DMA9, FAST9, GEN9, PAIR9, QUAD9):
        assert {1, 3, 31, 32} <= SEEN[k], (k, sorted(SEEN[k]))
    print("coverage:", {k: sorted(v) for k, v in SEEN.items()})


# ------------------------------------------------------------------------------------------------ tier C: finish
FINISH_SPLITS = (1, 2, 3, 4, 5, 15, 16, 17, 32, 33, 63, 64, 65, 130)

# (id, taps, K, Ncols, n_inner, layout): "conv" = dense torch layout dw[n][k][t]; "deconv" = dw[k][c][o], column o * n_inner + c
FINISH_GENERIC = [
    ("conv9-12-20", 9, 12, 20, 20, "conv"), ("conv1-12-20", 1, 12, 20, 20, "conv"),
    ("conv9-40-36", 9, 40, 36, 36, "conv"), ("conv1-40-36", 1, 40, 36, 36, "conv"),
    ("deconv4-12-5", 1, 12, 20, 5, "deconv"), ("deconv4-12-16", 1, 12, 64, 16, "deconv"),
    ("deconv4-40-17", 1, 40, 68, 17, "deconv"), ("deconv4-40-36", 1, 40, 144, 36, "deconv"),
    ("deconv2-12-10", 1, 12, 20, 10, "deconv"), ("deconv2-40-18", 1, 40, 36, 18, "deconv"),
]
FINISH_TR = [   # (id, taps, K, Ncols, splits): K * Ncols >= 65536, dense layout; 33 slabs fall back to the generic kernel
    ("tr9-256-256", 9, 256, 256, (1, 2, 3, 4, 5, 15, 16, 17, 32, 33)),
    ("tr1-256-256", 1, 256, 256, (1, 2, 3, 4, 5, 15, 16, 17, 32, 33)),
    ("tr9-264-256", 9, 264, 256, (1, 3, 4, 32, 33)),
]
FINISH_WINO = [("wino-8-4", 8, 4), ("wino-12-36", 12, 36), ("wino-32-65", 32, 65)]


def _finish(slabs, n_split, taps, k, nc, n_inner, dw, strides, db):
    from unet_nested4tiny_objects_keypoints_amd import _lib

    def p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.lib().unetpp_wgrad_finish(p(slabs), n_split, taps, k, nc, n_inner, p(dw), strides[0], strides[1], strides[2],
                                          strides[3], p(db), st)


def _integer_slabs(seed, n_split, floats, step=1):
    """[n_split, floats] int64 in [-40, 40] * step, every slab its own values"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-40, 41, (n_split, floats), generator=g) * step


def _finish_case(dev, slabs_i, splits, taps, k, nc, n_inner, strides, expect):
    """unetpp_wgrad_finish on the first n slabs for every n of splits; expect(summed [floats] float64) -> (dw flat, db)"""
    slabs = slabs_i.float().to(dev)
    cum = torch.cumsum(slabs_i, 0)
    for n_split in splits:
        want_dw, want_db = expect(cum[n_split - 1].double())
        dw_buf, dw = _guarded(want_dw.numel(), dev)
        db_buf, db = _guarded(want_db.numel(), dev)
        assert _finish(slabs, n_split, taps, k, nc, n_inner, dw, strides, db) == 0
        dw2_buf, dw2 = _guarded(want_dw.numel(), dev)
        assert _finish(slabs, n_split, taps, k, nc, n_inner, dw2, strides, None) == 0
        db3_buf, db3 = _guarded(want_db.numel(), dev)
        assert _finish(slabs, n_split, taps, k, nc, n_inner, None, strides, db3) == 0
        torch.cuda.synchronize()
        for buf, t in ((dw_buf, dw), (db_buf, db), (dw2_buf, dw2), (db3_buf, db3)):
            assert _intact(buf, t.numel()), "n_split %d: a sentinel was overwritten" % n_split
        for got, want, what in ((dw, want_dw, "dw"), (dw2, want_dw, "dw (db=None)"), (db, want_db, "db"), (db3, want_db, "db (dw=None)")):
            g = got.cpu().double()
            assert torch.equal(g, want), "n_split %d %s: %s" % (n_split, what, _mismatch(g, want))


def _generic_expect(taps, k, nc, n_inner, strides):
    def expect(total):
        rows = total.view(taps * k + 1, nc)
        dw = wo.scatter_dw(rows[:-1].reshape(taps, k, nc), strides, n_inner)
        return dw, rows[-1].view(nc // n_inner, n_inner).sum(0)
    return expect


def _layout_strides(layout, taps, k, nc, n_inner):
    if layout == "conv":
        return (1, taps, k * taps, 0)
    n_outer = nc // n_inner
    return (0, n_inner * n_outer, n_outer, 1)


@pytest.mark.parametrize("row", FINISH_GENERIC, ids=[r[0] for r in FINISH_GENERIC])
def test_finish_generic_on_integer_slabs(dev, row):
    """wgrad_finish_kernel: the 4 x SG unrolled slab loop and its remainder, 1..16 slab groups, dense and deconvolution
    destinations, and the extra bias blocks that sum the pixel phases (16 channels per block: n_inner 5, 16, 17, 36)."""
    name, taps, k, nc, n_inner, layout = row
    strides = _layout_strides(layout, taps, k, nc, n_inner)
    slabs = _integer_slabs(zlib.crc32(name.encode()), max(FINISH_SPLITS), (taps * k + 1) * nc)
    _finish_case(dev, slabs, FINISH_SPLITS, taps, k, nc, n_inner, strides, _generic_expect(taps, k, nc, n_inner, strides))


@pytest.mark.parametrize("row", FINISH_TR, ids=[r[0] for r in FINISH_TR])
def test_finish_transposing_on_integer_slabs(dev, row):
    """wgrad_finish_tr_kernel (K * Ncols >= 65536, dense layout, at most 32 slabs), and the same values from the generic
    kernel that 33 slabs fall back to"""
    name, taps, k, nc, splits = row
    strides = _layout_strides("conv", taps, k, nc, nc)
    slabs = _integer_slabs(zlib.crc32(name.encode()), max(splits), (taps * k + 1) * nc)
    _finish_case(dev, slabs, splits, taps, k, nc, nc, strides, _generic_expect(taps, k, nc, nc, strides))


@pytest.mark.parametrize("row", FINISH_WINO, ids=[r[0] for r in FINISH_WINO])
def test_finish_winograd_on_integer_slabs(dev, row):
    """wgrad_finish_wino_kernel: slabs [K][Ncols][16 planes] + bias row in multiples of 4, so that G^T U G (multiples of
    1/4 of them) is an integer; expected from the oracle's float64 G^T U G with the unsigned-last-row signs"""
    name, k, nc = row
    strides = (1, 9, 9 * k, 0)
    slabs = _integer_slabs(zlib.crc32(name.encode()), max(FINISH_SPLITS), (16 * k + 1) * nc, step=4)

    def expect(total):
        u = total[:16 * k * nc].view(k, nc, 16).permute(2, 0, 1).contiguous()
        return wo.scatter_dw(wo.wino_finish(u), strides, nc), total[16 * k * nc:]
    _finish_case(dev, slabs, FINISH_SPLITS, 16, k, nc, nc, strides, expect)


def test_finish_refuses_bad_arguments(dev):
    slabs = torch.zeros(4 * (9 * 8 + 1) * 8, device=dev)
    dw, db = torch.zeros(9 * 8 * 8, device=dev), torch.zeros(8, device=dev)
    s9 = (1, 9, 72, 0)
    assert _finish(slabs, 2, 9, 8, 8, 8, dw, s9, db) == 0
    for args in [(None, 2, 9, 8, 8, 8), (slabs, 0, 9, 8, 8, 8), (slabs, 2, 0, 8, 8, 8), (slabs, 2, 9, 0, 8, 8),
                 (slabs, 2, 9, 8, 0, 8), (slabs, 2, 9, 8, 8, 0), (slabs, 2, 9, 8, 8, 3),   # Ncols % n_inner != 0
                 (slabs, 1, 16, 4, 8, 4),                                                   # Winograd slabs with pixel phases
                 (slabs, 2, 1, 8, 40, 8)]:                                                  # more than 4 phases per channel
        assert _finish(args[0], *args[1:], dw, s9, db) == -1, args[1:]
    torch.cuda.synchronize()
