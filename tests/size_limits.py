"""Shared by tests/test_size_limits_host.py and tests/test_gpu_size_limits.py (no tests in here): the cells that put the
layer kernels on both sides of their 32-bit size limits, integer data generated on the device, the crops that go to
the host, and output buffers between sentinels.

Why integers: with |x|, |w| <= 2 (`t.random_(-2, 3)`, the value range of gemm_oracle._ints) and K <= 9 * 128 every
product and every fp32 partial sum of every kernel is an exact integer (|sum| <= 4608), through the Winograd transforms
as well while helpers.wino_magnitude stays below 2^22 (WINO_MAGNITUDE_LIMIT; tests/test_size_limits_host.py asserts it
for the operand ranges used here, as tests/test_gemm_oracle_host.py does for the existing exact rows).  So two launches
that cut the same tensor into different units must agree BITWISE, and a crop must EQUAL its float64 sum.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

PAD = 64                 # sentinel elements on both sides of an output (tests/test_gpu_gemm_bf16_exact.py)
SENTINEL = -776.0        # a bf16 number
CROP_H, CROP_W = 40, 48  # pixels of a crop, all channels
MAX_CROPS = 8
WINO_MAGNITUDE_LIMIT = 2.0 ** 22
X_ABS, W_ABS = 2, 2      # |values| of fill_ints and of the weights
FOLD_ABS = 6             # |relu(x * scale + shift)| with integer |scale|, |shift| <= 2
PEAK_BYTES = 32 * 2 ** 30

WINO, FAST9, PW32 = "gemm_wino_kernel", "gemm_fast_kernel<9>", "gemm_pw_kernel"
PIX9, PIX1 = "gemm_pix_kernel<9>", "gemm_pix_kernel<1>"
DMA9, REG9, PWB = "gemm_bf16_dma_kernel<9>", "gemm_bf16_kernel<9>", "gemm_pw_bf16_kernel"
REFUSED = "EINVAL"


# ------------------------------------------------------------------------------------------------ the cell table
@dataclass(frozen=True)
class GemmCell:
    """One big launch.  big: which side holds the big tensor (its C is 128; the other side's is `small`)."""
    id: str
    dtype: str                 # "f32" / "bf16"
    taps: int
    big: str                   # "in" / "out"
    n: int
    h: int
    w: int
    label: str                 # what must run; REFUSED: ops.gemm_fwd raises
    small: int = 8
    mode: str = "plain"        # plain / fold (BatchNorm fold + ReLU on load) / bias-relu / accgate (gated accumulate)
    direct: bool = False
    planned: Optional[str] = None   # unetpp_gemm_plan WITH a weight image where that differs from `label`
    no_lean_twin: bool = False      # also bitwise equal to the same launch under WINO_NO_LEAN=1
    peak_gib: float = 0.0           # device memory the GPU cell needs at its peak (stated in the test's docstring)

    @property
    def c_in(self):
        return 128 if self.big == "in" else self.small

    @property
    def c_out(self):
        return 128 if self.big == "out" else self.small

    @property
    def esize(self):
        return 4 if self.dtype == "f32" else 2

    @property
    def big_shape(self):
        return (self.n, self.h, self.w, 128)


S = 1024
# `planned` = REFUSED: the plan with a weight image refuses tensors of 2^31 elements (gemm_units.h fast_args), ops.gemm_fwd
# plans again without one: fp32 then runs the generic kernel, bf16 has none and raises.
GEMM_CELLS = [
    GemmCell("wino-lean-max", "f32", 9, "in", 1, 4095, S, WINO, no_lean_twin=True, peak_gib=3.0),
    GemmCell("wino-first-general", "f32", 9, "in", 4, S, S, WINO, no_lean_twin=True, peak_gib=3.0),
    # 2^31 + 2^29 bytes.  (A view of exactly 2^31 bytes, the cell above, would still be read correctly by a lean
    # instantiation: its offsets stay below the out-of-range mark 0x80000000.  From here on the mark lies INSIDE the
    # view, and a lean launch would read data where the zero padding belongs -- the first crop and the twin see it.)
    GemmCell("wino-general-mark-inside", "f32", 9, "in", 5, S, S, WINO, no_lean_twin=True, peak_gib=3.5),
    GemmCell("wino-over-4GiB/plain", "f32", 9, "in", 9, S, S, WINO, peak_gib=5.5),
    GemmCell("wino-over-4GiB/fold", "f32", 9, "in", 9, S, S, WINO, mode="fold", peak_gib=5.5),
    GemmCell("wino-out-over-4GiB/bias-relu", "f32", 9, "out", 9, S, S, WINO, mode="bias-relu", peak_gib=6.5),
    GemmCell("wino-out-over-4GiB/accgate", "f32", 9, "out", 9, S, S, WINO, mode="accgate", peak_gib=15.0),
    GemmCell("fast9-over-4GiB/in", "f32", 9, "in", 9, S, S, FAST9, direct=True, peak_gib=6.5),
    GemmCell("fast9-over-4GiB/out", "f32", 9, "out", 9, S, S, FAST9, direct=True, peak_gib=6.5),
    GemmCell("pw-over-4GiB", "f32", 1, "in", 9, S, S, PW32, small=32, peak_gib=6.5),
    GemmCell("pix9-2^31", "f32", 9, "in", 16, S, S, PIX9, planned=REFUSED, peak_gib=9.5),
    GemmCell("pix1-2^31", "f32", 1, "out", 16, S, S, PIX1, planned=REFUSED, peak_gib=10.0),
    GemmCell("dma-max", "bf16", 9, "in", 1, 8191, S, DMA9, peak_gib=3.0),
    GemmCell("dma-first-register", "bf16", 9, "in", 8, S, S, REG9, peak_gib=3.0),
    GemmCell("dma-out-3GiB", "bf16", 9, "out", 12, S, S, DMA9, small=32, peak_gib=5.0),
    GemmCell("bf16-near-2^31/taps9", "bf16", 9, "in", 1, 16383, S, REG9, peak_gib=5.0),
    GemmCell("bf16-near-2^31/taps1", "bf16", 1, "in", 1, 16383, S, PWB, small=32, peak_gib=6.0),
    GemmCell("bf16-2^31-refused", "bf16", 9, "in", 16, S, S, REFUSED, planned=REFUSED, peak_gib=5.0),
]

# The 2x2 stride-2 transposed convolution as a pointwise GEMM with four pixel-phase output views (engine.pack_deconv_fwd):
# 3 x 1024 x 1024 x 128 -> 3 x 2048 x 2048 x 96, an output of 4.5 GiB.  Its label from the launchers' rules: 1 tap, no
# Winograd; gemm_pw_kernel keeps the whole weight in LDS and refuses (K N + N) 4 = (128 * 384 + 384) * 4 = 198144 bytes
# > 148 KB (gemm_pw.hip gemm_pw_applies); the next kernel with a weight image is gemm_fast_kernel<1>.
DECONV_CELL = dict(id="deconv-over-4GiB", n=3, h=S, w=S, c_in=128, c_out=96, label="gemm_fast_kernel<1>", peak_gib=8.0)

# The issue's host table: input views V(128), output V(32), a weight image set; columns f32 3x3 / f32 3x3 direct /
# f32 1x1 / f32 3x3 without image / bf16 3x3 / bf16 1x1.
HOST_COLUMNS = [dict(taps=9), dict(taps=9, flags="direct"), dict(taps=1), dict(taps=9, image=False),
                dict(taps=9, flags="bf16"), dict(taps=1, flags="bf16")]
HOST_TABLE = [
    ((1, 4095, S), (WINO, FAST9, PW32, PIX9, DMA9, PWB)),
    ((4, S, S), (WINO, FAST9, PW32, PIX9, DMA9, PWB)),
    ((8, S, S), (WINO, FAST9, PW32, PIX9, REG9, PWB)),
    ((12, S, S), (WINO, FAST9, PW32, PIX9, REG9, PWB)),
    ((1, 16383, S), (WINO, FAST9, PW32, PIX9, REG9, PWB)),
    ((16, S, S), (REFUSED, REFUSED, REFUSED, PIX9, REFUSED, REFUSED)),
]


@dataclass(frozen=True)
class PoolCell:
    """affine_relu_pool with scale / shift / ReLU and act, pooled, pool_idx requested, then maxpool_bwd on its winners
    (fp32 NHWC, C = 128): both sides of stream_rows_form_ok (stream_select.h)."""
    id: str
    n: int
    h: int
    w: int
    fwd_label: str
    bwd_label: str
    c: int = 128
    dtype: str = "f32"
    peak_gib: float = 0.0


# The bf16 forms refuse octet items >= 2^31 (pointwise_bf16.hip), which needs a 32 GiB tensor: out of scope.  BF16_H x 1024
# x 128 is 2^31 + 2^19 elements, 2^32 + 2^20 bytes of bf16: four rows past the offset where a 32-bit byte offset and a signed
# 32-bit element offset wrap (1 x 16382 x 1024 x 128 would stop 2^19 bytes short of it).
BF16_H = 16386
POOL_CELLS = [
    PoolCell("pool-rows-max", 1, 16382, S, "affine_relu_pool_rows", "maxpool_bwd_rows", peak_gib=21.0),
    PoolCell("pool-general-2^31", 16, S, S, "affine_relu_pool<4>", "maxpool_bwd<4>", peak_gib=21.0),
    PoolCell("pool-bf16-over-4GiB", 1, BF16_H, S, "affine_relu_pool_bf16", "maxpool_bwd_bf16", dtype="bf16", peak_gib=11.0),
]


@dataclass(frozen=True)
class BilinearCell:
    """bilinear2x_fwd into an output of (n, 2h, 2w, 128), then bilinear2x_bwd (accumulating) from a gradient of that size"""
    id: str
    n: int
    h: int                     # of the input
    w: int
    fwd_label: str
    bwd_label: str
    c: int = 128
    dtype: str = "f32"
    peak_gib: float = 0.0


BILINEAR_CELLS = [
    BilinearCell("bilinear-out-2^31", 4, S, S, "bilinear2x_fwd", "bilinear2x_bwd", peak_gib=15.0),
    BilinearCell("bilinear-bf16-over-4GiB", 1, BF16_H // 2, 512, "bilinear2x_fwd_bf16", "bilinear2x_bwd_bf16", dtype="bf16", peak_gib=7.5),
]

@dataclass(frozen=True)
class BnCell:
    """ops.bn_backward (reduce, finalize, apply; dy in place, as the engine calls it) on C = 128, with and without the
    gradient of the max-pool routed through it, on both sides of stream_bn_pool_ok (stream_select.h): below 2^31 elements the
    pool-fused row kernels run, at 2^31 a maxpool_bwd pass and then the plain kernels.  label: the apply's, the last
    launch; adds: the form of tests/test_gpu_streaming.reduce_adds that counts the additions of a partial row."""
    id: str
    dtype: str
    n: int
    h: int
    w: int
    pool: bool
    label: str
    adds: str
    c: int = 128
    peak_gib: float = 0.0


BN_CELLS = [
    BnCell("bn-rows-max/pool", "f32", 1, 16382, S, True, "bn_bwd_apply_pool", "pool", peak_gib=28.5),
    BnCell("bn-rows-max/plain", "f32", 1, 16382, S, False, "bn_bwd_apply<4>", "vec", peak_gib=26.0),
    BnCell("bn-2^31/pool", "f32", 16, S, S, True, "bn_bwd_apply<4>", "vec", peak_gib=28.5),
    BnCell("bn-bf16-over-4GiB/pool", "bf16", 1, BF16_H, S, True, "bn_bwd_apply_bf16/pool", "bf16", peak_gib=15.0),
]


@dataclass(frozen=True)
class HeadCell:
    """head_fwd, head_bwd (and heads_mean_fwd over two heads where mean_label is set) on NHWC features of C = 32 with 4
    classes; p_drop = 0, or 0.4 with a given mask.  fp32 (head_select.h): the stream / pow2 forms need pixels * C <
    0x7fffffff, beyond it head_fwd_tiled / head_bwd_vec run with 64-bit offsets; bf16: the octet forms count pixels in 32
    bits and address elements in 64: 32 x 2048 x 2048 x 32 is 2^32 elements."""
    id: str
    dtype: str
    n: int
    h: int
    w: int
    fwd_label: str
    bwd_label: str
    mean_label: Optional[str] = None
    p_drop: float = 0.0
    accumulate: bool = False
    twin_same_form: bool = False   # an image's launch runs the big launch's form: the bitwise twin is asserted to run
    c: int = 32
    n_cls: int = 4
    peak_gib: float = 0.0


HEAD_CELLS = [
    HeadCell("head-f32-under-2^31", "f32", 1, 32766, 2048, "head_fwd_stream<3,4,0>", "head_bwd_pow2<3,0,4>",
             accumulate=True, peak_gib=28.5),
    HeadCell("head-f32-under-2^31/mask", "f32", 1, 32766, 2048, "head_fwd_stream<3,4,2>", "head_bwd_pow2<3,2,4>",
             p_drop=0.4, peak_gib=21.5),
    HeadCell("head-f32-2^31", "f32", 16, 2048, 2048, "head_fwd_tiled", "head_bwd_vec", accumulate=True, peak_gib=28.5),
    HeadCell("head-bf16-2^32", "bf16", 32, 2048, 2048, "head_fwd_bf16<2,0,4>", "head_bwd_bf16<2,0,4>",
             mean_label="heads_mean_bf16<2,4>", twin_same_form=True, peak_gib=22.5),
]

# nchw_to_nhwc and back at 16 x 128 x 1024 x 1024 (2^31 elements; three such tensors: 24.5 GiB at the peak)
LAYOUT_CELL = ("layout-2^31", (16, 128, S, S), "nchw_to_nhwc", "nhwc_to_nchw", 25.0)


def gemm_plan_args(cell: GemmCell):
    """arguments of tests/test_gemm_plan.desc for the cell's one big launch"""
    from tests.test_gemm_plan import V
    fold = cell.mode == "fold"
    acc = cell.mode == "accgate"
    return dict(n=cell.n, h=cell.h, w=cell.w, taps=cell.taps, ins=[V(cell.c_in, fold=fold)],
                outs=[V(cell.c_out, relu=cell.mode == "bias-relu", gate=acc, accumulate=acc)],
                flags=("bf16" if cell.dtype == "bf16" else "") + (" direct" if cell.direct else ""))


# ------------------------------------------------------------------------------------------------ device data
FILL_CHUNK = 2 ** 28


def fill_ints(t: torch.Tensor, seed: int) -> torch.Tensor:
    """Fills an allocated (contiguous) tensor in place with integers -2 .. 2 (a fifth of them zero), chunk by chunk:
    no int64 temporary, no host tensor, and the same values for the same seed, shape and type."""
    assert t.is_contiguous()
    g = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    for lo in range(0, flat.numel(), FILL_CHUNK):
        flat[lo:lo + FILL_CHUNK].random_(-X_ABS, X_ABS + 1, generator=g)
    return t


def int_weights(shape, seed: int, lo: int = -W_ABS, hi: int = W_ABS) -> torch.Tensor:
    """small host tensor of integers lo .. hi (float32)"""
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def guarded(shape, dtype, dev, fill_seed: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (flat buffer with PAD sentinels on both sides, the tensor inside it).  A plain output's interior starts as
    NaN, an accumulating one's (fill_seed) as integer data."""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.empty(numel + 2 * PAD, dtype=dtype, device=dev)
    buf[:PAD] = SENTINEL
    buf[PAD + numel:] = SENTINEL
    t = buf[PAD:PAD + numel].view(shape)
    if fill_seed is None:
        t.view(-1).fill_(float("nan"))
    else:
        fill_ints(t, fill_seed)
    return buf, t


def guards_intact(buf: torch.Tensor) -> bool:
    return bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all())


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor, chunk: int = 2 ** 28) -> bool:
    """bitwise equality of two tensors of one shape and type on the device (NaN == NaN), no temporary above 2 GiB"""
    assert a.shape == b.shape and a.dtype == b.dtype
    if not (a.is_contiguous() and b.is_contiguous()):
        return all(same_bits(a[i].contiguous(), b[i].contiguous(), chunk) for i in range(a.shape[0]))
    fa, fb = bits(a).view(-1), bits(b).view(-1)
    return all(torch.equal(fa[lo:lo + chunk], fb[lo:lo + chunk]) for lo in range(0, fa.numel(), chunk))


def any_nan(t: torch.Tensor, chunk: int = 2 ** 28) -> bool:
    flat = t.view(-1)
    return any(bool(torch.isnan(flat[lo:lo + chunk]).any()) for lo in range(0, flat.numel(), chunk))


# ------------------------------------------------------------------------------------------------ crops
def _window_at(shape, elem: int):
    """the window (n, y0, x0, rows, cols) around the pixel that holds element offset `elem`, clamped into its image"""
    n_img, h, w, c = shape
    p = elem // c
    n, r = divmod(p, h * w)
    y, x = divmod(r, w)
    ch, cw = min(CROP_H, h), min(CROP_W, w)
    return (n, min(max(y - ch // 2, 0), h - ch), min(max(x - cw // 2, 0), w - cw), ch, cw)


def window_span(shape, win):
    """(first, one past the last) element offset of a window"""
    _, h, w, c = shape
    n, y0, x0, ch, cw = win
    return ((n * h + y0) * w + x0) * c, ((n * h + y0 + ch - 1) * w + x0 + cw) * c


def choose_crops(shape, esize: int):
    """At most MAX_CROPS windows (n, y0, x0, rows <= 40, cols <= 48), all channels, of an NHWC tensor:
    image 0's top-left border; the last image's bottom-right border; one window straddling each of the byte offsets
    2^31 and 2^32 and the element offset 2^31 that the tensor reaches (rows above the offset and rows below it; windows
    do not cross images, so where the offset is an image's first element the window begins there); and the
    aliases of the last window -- its offset minus 2^32 bytes, and minus 2^31 elements -- where those are >= 0.
    A wrapped store lands in the alias windows, a wrapped load shows in the straddling ones."""
    n_img, h, w, c = shape
    numel = n_img * h * w * c
    ch, cw = min(CROP_H, h), min(CROP_W, w)
    first = (0, 0, 0, ch, cw)
    last = (n_img - 1, h - ch, w - cw, ch, cw)
    wins = [first, last]
    for elem in (2 ** 31 // esize, 2 ** 32 // esize, 2 ** 31):
        if numel > elem:
            wins.append(_window_at(shape, elem))
    last_pixel = ((n_img - 1) * h + h - 1) * w + w - 1      # the tensor's last pixel: inside the last window
    for back in (2 ** 32 // esize, 2 ** 31):
        e = last_pixel * c - back
        if e >= 0:
            n, y0, x0, _, _ = _window_at(shape, e)
            p = e // c                                      # keep the aliased pixel at the window's far corner if possible
            y, x = divmod(p % (h * w), w)
            wins.append((n, min(max(y - ch + 1, 0), h - ch), min(max(x - cw + 1, 0), w - cw), ch, cw))
    out = []
    for win in wins:
        if win not in out:
            out.append(win)
    assert len(out) <= MAX_CROPS
    return out


def crop_with_halo(t: torch.Tensor, win, halo: int, load=None) -> torch.Tensor:
    """float64 host copy [rows + 2 halo, cols + 2 halo, C] of a window of a device NHWC tensor, zero outside the image;
    load: the kernel's transform on load, applied to the pixels inside the image (the padding stays zero)"""
    _, h, w, c = t.shape
    n, y0, x0, ch, cw = win
    out = torch.zeros(ch + 2 * halo, cw + 2 * halo, c, dtype=torch.float64)
    ys, ye = max(y0 - halo, 0), min(y0 + ch + halo, h)
    xs, xe = max(x0 - halo, 0), min(x0 + cw + halo, w)
    inside = t[n, ys:ye, xs:xe].cpu().double()
    out[ys - (y0 - halo):ye - (y0 - halo), xs - (x0 - halo):xe - (x0 - halo)] = inside if load is None else load(inside)
    return out


def crop(t: torch.Tensor, win) -> torch.Tensor:
    """host copy of a window of a device NHWC tensor, in its own type"""
    n, y0, x0, ch, cw = win
    return t[n, y0:y0 + ch, x0:x0 + cw].cpu()


def bands(n: int, h: int, rows: int = 1024, halo: int = 0):
    """(image, first row, one past the last row, first row read, one past the last row read): every image cut into bands
    of at most `rows` rows (an even number), each far below every size limit; `halo` rows of the image are read on both
    sides where the image has them, so the band's own rows see the neighbours a 3x3 needs."""
    for i in range(n):
        for a in range(0, h, rows):
            b = min(a + rows, h)
            yield i, a, b, max(a - halo, 0), min(b + halo, h)


def wino_magnitude_bound(c_in: int, x_abs: float, w_abs: float, extra: float = 0.0) -> float:
    """helpers.wino_magnitude of the largest operands of a range (it is monotone in |x| and |w|) plus bias / old value"""
    from tests.helpers import wino_magnitude
    x = torch.full((1, c_in, 6, 6), float(x_abs), dtype=torch.float64)
    w = torch.full((1, c_in, 3, 3), float(w_abs), dtype=torch.float64)
    return float(wino_magnitude(x, w).max()) + extra
