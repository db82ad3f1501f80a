"""Float64 statement of the weight gradient as ops.wgrad takes it, and the operands its exact tests run on.

    dW[tap][k][n] = sum over pixels p of x[p (+) tap, k] * dy[p, n]          db[n] = sum over p of dy[p, n]

x and dy are virtual concatenations of views (channel slices of NHWC tensors, dy possibly on a strided pixel grid), x
may carry a folded scale / shift / ReLU, dy a ReLU gate.  The sums are written out as shifted slices and einsums (no
autograd: tests/test_wgrad_oracle_host.py holds THIS file against autograd).

Why equality can be demanded.  On small-integer operands every product, every partial sum, the Winograd transforms
B^T d B and A dY A^T, and the multiples of 1/4 the finish's G^T . G introduces are exactly representable in fp32 as
long as the sum of ABSOLUTE terms an accumulator can see stays below 2^22 (`exactness_margin`, a precondition of the
data, not a tolerance).  Then the result is the same in any summation order and for any split, and a kernel that
drops, duplicates, misplaces or reuses a single term is off by at least 1/4 somewhere.
"""
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

F64 = torch.float64
EXACT_LIMIT = 2.0 ** 22

# F(2x2, 3x3) of the weight gradient: dg = G^T [ sum over 2x2 tiles of (B^T d B) . (A dY A^T) ] G
WINO_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
WINO_G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
WINO_A = [[1, 0], [1, 1], [1, -1], [0, -1]]
# the kernel takes A's last row as (0, +1) and the finish multiplies plane (a, b) by (-1)^[a == 3] (-1)^[b == 3]
WINO_A_UNSIGNED = [[1, 0], [1, 1], [1, -1], [0, 1]]
WINO_G_SIGNED = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, -1]]


def tile_geom(h: int, w: int):
    """(log2tw, tiles_x, tiles_y) of the 256-pixel patches (csrc/common.h tile_geom): 32 x 8, 16 x 16 or 8 x 32"""
    l = 3
    while (1 << l) < w and l < 5:
        l += 1
    tw, th = 1 << l, 256 >> l
    return l, (w + tw - 1) // tw, (h + th - 1) // th


def pixel_tiles(n: int, h: int, w: int) -> int:
    _, tx, ty = tile_geom(h, w)
    return n * tx * ty


@dataclass
class OView:
    """unetpp_view on the host: a channel slice of an NHWC float64 tensor on a strided pixel grid.  scale / shift are
    indexed by the channel INSIDE the slice; gate has the tensor's geometry (the value is kept where gate > 0)."""
    t: torch.Tensor
    c_off: int = 0
    c_len: Optional[int] = None
    sy: int = 1
    sx: int = 1
    oy: int = 0
    ox: int = 0
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    relu: bool = False
    gate: Optional[torch.Tensor] = None

    @property
    def width(self) -> int:
        return self.t.shape[3] - self.c_off if self.c_len is None else self.c_len

    def _cut(self, t, h, w):
        return t[:, self.oy:self.oy + (h - 1) * self.sy + 1:self.sy, self.ox:self.ox + (w - 1) * self.sx + 1:self.sx,
                 self.c_off:self.c_off + self.width]

    def logical(self, h: int, w: int) -> torch.Tensor:
        """[N, h, w, c_len] float64: what the kernel multiplies (load transform and gate applied)"""
        v = self._cut(self.t, h, w).to(F64)
        if self.scale is not None:
            v = v * self.scale.to(F64) + self.shift.to(F64)
        if self.relu:
            v = v.clamp_min(0.0)
        if self.gate is not None:
            v = torch.where(self._cut(self.gate, h, w) > 0, v, torch.zeros_like(v))
        return v


def concat(views, h, w) -> torch.Tensor:
    return torch.cat([v.logical(h, w) for v in views], 3)


def shifted_sums(x: torch.Tensor, dy: torch.Tensor, taps: int) -> torch.Tensor:
    """[taps, K, Ncols]: plane 3 r + s = sum over pixels of x[p + (r - 1, s - 1)] (zero outside the image) * dy[p]"""
    n, h, w, _ = x.shape
    if taps == 1:
        return torch.einsum("nhwk,nhwc->kc", x, dy)[None]
    assert taps == 9
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    return torch.stack([torch.einsum("nhwk,nhwc->kc", xp[:, r:r + h, s:s + w], dy) for r in range(3) for s in range(3)])


def scatter_dw(planes: torch.Tensor, dw_strides, n_inner: int, dw_numel: Optional[int] = None) -> torch.Tensor:
    """planes [taps, K, Ncols] -> the flat destination: element (t, k, n) at t d_t + k d_k + (n % n_inner) d_n +
    (n // n_inner) d_o.  Every destination element must be hit exactly once."""
    taps, k, nc = planes.shape
    d_t, d_k, d_n, d_o = dw_strides
    t_i = torch.arange(taps).view(-1, 1, 1)
    k_i = torch.arange(k).view(1, -1, 1)
    n_i = torch.arange(nc).view(1, 1, -1)
    idx = (t_i * d_t + k_i * d_k + (n_i % n_inner) * d_n + (n_i // n_inner) * d_o).reshape(-1)
    numel = int(idx.max()) + 1 if dw_numel is None else dw_numel
    assert idx.numel() == numel and torch.unique(idx).numel() == numel, "the strides do not tile the destination"
    out = torch.empty(numel, dtype=planes.dtype)
    out[idx] = planes.reshape(-1)
    return out


def wgrad_reference(h, w, taps, xs, dys, dw_strides, n_inner=None, dw_numel=None):
    """(dW flat in the destination layout, db [n_inner]) in float64.  n_inner < Ncols is the deconvolution form: column
    o * n_inner + c is pixel phase o of output channel c, and db[c] sums its phases."""
    x, dy = concat(xs, h, w), concat(dys, h, w)
    nc = dy.shape[3]
    n_inner = nc if n_inner is None else n_inner
    assert nc % n_inner == 0
    dw = scatter_dw(shifted_sums(x, dy, taps), dw_strides, n_inner, dw_numel)
    db = dy.sum((0, 1, 2)).view(nc // n_inner, n_inner).sum(0)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), "the oracle read a poisoned element"
    return dw, db


# ------------------------------------------------------------------------------------------------ Winograd form
def wino_planes(x: torch.Tensor, dy: torch.Tensor, absolute: bool = False) -> torch.Tensor:
    """[16, K, Ncols]: plane 4 a + b = sum over 2x2 tiles of (B^T d B)[a][b] * (A' dY A'^T)[a][b], A' = A with the
    unsigned last row (what the kernel's slabs hold).  absolute: |B^T|, |A'| on the operands given (magnitudes)."""
    n, h, w, _ = x.shape
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = torch.nn.functional.pad(x, (0, 0, 1, 2 * tw - w + 1, 1, 2 * th - h + 1))
    yp = torch.nn.functional.pad(dy, (0, 0, 0, 2 * tw - w, 0, 2 * th - h))
    bt = torch.tensor(WINO_BT, dtype=x.dtype)
    au = torch.tensor(WINO_A_UNSIGNED, dtype=x.dtype)
    if absolute:
        bt, au = bt.abs(), au.abs()
    d = torch.stack([torch.stack([xp[:, a:a + 2 * th:2, b:b + 2 * tw:2] for b in range(4)]) for a in range(4)])
    e = torch.stack([torch.stack([yp[:, p::2, q::2] for q in range(2)]) for p in range(2)])
    v = torch.einsum("ia,jb,abntuk->ijntuk", bt, bt, d)
    m = torch.einsum("ip,jq,pqntuc->ijntuc", au, au, e)
    return torch.einsum("ijntuk,ijntuc->ijkc", v, m).reshape(16, x.shape[3], dy.shape[3])


def wino_finish(u: torch.Tensor, absolute: bool = False) -> torch.Tensor:
    """G^T U G with the sign of the unsigned last row: [16, K, Ncols] -> [9, K, Ncols]"""
    g = torch.tensor(WINO_G_SIGNED, dtype=u.dtype)
    if absolute:
        g = g.abs()
    k, nc = u.shape[1:]
    return torch.einsum("ar,bc,abkn->rckn", g, g, u.view(4, 4, k, nc)).reshape(9, k, nc)


# ------------------------------------------------------------------------------------------------ cases and operands
@dataclass(frozen=True)
class Case:
    """One row of a case table.  xs: (C of the tensor, c_off, c_len) per x view; dy: the same for dy.  deconv: dy is a
    tensor at twice the resolution seen through its four pixel phases (c_len = output channels per phase), dW in the
    transposed-convolution layout [K][co][2][2].  fold: per x view, scale / shift / ReLU folded into the read."""
    id: str
    label: str
    shape: Tuple[int, int, int]
    xs: Tuple[Tuple[int, int, int], ...]
    dy: Tuple[int, int, int]
    splits: Tuple[int, ...]
    taps: int = 9
    deconv: bool = False
    fold: Tuple[bool, ...] = ()
    gate: bool = False
    bf16: bool = False
    direct: bool = False
    dy_pad: int = 0   # deconvolution form: rows / columns of the dy tensor past the last phase pixel

    @property
    def k(self):
        return sum(v[2] for v in self.xs)

    @property
    def ncols(self):
        return self.dy[2] * (4 if self.deconv else 1)

    @property
    def first_layer(self):
        return self.label == "small_cin_wgrad_kernel"

    @property
    def wino(self):
        return self.label == "wgrad_wino_kernel"

    @property
    def cover(self):
        """the coverage key: the label, told apart where one label names several instantiations"""
        if self.first_layer:
            return "%s C=%d %s" % (self.label, self.xs[0][0], "bf16" if self.bf16 else "fp32")
        if self.wino:
            return "%s %s" % (self.label, "folded" if any(self.fold) else "plain")
        return self.label

    @property
    def dw_shape(self):
        if self.deconv:
            return (self.k, self.dy[2], 2, 2)
        return (self.dy[2], self.k, 3, 3) if self.taps == 9 else (self.dy[2], self.k, 1, 1)

    @property
    def dw_strides(self):
        if self.deconv:
            return (0, 4 * self.dy[2], 4, 1)
        return (1, 9, 9 * self.k, 0) if self.taps == 9 else (0, 1, self.k, 0)

    @property
    def n_inner(self):
        return self.dy[2]

    @property
    def max_split(self):
        return min(4096, pixel_tiles(*self.shape))


def _v3(v):
    return (v, 0, v) if isinstance(v, int) else tuple(v)


def case(id, label, shape, xs, dy, splits, fold=False, **kw) -> Case:
    xs = tuple(_v3(v) for v in xs)
    if isinstance(fold, bool):
        fold = (fold,) * len(xs)
    return Case(id, label, tuple(shape), xs, _v3(dy), tuple(splits), fold=tuple(fold), **kw)


@dataclass
class Operands:
    xs: list
    dys: list


def _gen(c: Case, salt: str):
    return torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (c.id, salt)).encode()))


def _poison_outside(t: torch.Tensor, c_off: int, c_len: int) -> torch.Tensor:
    """NaN in the channels a view does not cover: a kernel that reads past its slice cannot stay exact"""
    t[..., :c_off] = float("nan")
    t[..., c_off + c_len:] = float("nan")
    return t


def _ints(g, shape, lo, hi, zero_share):
    v = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    return v * (torch.rand(shape, generator=g) >= zero_share)


def fold_parameters(g, c_len: int):
    """scale in {0, +-0.5, +-1, +-2} with a zero, a negative and a positive channel, shift a multiple of 0.5 in [-4, 4]:
    x * scale + shift is the same number fused or not, and a bf16 value"""
    choices = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=F64)
    scale = choices[torch.randint(0, 7, (c_len,), generator=g)]
    scale[0], scale[1], scale[2] = 0.0, -1.0, 2.0
    shift = torch.randint(-8, 9, (c_len,), generator=g).to(F64) * 0.5
    shift[0] = 1.5   # (the zero-scale channel still carries a value)
    return scale, shift


def _dy_views(c: Case, t: torch.Tensor, gate):
    _, c_off, c_len = c.dy
    if c.deconv:
        return [OView(t, c_off, c_len, sy=2, sx=2, oy=a, ox=b, gate=gate) for a in (0, 1) for b in (0, 1)]
    return [OView(t, c_off, c_len, gate=gate)]


def _dy_tensor_shape(c: Case):
    n, h, w = c.shape
    return (n, 2 * h + c.dy_pad, 2 * w + c.dy_pad, c.dy[0]) if c.deconv else (n, h, w, c.dy[0])


def _poison_dy(c: Case, t: torch.Tensor) -> torch.Tensor:
    _poison_outside(t, c.dy[1], c.dy[2])
    if c.deconv and c.dy_pad:   # pixels that belong to no phase of the launch
        n, h, w = c.shape
        t[:, 2 * h:] = float("nan")
        t[:, :, 2 * w:] = float("nan")
    return t


def integer_operands(c: Case, zero_share: float = 0.25) -> Operands:
    """x in [-3, 3], dy in [-2, 2], a share of zeros, gate values in [-2, 2]; seeded by the case id"""
    n, h, w = c.shape
    g = _gen(c, "int")
    xs = []
    for (ct, c_off, c_len), fold in zip(c.xs, c.fold):
        t = _poison_outside(_ints(g, (n, h, w, ct), -3, 3, zero_share), c_off, c_len)
        scale, shift = fold_parameters(g, c_len) if fold else (None, None)
        xs.append(OView(t, c_off, c_len, scale=scale, shift=shift, relu=fold))
    shape = _dy_tensor_shape(c)
    t = _poison_dy(c, _ints(g, shape, -2, 2, zero_share))
    gate = _poison_dy(c, _ints(g, shape, -2, 2, 0.0)) if c.gate else None
    return Operands(xs, _dy_views(c, t, gate))


def impulse_pixels(n: int, h: int, w: int):
    """(image, y, x): the four image corners (the last one is the last pixel of the last image), both sides of a patch
    boundary in x and in y where the image has one, and a pixel inside the first patch"""
    l, tiles_x, tiles_y = tile_geom(h, w)
    tw, th = 1 << l, 256 >> l
    px = [(0, 0, 0), (0, 0, w - 1), (n - 1, h - 1, 0), (n - 1, h - 1, w - 1)]
    if tiles_x > 1:
        px += [(0, min(3, h - 1), tw - 1), (0, min(3, h - 1), tw)]
    if tiles_y > 1:
        px += [(n - 1, th - 1, min(5, w - 1)), (n - 1, th, min(5, w - 1))]
    px.append((0, min(h - 1, 2), min(w - 1, 9)))
    out = []
    for p in px:
        if p not in out:
            out.append(p)
    return out


def impulse_operands(c: Case, chunk: int):
    """Full-mantissa x (randn in fp32; bf16 cases: rounded to bf16), dy zero except a 1.0 at impulse pixel i in column
    i: dW[:, k, i] is then the 3x3 window of x around that pixel -- for a direct sum a COPY of x.  The impulse pixels are
    taken Ncols at a time (`chunk`); a fold is scale 1, shift 0, ReLU (exact); a gate is positive except at the chunk's
    first pixel, whose column must come out zero.  Returns (operands, [(pixel, column)])."""
    n, h, w = c.shape
    assert not c.deconv
    g = _gen(c, "impulse")
    pixels = impulse_pixels(n, h, w)
    nc = c.dy[2]
    mine = pixels[chunk * nc:(chunk + 1) * nc]
    assert mine, "no such chunk"
    xs = []
    for (ct, c_off, c_len), fold in zip(c.xs, c.fold):
        t = torch.randn((n, h, w, ct), generator=g, dtype=torch.float32)
        if c.bf16 and not c.first_layer:
            t = t.bfloat16().float()
        t = _poison_outside(t.to(F64), c_off, c_len)
        one, zero = (torch.ones(c_len, dtype=F64), torch.zeros(c_len, dtype=F64)) if fold else (None, None)
        xs.append(OView(t, c_off, c_len, scale=one, shift=zero, relu=fold))
    t = torch.zeros(_dy_tensor_shape(c), dtype=F64)
    gate = torch.ones_like(t) if c.gate else None
    pairs = []
    for col, (i, y, x) in enumerate(mine):
        t[i, y, x, c.dy[1] + col] = 1.0
        pairs.append(((i, y, x), col))
    if c.gate:
        gate[mine[0][0], mine[0][1], mine[0][2]] = -1.0
        _poison_dy(c, gate)
    return Operands(xs, _dy_views(c, _poison_dy(c, t), gate)), pairs


def impulse_chunks(c: Case) -> int:
    return (len(impulse_pixels(*c.shape)) + c.dy[2] - 1) // c.dy[2]


def reference(c: Case, ops: Operands):
    n, h, w = c.shape
    numel = 1
    for s in c.dw_shape:
        numel *= s
    return wgrad_reference(h, w, c.taps, ops.xs, ops.dys, c.dw_strides, c.n_inner, numel)


def exactness_margin(c: Case, ops: Operands) -> float:
    """The largest sum of absolute terms any fp32 accumulator of the case can see: conv(|x|, |dy|) and sum |dy| for the
    direct sums; for the Winograd kernel the same through |B^T| and |A| (the transform-domain planes) and through |G|
    (the finish, which works in multiples of 1/4).  Exactness needs margin < 2^22 (EXACT_LIMIT)."""
    n, h, w = c.shape
    x, dy = concat(ops.xs, h, w).abs(), concat(ops.dys, h, w).abs()
    m = max(float(shifted_sums(x, dy, c.taps).max()), float(dy.sum((0, 1, 2)).max()))
    if c.wino:
        u = wino_planes(x, dy, absolute=True)
        m = max(m, float(u.max()), float(wino_finish(u, absolute=True).max()))
    return m
