"""Float64 statement of ops.gemm_fwd as the library takes it, the operands its exact tests run on, the case rows of
tests/test_gpu_gemm_bf16_exact.py and a host restatement of the launchers' choices for them.

    acc[p, n] = sum over taps, k of X[p (+) tap, k] * W[tap, k, n]           (zero padding AFTER the load transform)
    X         = the concatenation of the input views, each bf(relu(fma(x, scale, shift))) where it carries a transform
    out       = epilogue(acc, bias, ReLU, gate, old)                         (`epilogue`: one of two rounding rules)

The sum is written as explicit shifted slices (no conv2d, no autograd: tests/test_gemm_oracle_host.py holds THIS file
against them).  Input views are tests/wgrad_oracle.py's OView: channel slices, strided phase views, folded scale /
shift / ReLU.

Why equality can be demanded.  bf16 holds the integers up to 256, every product of two of them is an fp32 number, and
every fp32 partial sum is exact in any order while the sum of ABSOLUTE terms stays below 2^24 times the data's granule
(`exactness_margin` < EXACT_LIMIT = 2^22: the granule may be 1/4).  What is left are the roundings to bf16, each a
round-to-nearest-even of an exactly known fp32 number, so the stored bits are determined, ties included (257 -> 256,
259 -> 260).  The family has TWO rules for where it rounds (`epilogue`, ROUNDINGS): gemm_bf16_kernel and
gemm_bf16_dma_kernel round acc + bias (after ReLU) to bf16 and, when the view carries a gate or accumulates, apply those
in fp32 to the ROUNDED value and round again; gemm_pw_bf16_kernel keeps fp32 through all of it and rounds once.
"""
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

from tests.wgrad_oracle import EXACT_LIMIT, F64, OView, concat, tile_geom  # noqa: F401  (re-exported)

REG9, REG1 = "gemm_bf16_kernel<9>", "gemm_bf16_kernel<1>"
DMA9, DMA1 = "gemm_bf16_dma_kernel<9>", "gemm_bf16_dma_kernel<1>"
PWB, SMALL, FLD = "gemm_pw_bf16_kernel", "small_cin_fwd_kernel", "first_layer_dgrad_bf16"
# roundings between the fp32 accumulator and the stored bf16 value when the view has a gate or accumulates
ROUNDINGS = {REG9: 2, REG1: 2, DMA9: 2, DMA1: 2, PWB: 1, SMALL: 1}


# ------------------------------------------------------------------------------------------------ bf16 rounding
def bf(x: torch.Tensor) -> torch.Tensor:
    """round-to-nearest-even of an fp32 number to bf16, on the bit pattern (no torch.bfloat16 cast: the host test holds
    this against the cast).  x: float64 holding fp32 numbers exactly (asserted: otherwise there would be a rounding to
    fp32 in front that the kernels do not have).  NaN passes through."""
    f = x.to(torch.float32)
    ok = torch.isnan(x) | (f.to(F64) == x)
    assert bool(ok.all()), "bf() of a value that is no fp32 number"
    b = f.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000)
    r = torch.where(r >= 2 ** 31, r - 2 ** 32, r).to(torch.int32)
    return torch.where(torch.isnan(x), x, r.view(torch.float32).to(F64))


def is_tie(x: torch.Tensor) -> torch.Tensor:
    """the fp32 number lies exactly between two bf16 numbers"""
    b = x.to(torch.float32).view(torch.int32).to(torch.int64) & 0xFFFF
    return (b == 0x8000) & ~torch.isnan(x)


def fp32_exact(x: torch.Tensor) -> bool:
    return bool((torch.isnan(x) | (x.to(torch.float32).to(F64) == x)).all())


# ------------------------------------------------------------------------------------------------ weights [taps][K][N]
def w_conv_fwd(w):
    """torch Conv2d weight [co, ci, kh, kw] -> [taps][ci][co], tap = 3 r + s"""
    co, ci, kh, kw = w.shape
    return w.permute(2, 3, 1, 0).reshape(kh * kw, ci, co)


def w_conv_dgrad(w):
    """[co, ci, kh, kw] -> [taps rotated by 180 degrees][co][ci]: dx = the same sum over dy with these weights"""
    co, ci, kh, kw = w.shape
    return w.flip(2, 3).permute(2, 3, 0, 1).reshape(kh * kw, co, ci)


def w_deconv_fwd(w):
    """ConvTranspose2d(2, 2) weight [ci, co, 2, 2] -> [1][ci][4 co], column (2 a + b) co + c: phase (a, b) of channel c"""
    ci, co = w.shape[:2]
    return w.permute(0, 2, 3, 1).reshape(1, ci, 4 * co)


def w_deconv_dgrad(w):
    """[ci, co, 2, 2] -> [1][4 co][ci], row (2 a + b) co + c"""
    ci, co = w.shape[:2]
    return w.permute(2, 3, 1, 0).reshape(1, 4 * co, ci)


WEIGHT_FORMS = {"fwd": w_conv_fwd, "dgrad": w_conv_dgrad, "deconv_fwd": w_deconv_fwd, "deconv_dgrad": w_deconv_dgrad}


# ------------------------------------------------------------------------------------------------ the sum
def gemm_sum(x: torch.Tensor, wt: torch.Tensor) -> torch.Tensor:
    """x [N, h, w, K], wt [taps, K, Ncols] -> [N, h, w, Ncols]: tap 3 r + s reads pixel (y + r - 1, x + s - 1), zero
    outside the image.  (+ 0.0: an accumulator starts at +0, so a sum of zeros of either sign is +0)"""
    taps = wt.shape[0]
    n, h, w, _ = x.shape
    if taps == 1:
        return x @ wt[0] + 0.0
    assert taps == 9
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(n, h, w, wt.shape[2], dtype=x.dtype)
    for r in range(3):
        for s in range(3):
            acc = acc + xp[:, r:r + h, s:s + w] @ wt[3 * r + s]
    return acc + 0.0


def load_view(v: OView, h: int, w: int, bf16: bool = True) -> torch.Tensor:
    """what the kernel multiplies: bf(relu(fma(x, scale, shift))), the fma in fp32 (its exact value must be an fp32
    number: the `fold` precondition), a gate on load applied last (fp32 kernels)"""
    x = v._cut(v.t, h, w).to(F64)
    if v.scale is not None:
        x = x * v.scale.to(F64) + v.shift.to(F64)
        assert not bf16 or fp32_exact(x), "x * scale + shift is no fp32 number"
    if v.relu:
        x = x.clamp_min(0.0)
    if bf16 and (v.scale is not None or v.relu):
        x = bf(x)
    if v.gate is not None:
        x = torch.where(v._cut(v.gate, h, w) > 0, x, torch.zeros_like(x))
    return x


def epilogue(acc, bias, relu, gate, gate_sum, old, roundings, bf16=True):
    """-> (stored, first): `first` is the value in front of the first rounding.
    roundings == 2:  s = bf(relu?(acc + bias)); gate unless it is the gate of the sum; + old in fp32; gate of the sum;
                     bf(.) again, only when a gate or an accumulate is present
    roundings == 1:  the same sequence without the first bf"""
    assert roundings in (1, 2)
    v = acc if bias is None else acc + bias
    if relu:
        v = v.clamp_min(0.0)
    first = v
    rmw = gate is not None or old is not None
    if bf16 and roundings == 2:
        v = bf(v)
    if gate is not None and not gate_sum:
        v = torch.where(gate > 0, v, torch.zeros_like(v))
    if old is not None:
        v = v + old
    if gate is not None and gate_sum:
        v = torch.where(gate > 0, v, torch.zeros_like(v))
    if bf16 and (roundings == 1 or rmw):
        v = bf(v)
    return v, first


# ------------------------------------------------------------------------------------------------ case rows
@dataclass(frozen=True)
class Row:
    """One launch.  ins: (C of the tensor, c_off, c_len) per input view; outs: (C, c_off, c_len, kind), kind one of
    store / acc / gate / accgate (accumulate + gate of the sum).  form: fwd / dgrad (weights of a Conv2d, taps 9 or 1),
    deconv_fwd (one input view, the outs entry is the tensor at twice the resolution seen through its four phases),
    deconv_dgrad (the ins entry is that tensor, K = 4 c_len).  family: k9 / k1 (gemm_bf16*.hip, PW_DIRECT=0 for k1), pw
    (default dispatch of a pointwise launch), small, fld.  claims: what the data must do (asserted on the CPU)."""
    id: str
    family: str
    shape: Tuple[int, int, int]
    form: str
    ins: Tuple[Tuple[int, int, int], ...]
    outs: Tuple[Tuple[int, int, int, str], ...]
    taps: int = 9
    relu: bool = False
    bias: bool = False          # integer bias that pushes every second column to about +-300
    stats: bool = False
    fold: str = ""              # "" / exact / round: scale, shift, ReLU folded into the first input view
    data: str = "int"           # int / impulse_w / impulse_x
    variants: Tuple[str, ...] = ()
    multi: bool = False         # more units than workgroups at 8 CUs, in every variant
    claims: Tuple[str, ...] = ()
    wmax: int = 2

    @property
    def deconv(self):
        return self.form.startswith("deconv")

    @property
    def in_lens(self):
        return [v[2] for v in self.ins] * (4 if self.form == "deconv_dgrad" else 1)

    @property
    def out_lens(self):
        return [v[2] for v in self.outs] * (4 if self.form == "deconv_fwd" else 1)

    @property
    def k(self):
        return sum(self.in_lens)

    @property
    def ncols(self):
        return sum(self.out_lens)

    @property
    def plain_out(self):
        return all(o[3] == "store" for o in self.outs)


def _v3(v):
    return (v, 0, v) if isinstance(v, int) else tuple(v)


def _v4(v):
    if isinstance(v, int):
        return (v, 0, v, "store")
    if len(v) == 2:
        return (v[0], 0, v[0], v[1])
    return tuple(v) if len(v) == 4 else tuple(v) + ("store",)


def row(id, family, shape, form, ins, outs, **kw) -> Row:
    """claims follow from the data: an integer row with the tie bias rounds (>= 1 % of its elements) and has ties; with
    an accumulating view on top the two rounding rules differ somewhere; a rounding fold rounds on load"""
    kw = dict(kw)
    kw["variants"] = tuple(kw["variants"])
    outs = tuple(_v4(v) for v in outs)
    claims = []
    if kw.get("data", "int") == "int":
        if kw.get("bias") or kw.get("fold") == "round":
            claims.append("round")
        if kw.get("bias"):
            claims.append("ties")
            if family != "small" and any(o[3] in ("acc", "accgate") for o in outs):
                claims.append("disc")
        if kw.get("fold") == "round":
            claims.append("fold")
    return Row(id, family, tuple(shape), form, tuple(_v3(v) for v in ins), outs, claims=tuple(claims), **kw)


# ------------------------------------------------------------------------------------------------ operands
@dataclass
class Operands:
    ins: list                    # OView per input view (float64 tensors; NaN outside the slices)
    weight: torch.Tensor         # the parameter in its torch layout (float64)
    wt: torch.Tensor             # [taps][K][Ncols]
    bias: Optional[torch.Tensor]       # per GEMM column (deconv_fwd: the channel bias once per phase) or None
    bias_param: Optional[torch.Tensor]  # the parameter (deconv_fwd: per channel)
    out_tensors: list            # initial contents of every output tensor (NaN where nothing may be read)
    outs: list = field(default_factory=list)   # (tensor index, OView over it (gate = its gate tensor or None), kind)


def _gen(r: Row, salt: str):
    return torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (r.id, salt)).encode()))


def _ints(g, shape, lo, hi, zero_share=0.25):
    v = torch.randint(lo, hi + 1, shape, generator=g).to(F64)
    return torch.where(torch.rand(shape, generator=g) >= zero_share, v, torch.zeros_like(v))   # (no -0.0)


def _full_mantissa(g, shape):
    """+-(1 + m / 128) 2^e, m in 0 .. 127, e in -3 .. 3: every bf16 mantissa bit in use, never zero, and the sum of two
    of them is an fp32 number"""
    m = torch.randint(0, 128, shape, generator=g).to(F64)
    e = torch.randint(-3, 4, shape, generator=g).to(F64)
    sgn = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=g).to(F64)
    return sgn * (1.0 + m / 128.0) * torch.pow(torch.tensor(2.0, dtype=F64), e)


def _poison(t, c_off, c_len):
    t[..., :c_off] = float("nan")
    t[..., c_off + c_len:] = float("nan")
    return t


def _weight_shape(r: Row):
    kk = 3 if r.taps == 9 else 1
    if r.form == "fwd":
        return (r.ncols, r.k, kk, kk)
    if r.form == "dgrad":
        return (r.k, r.ncols, kk, kk)
    if r.form == "deconv_fwd":
        return (r.k, r.outs[0][2], 2, 2)
    return (r.ncols, r.ins[0][2], 2, 2)


def tie_bias(g, n: int, positive: bool = False) -> torch.Tensor:
    """an integer per column: +-(297 .. 303) on every second column (sums of a few dozen then land in 257 .. 511, where
    every odd integer is a tie), -2 .. 2 on the others; positive: under a ReLU (no column may come out all zero)"""
    b = torch.randint(-2, 3, (n,), generator=g).to(F64)
    big = (297 + torch.randint(0, 7, (n,), generator=g)).to(F64) * (1 - 2 * (torch.arange(n) % 4 == 1).to(F64))
    if positive:
        big = big.abs()
    return torch.where(torch.arange(n) % 2 == 1, big, b)


def fold_parameters(g, c_len: int, kind: str):
    """exact: scale in {0, +-0.5, +-1, +-2}, shift a multiple of 0.5 (x in [-3, 3]: the fma is a bf16 number);
    round: scale in {17, 33}, shift in {0.5, 1} (x in [-15, 15]: 255.5 -> 256, 463 -> 464, ...)"""
    if kind == "exact":
        choices = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=F64)
        scale = choices[torch.randint(0, 7, (c_len,), generator=g)]
        scale[0], scale[1], scale[2] = 0.0, -1.0, 2.0
        shift = torch.randint(-8, 9, (c_len,), generator=g).to(F64) * 0.5
        shift[0] = 1.5
        return scale, shift
    scale = torch.tensor([17.0, 33.0], dtype=F64)[torch.randint(0, 2, (c_len,), generator=g)]
    shift = torch.tensor([0.5, 1.0], dtype=F64)[torch.randint(0, 2, (c_len,), generator=g)]
    scale[0], shift[0] = 17.0, 0.5
    return scale, shift


def _impulse_pixels(n, h, w):
    """pixels three apart in both directions (their 3x3 windows do not meet), the image corners among them"""
    ys = sorted(set(list(range(0, h, 3)) + ([h - 1] if (h - 1) % 3 == 0 else [])))
    xs = list(range(0, w, 3))
    return [(i, y, x) for i in range(n) for y in ys for x in xs]


def operands(r: Row) -> Operands:
    n, h, w = r.shape
    g = _gen(r, r.data)
    full = r.data != "int"          # full-mantissa bf16 values somewhere
    # ---- inputs
    hi_, wi_ = (2 * h, 2 * w) if r.form == "deconv_dgrad" else (h, w)
    ins = []
    for i, (ct, c_off, c_len) in enumerate(r.ins):
        fold = r.fold if i == 0 else ""
        if r.data == "impulse_w":
            t = _full_mantissa(g, (n, hi_, wi_, ct))
        elif r.data == "impulse_x":
            t = torch.zeros((n, hi_, wi_, ct), dtype=F64)
            for j, (b, y, x) in enumerate(_impulse_pixels(n, hi_, wi_)):
                t[b, y, x, c_off + j % c_len] = 1.0
        else:
            lim = 15 if fold == "round" else 3
            t = _ints(g, (n, hi_, wi_, ct), -lim, lim)
        t = _poison(t, c_off, c_len)
        scale, shift = fold_parameters(g, c_len, fold) if fold else (None, None)
        if r.form == "deconv_dgrad":
            ins += [OView(t, c_off, c_len, sy=2, sx=2, oy=a, ox=b) for a in (0, 1) for b in (0, 1)]
        else:
            ins.append(OView(t, c_off, c_len, scale=scale, shift=shift, relu=bool(fold)))
    # ---- weights
    shape = _weight_shape(r)
    if r.data == "impulse_w":        # one 1.0 per GEMM column: the output is a shifted copy of one input channel
        wt = torch.zeros(r.taps, r.k, r.ncols, dtype=F64)
        for c in range(r.ncols):
            wt[(5 * c + 1) % r.taps, (7 * c + 3) % r.k, c] = 1.0
        weight = _invert_weight_form(r, wt, shape)
    elif r.data == "impulse_x":      # full-mantissa bf16 weights: the output around an impulse is a copy of them
        weight = _full_mantissa(g, shape)
    else:
        weight = _ints(g, shape, -r.wmax, r.wmax)
    wt = WEIGHT_FORMS[r.form](weight).contiguous()
    # ---- bias
    bias = bias_param = None
    if r.bias:
        bias_param = tie_bias(g, r.outs[0][2] if r.form == "deconv_fwd" else r.ncols, r.relu)
        bias = bias_param.repeat(4) if r.form == "deconv_fwd" else bias_param
    # ---- outputs: NaN wherever nothing may be read, integers where the view accumulates, a gate with zeros and negatives
    ho, wo_ = (2 * h, 2 * w) if r.form == "deconv_fwd" else (h, w)
    out_tensors, outs = [], []
    for (ct, c_off, c_len, kind) in r.outs:
        t = torch.full((n, ho, wo_, ct), float("nan"), dtype=F64)
        gate = None
        if kind in ("acc", "accgate"):
            t[..., c_off:c_off + c_len] = (_full_mantissa(g, (n, ho, wo_, c_len)) if full else _ints(g, (n, ho, wo_, c_len), -3, 3))
        if kind in ("gate", "accgate"):
            gate = _poison(_ints(g, (n, ho, wo_, ct), -2, 2, 0.0), c_off, c_len)
        out_tensors.append(t)
        idx = len(out_tensors) - 1
        if r.form == "deconv_fwd":
            outs += [(idx, OView(t, c_off, c_len, sy=2, sx=2, oy=a, ox=b, gate=gate), kind) for a in (0, 1) for b in (0, 1)]
        else:
            outs.append((idx, OView(t, c_off, c_len, gate=gate), kind))
    return Operands(ins, weight, wt, bias, bias_param, out_tensors, outs)


def _invert_weight_form(r: Row, wt, shape):
    """the parameter whose GEMM operand is wt (the forms are permutations: scatter through an index tensor)"""
    numel = 1
    for s in shape:
        numel *= s
    idx = WEIGHT_FORMS[r.form](torch.arange(numel, dtype=F64).view(shape)).reshape(-1).long()
    flat = torch.empty(numel, dtype=F64)
    flat[idx] = wt.reshape(-1)
    return flat.view(shape)


# ------------------------------------------------------------------------------------------------ reference
@dataclass
class Expected:
    out_tensors: list            # float64, what every output tensor must hold afterwards (NaN where it started as NaN)
    stats: Optional[torch.Tensor]     # [Ncols, 2]: sum and sum of squares of the STORED values
    first: torch.Tensor          # [N, h, w, Ncols] in front of the first rounding
    acc: torch.Tensor


def reference(r: Row, ops: Operands, roundings: int, bf16: bool = True) -> Expected:
    n, h, w = r.shape
    x = torch.cat([load_view(v, h, w, bf16) for v in ops.ins], 3)
    acc = gemm_sum(x, ops.wt)
    assert bool(torch.isfinite(acc).all()), "the oracle read a poisoned element"
    res = [t.clone() for t in ops.out_tensors]
    firsts, stored_all = [], []
    c0 = 0
    for idx, v, kind in ops.outs:
        cols = slice(c0, c0 + v.width)
        c0 += v.width
        old = v._cut(ops.out_tensors[idx], h, w) if kind in ("acc", "accgate") else None
        gate = v._cut(v.gate, h, w) if v.gate is not None else None
        stored, first = epilogue(acc[..., cols], None if ops.bias is None else ops.bias[cols], r.relu, gate,
                                 kind == "accgate", old, roundings, bf16)
        assert bool(torch.isfinite(stored).all()), "the oracle read a poisoned element"
        v._cut(res[idx], h, w)[...] = stored
        firsts.append(first)
        stored_all.append(stored)
    st = torch.cat(stored_all, 3)
    stats = torch.stack([st.sum((0, 1, 2)), (st * st).sum((0, 1, 2))], 1) if r.stats else None
    return Expected(res, stats, torch.cat(firsts, 3), acc)


def exactness_margin(r: Row, ops: Operands) -> float:
    """A precondition of the data, not a tolerance: the largest conv(|X|, |W|) + |b| + |old| any accumulator or epilogue
    value of the launch can see (to stay below EXACT_LIMIT); statistics rows: also every column's sum of stored^2, scaled
    so that its limit 2^24 reads as EXACT_LIMIT; fold rows: `load_view` asserts that the fma is an fp32 number."""
    n, h, w = r.shape
    x = torch.cat([load_view(v, h, w) for v in ops.ins], 3).abs()
    m = gemm_sum(x, ops.wt.abs())
    if ops.bias is not None:
        m = m + ops.bias.abs()
    c0, worst = 0, 0.0
    for idx, v, kind in ops.outs:
        mm = m[..., c0:c0 + v.width]
        c0 += v.width
        if kind in ("acc", "accgate"):
            mm = mm + v._cut(ops.out_tensors[idx], h, w).abs()
        worst = max(worst, float(mm.max()))
    if r.stats:
        e = reference(r, ops, 2)
        worst = max(worst, float(e.stats[:, 1].max()) * EXACT_LIMIT / 2.0 ** 24, float(e.stats[:, 0].abs().max()))
    return worst


def max_terms(r: Row, ops: Operands) -> float:
    """impulse rows: the largest number of nonzero products any output element adds (must be 1: a copy)"""
    n, h, w = r.shape
    x = torch.cat([load_view(v, h, w) for v in ops.ins], 3)
    return float(gemm_sum((x != 0).to(F64), (ops.wt != 0).to(F64)).max())


# ------------------------------------------------------------------------------------------------ the launchers' choices
def _ceil(a, b):
    return -(-a // b)


def fast_geometry(r: Row):
    """gemm_units.h fast_args(kc 32, ncol 32) + gemm_bf16.hip bf16_gemm_args: tile width, patches, column tiles,
    chunks and the column tiles per unit (two when the launch takes no statistics and has an even number of them)"""
    n, h, w = r.shape
    l2, tx, ty = tile_geom(h, w)
    n_tiles = sum(_ceil(c, 32) for c in r.out_lens)
    n_chunks = sum(_ceil(c, 32) for c in r.in_lens)
    nt_unit = 2 if (not r.stats and n_tiles % 2 == 0) else 1
    aligned = all(((v[0] | v[1] | v[2]) & 7) == 0 for v in r.ins + tuple(o[:3] for o in r.outs))
    return dict(log2tw=l2, patches=n * tx * ty, tiles_x=tx, n_tiles=n_tiles, n_chunks=n_chunks, nt_unit=nt_unit, aligned=aligned)


def dma_takes(r: Row) -> bool:
    """gemm_bf16_dma.hip launch_gemm_bf16_dma under BF16_DMA_ALL=1: plain input views of whole 32-channel chunks that
    share one tensor geometry"""
    return (not r.fold and all(c % 32 == 0 for c in r.in_lens) and len({v[0] for v in r.ins}) == 1
            and fast_geometry(r)["aligned"])


def _workers(per_cu, cus):
    return max(8, (per_cu * cus) & ~7)


def launch_plan(r: Row, variant: str, cus: int) -> dict:
    """-> label, key (the instantiation: template arguments and launch constants), units, workers.
    variants: reg (BF16_NO_DMA=1), dma4 (BF16_DMA_FORM=4, BF16_DMA_ALL=1), dma8 (BF16_DMA_FORM=8, BF16_DMA_ALL=1),
    pw (default switches), small, fld; k1 rows run with PW_DIRECT=0."""
    n, h, w = r.shape
    if variant == "fld":
        return dict(label=FLD, key="%s C=%d" % (FLD, r.outs[0][2]), units=_ceil(n * h * w, 256), workers=4096)
    if variant == "small":
        c = r.ins[0][0]
        geo = fast_geometry(r)
        return dict(label=SMALL, key="%s C=%d %s" % (SMALL, c, "stats" if r.stats else "plain"), units=geo["patches"],
                    workers=min(2048, cus * (3 if c >= 3 else 4)))
    geo = fast_geometry(r)
    assert geo["aligned"], r.id
    t = r.taps
    if variant == "pw":
        p = pw_plan(r)
        if p is not None:
            waves = p["threads"] // 64
            key = "%s QC=%d NCBP=%d EPI=%d threads=%d kchunk=%d pass=%d" % (PWB, p["qc"], p["ncbp"], p["epi"], p["threads"],
                                                                         p["n_kchunk"], p["n_pass"])
            return dict(label=PWB, key=key, units=_ceil(p["n_tiles"], waves), workers=cus * (16 // waves), **p)
        variant = "dma4" if dma_takes(r) else "reg"     # the fallbacks of the default dispatch
    if variant in ("dma4", "dma8") and dma_takes(r):
        form = 8 if (variant == "dma8" and t == 9 and not r.stats and geo["log2tw"] == 5) else 4
        if form == 8:
            nt = 2 if geo["n_tiles"] % 2 == 0 else 1
            units = n * _ceil(h, 16) * geo["tiles_x"] * (geo["n_tiles"] // nt)
            resident = (geo["n_tiles"] // nt) * geo["n_chunks"] <= 4 // nt
            key = "%s waves=8 tw=32 NT=%d %s" % (DMA9, nt, "resident" if resident else "streamed")
            return dict(label=DMA9, key=key, units=units, workers=_workers(1, cus))
        nt = 1 if t == 9 else geo["nt_unit"]
        units = geo["patches"] * (geo["n_tiles"] // nt)
        rw = not (t == 1 and not r.stats and r.plain_out)
        key = "%s waves=4 tw=%d NT=%d%s %s" % (DMA9 if t == 9 else DMA1, 1 << geo["log2tw"], nt, " STATS" if r.stats else "",
                                              "rw" if rw else "plain")
        return dict(label=DMA9 if t == 9 else DMA1, key=key, units=units, workers=_workers(2 if rw else 3, cus))
    nt = geo["nt_unit"]
    key = "%s tw=%d NT=%d%s" % (REG9 if t == 9 else REG1, 1 << geo["log2tw"], nt, " STATS" if r.stats else "")
    return dict(label=REG9 if t == 9 else REG1, key=key, units=geo["patches"] * (geo["n_tiles"] // nt), workers=_workers(2, cus))


def pwb_block_count(units: int) -> int:
    if units in (1, 2, 4, 8):
        return units
    return 8 if (units > 8 and units % 8 == 0) else 0


def pw_plan(r: Row):
    """gemm_pw_bf16.hip launch_gemm_pw_bf16: None where it refuses the launch"""
    n, h, w = r.shape
    if r.taps != 1 or r.stats or w % 16 or r.fold:
        return None
    if any(c % 32 for c in r.in_lens + r.out_lens) or not fast_geometry(r)["aligned"]:
        return None
    k, nc = r.k, r.ncols
    plain = r.plain_out and not r.relu
    qc, ncbp = pwb_block_count(k // 32), pwb_block_count(nc // 32)
    if qc == 0 or ncbp == 0:
        return None
    if not plain and ncbp == 8:
        ncbp = 4
    lds = k * nc * 2 + nc * 4
    if lds > 148 * 1024:
        return None
    threads = 256 if lds <= 38 * 1024 else 512 if lds <= 78 * 1024 else 1024
    return dict(qc=qc, ncbp=ncbp, epi=0 if plain else 1, threads=threads, n_kchunk=(k // 32) // qc, n_pass=(nc // 32) // ncbp,
                tiles_x=w // 16, n_tiles=n * h * (w // 16), lds=lds)


# ------------------------------------------------------------------------------------------------ the GPU rows
ALL3, REGONLY, K1V = ("dma4", "dma8", "reg"), ("reg",), ("dma4", "reg")
G57, G1612, G2016, G2440, G3721, G3370, G4072 = (3, 5, 7), (2, 20, 12), (2, 20, 16), (1, 24, 40), (1, 37, 21), (1, 33, 70), (2, 40, 72)
G2472 = (2, 24, 72)   # 18 patches: more than the 16 workgroups of a statistics launch at 8 CUs, few enough pixels for exact sums of squares
KINDS4 = [(32, "store"), (32, "acc"), (32, "gate"), (32, "accgate")]

K9_ROWS = [
    # one chunk into one tile, every tile width, the plain / ReLU / bias / statistics epilogues
    row("k9-32-32-plain-multi", "k9", G4072, "fwd", [32], [32], variants=ALL3, multi=True),
    row("k9-32-32-relu-ties", "k9", G2440, "fwd", [32], [32], relu=True, bias=True, variants=ALL3),
    row("k9-32-32-ties-tw8", "k9", G57, "fwd", [32], [32], bias=True, variants=K1V),
    row("k9-32-32-relu-ties-tw16", "k9", G2016, "fwd", [32], [32], relu=True, bias=True, variants=K1V),
    row("k9-32-32-stats-multi", "k9", G2472, "fwd", [32], [32], stats=True, variants=ALL3, multi=True, wmax=1),
    row("k9-32-32-stats-ties-tw8", "k9", G57, "fwd", [32], [32], stats=True, bias=True, variants=K1V),
    row("k9-32-32-stats-relu-tw16", "k9", G1612, "fwd", [32], [32], stats=True, relu=True, variants=K1V),
    row("k9-32-32-stats-ragged", "k9", G3721, "fwd", [32], [32], stats=True, variants=K1V),
    # several chunks, odd and even numbers of column tiles, concatenation, slices, the resident image of the 8-wave form
    row("k9-cat192-64", "k9", G3370, "fwd", [64, 64, 64], [64], relu=True, bias=True, variants=ALL3),
    row("k9-64-96-odd-tiles", "k9", G3721, "fwd", [64], [96], bias=True, variants=ALL3),
    row("k9-64-96-stats", "k9", G57, "fwd", [64], [96], stats=True, variants=K1V, wmax=1),
    row("k9-64-64-multi", "k9", G4072, "fwd", [64], [64], relu=True, variants=ALL3, multi=True),
    row("k9-128-32-resident", "k9", G2440, "fwd", [128], [32], bias=True, variants=ALL3),
    row("k9-slices", "k9", G2016, "fwd", [(48, 8, 32)], [(72, 8, 64, "store")], bias=True, variants=K1V),
    row("k9-slices-tw32", "k9", G2440, "fwd", [(48, 16, 32)], [(72, 40, 32, "store")], relu=True, variants=ALL3),
    row("k9-partial-tw8", "k9", G57, "fwd", [16, 8, 40], [24], bias=True, variants=REGONLY),
    row("k9-partial-tw16", "k9", G2016, "fwd", [16, 8, 40], [24], relu=True, variants=K1V),   # (the LDS-DMA kernel refuses it)
    row("k9-partial-stats", "k9", G3721, "fwd", [16, 8, 40], [24], stats=True, variants=REGONLY),
    # input gradients: rotated weights, the four view kinds in one launch
    row("k9-dgrad-kinds-multi", "k9", G4072, "dgrad", [32], KINDS4, variants=ALL3, multi=True),
    row("k9-dgrad-kinds-tw8", "k9", G57, "dgrad", [32], KINDS4, bias=True, variants=K1V),
    row("k9-dgrad-kinds-tw16", "k9", G1612, "dgrad", [64], KINDS4[1:], bias=True, variants=K1V),
    row("k9-dgrad-disc", "k9", G3370, "dgrad", [64], [(64, "acc"), (32, "accgate"), (32, "gate")], bias=True, variants=ALL3),
    row("k9-dgrad-relu-sliced", "k9", G3721, "dgrad", [(40, 8, 32)], [(48, 16, 32, "accgate"), (32, "acc")], relu=True, bias=True,
        variants=ALL3),
    # fold on load (the register kernel): exact and rounding
    row("k9-fold-exact", "k9", G2440, "fwd", [32], [64], fold="exact", variants=REGONLY),
    row("k9-fold-exact-stats-multi", "k9", G2472, "fwd", [32], [32], fold="exact", stats=True, variants=REGONLY, multi=True, wmax=1),
    row("k9-fold-round", "k9", G3721, "fwd", [32, 32], [64], fold="round", bias=True, variants=REGONLY),
    row("k9-fold-round-tw8", "k9", G57, "fwd", [32], [32], fold="round", variants=REGONLY, wmax=1),
    row("k9-fold-round-tw16", "k9", G1612, "fwd", [(40, 8, 32)], [32], fold="round", variants=REGONLY),
    # impulses: shifted copies of full-mantissa tensors
    row("k9-impulse-w", "k9", G3721, "fwd", [32], [32], data="impulse_w", variants=ALL3),
    row("k9-impulse-w-64-64-tw16", "k9", G2016, "fwd", [64], [64], data="impulse_w", variants=K1V),
    row("k9-impulse-w-dgrad-acc", "k9", G2440, "dgrad", [32], [(32, "acc"), (32, "gate")], data="impulse_w", variants=ALL3),
    row("k9-impulse-x", "k9", G3721, "fwd", [32], [64], data="impulse_x", variants=ALL3),
    row("k9-impulse-x-tw8", "k9", G57, "fwd", [64], [32], data="impulse_x", variants=K1V),
]

K1_ROWS = [
    row("k1-deconv-fwd-64-32", "k1", (2, 12, 20), "deconv_fwd", [64], [32], taps=1, bias=True, variants=K1V),
    row("k1-deconv-fwd-multi", "k1", G4072, "deconv_fwd", [32], [32], taps=1, variants=K1V, multi=True),
    row("k1-deconv-fwd-sliced-tw8", "k1", G57, "deconv_fwd", [(40, 8, 32)], [(48, 8, 32, "store")], taps=1, bias=True, variants=K1V),
    row("k1-deconv-dgrad-accgate", "k1", (2, 12, 20), "deconv_dgrad", [32], [(64, "accgate")], taps=1, bias=True, variants=K1V),
    row("k1-deconv-dgrad-multi", "k1", G4072, "deconv_dgrad", [32], [(64, "accgate")], taps=1, variants=K1V, multi=True),
    row("k1-deconv-dgrad-one-tile-tw16", "k1", G1612, "deconv_dgrad", [(40, 8, 32)], [(32, "acc")], taps=1, bias=True, variants=K1V),
    row("k1-conv-64-32-one-tile-multi", "k1", G4072, "fwd", [64], [32], taps=1, bias=True, variants=K1V, multi=True),
    row("k1-conv-128-96-relu", "k1", G3721, "fwd", [64, 64], [96], taps=1, relu=True, bias=True, variants=K1V),
    row("k1-dgrad-kinds", "k1", G2440, "dgrad", [32], KINDS4, taps=1, bias=True, variants=K1V),
    row("k1-fold-exact", "k1", G2016, "fwd", [32], [64], taps=1, fold="exact", variants=REGONLY),
    row("k1-impulse-w-deconv", "k1", (2, 12, 20), "deconv_fwd", [64], [32], taps=1, data="impulse_w", variants=K1V),
    row("k1-impulse-x-deconv-dgrad", "k1", G2016, "deconv_dgrad", [32], [64], taps=1, data="impulse_x", variants=K1V),
]


def _pw_matrix():
    """every (QC, NCBP) cell at W = 16, 32, 48 with the plain and the read-modify-write epilogue; transposed-convolution
    views where the channel counts allow them (N a multiple of 128 forward, K a multiple of 128 backward)"""
    rows = []
    kinds = ("acc", "gate", "accgate")
    for qi, q in enumerate((1, 2, 4, 8)):
        for ci, c in enumerate((1, 2, 4, 8)):
            for wi, w in enumerate((16, 32, 48)):
                k, nc = 32 * q, 32 * c
                shape = (2, 3, w)
                tag = "q%d-c%d-w%d" % (q, c, w)
                if nc % 128 == 0:
                    rows.append(row("pw-plain-" + tag, "pw", shape, "deconv_fwd", [k], [nc // 4], taps=1, bias=True, variants=["pw"]))
                else:
                    rows.append(row("pw-plain-" + tag, "pw", shape, "fwd", [k], [nc], taps=1, bias=True, variants=["pw"]))
                kind = kinds[(qi + ci + wi) % 3]
                relu = (qi + wi) % 2 == 1
                if k % 128 == 0:
                    rows.append(row("pw-rmw-" + tag, "pw", shape, "deconv_dgrad", [k // 4], [(nc, kind)], taps=1, bias=True, relu=relu,
                                    variants=["pw"]))
                else:
                    outs = [(nc, kind)] if c == 1 else [(nc // 2, kind), (nc // 2, "acc")]
                    rows.append(row("pw-rmw-" + tag, "pw", shape, "dgrad", [k], outs, taps=1, bias=True, relu=relu, variants=["pw"]))
    return rows


PW_ROWS = _pw_matrix() + [
    row("pw-kchunk2-plain", "pw", (2, 3, 32), "fwd", [256, 256], [64], taps=1, bias=True, variants=["pw"]),
    row("pw-kchunk2-rmw", "pw", (2, 3, 48), "deconv_dgrad", [128], [(64, "accgate")], taps=1, bias=True, variants=["pw"]),
    row("pw-pass2-plain", "pw", (2, 3, 48), "deconv_fwd", [64], [128], taps=1, bias=True, variants=["pw"]),
    row("pw-pass4-rmw", "pw", (2, 3, 16), "dgrad", [64], [(256, "acc"), (256, "accgate")], taps=1, bias=True, variants=["pw"]),
    row("pw-relu-only", "pw", (2, 3, 32), "fwd", [64], [64], taps=1, relu=True, bias=True, variants=["pw"]),
    row("pw-multi-plain", "pw", (2, 40, 48), "deconv_fwd", [64], [32], taps=1, bias=True, variants=["pw"], multi=True),
    row("pw-multi-rmw", "pw", (2, 40, 48), "deconv_dgrad", [32], [(64, "accgate")], taps=1, bias=True, variants=["pw"], multi=True),
    row("pw-multi-1024", "pw", (5, 40, 48), "fwd", [256], [256], taps=1, variants=["pw"], multi=True),
    row("pw-impulse-w", "pw", (2, 5, 48), "deconv_fwd", [64], [32], taps=1, data="impulse_w", variants=["pw"]),
    row("pw-impulse-x-rmw", "pw", (2, 5, 32), "dgrad", [64], [(64, "acc"), (64, "gate")], taps=1, data="impulse_x", variants=["pw"]),
    # what it must refuse, with the kernel that takes the launch instead
    row("pw-refuse-k96", "pw", (2, 3, 32), "fwd", [96], [32], taps=1, bias=True, variants=["pw"]),
    row("pw-refuse-w20", "pw", (2, 3, 20), "fwd", [64], [64], taps=1, bias=True, variants=["pw"]),
    row("pw-refuse-fold", "pw", (2, 3, 32), "fwd", [64], [64], taps=1, fold="exact", variants=["pw"]),
    row("pw-refuse-lds", "pw", (1, 3, 16), "fwd", [512], [256], taps=1, variants=["pw"]),
]
PW_REFUSED = {"pw-refuse-k96": DMA1, "pw-refuse-w20": DMA1, "pw-refuse-fold": REG1, "pw-refuse-lds": DMA1}

SMALL_ROWS = [row("small-c%d-%s" % (c, "stats" if st else "plain"), "small", (3, 40, 72) if c == 1 else G4072, "fwd", [c], [32],
                  relu=(c != 3), bias=not st, stats=st, variants=["small"], multi=True if st else ["round", "ties"])
              for c in (1, 3, 4) for st in (False, True)] + [
    row("small-c3-ragged-tw8", "small", G57, "fwd", [3], [16], bias=True, stats=True, variants=["small"]),
    row("small-c2-ragged", "small", G3721, "fwd", [2], [64], bias=True, variants=["small"]),
]
FLD_ROWS = [row("fld-c%d" % c, "fld", s, "dgrad", [32 if c != 3 else 64], [c], variants=["fld"])
            for c, s in ((1, G3721), (2, G57), (3, G4072), (4, G2016))]

ROWS = K9_ROWS + K1_ROWS + PW_ROWS + SMALL_ROWS + FLD_ROWS
GRIDS = (None, 8)   # every CU of the device, and usable_cus(8)


def cells():
    """(row, variant, grid) of every GPU launch"""
    return [(r, v, g) for r in ROWS for v in r.variants for g in GRIDS]
