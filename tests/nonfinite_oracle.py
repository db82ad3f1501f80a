"""Non-finite values in the layer kernels: the float64 references with torch's semantics (relu and max_pool2d carry a
NaN), the footprints, and the plant list of tests/test_gpu_nonfinite.py.

For one launch with ONE planted value:

    R   the reference's non-finite output elements (float64, tests/gemm_oracle.py's sum without its finite-only guards)
    F   the output elements whose computation reads the planted element in the kernel as written: the 3x3 (1x1)
        neighbourhood for the direct and pointwise forms, every output of each 2x2 tile whose 4x4 input tile holds the
        pixel for Winograd F(2x2,3x3), the whole output column for a weight or bias element, everything for a scale /
        shift coefficient of an input channel

    rule 1 (containment)    outside F the launch with the plant stores the bits of the launch without it
    rule 2 (no laundering)  every element of R is non-finite in the kernel's output (a NaN where the reference has an
                            inf is fine: 0 * inf in a sum, inf - inf in the Winograd input transform)

tests/test_nonfinite_host.py holds R and F of every plant against each other on the CPU (R never empty, R inside F,
at least half of the output outside F for activation plants), so that the GPU cells cannot pass emptily.
"""
import copy
import struct
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from tests import gemm_oracle as go
from tests.gemm_oracle import G57, G2016, G4072, KINDS4, row
from tests.wgrad_oracle import F64, tile_geom

# ------------------------------------------------------------------------------------------------ planted values
# fp32 bit patterns: quiet NaN, all-ones positive and negative NaN, the smallest signalling NaN, the infinities
VALUES = {"qnan": 0x7FC00000, "nan7f": 0x7FFFFFFF, "nanff": 0xFFFFFFFF, "snan": 0x7F800001, "+inf": 0x7F800000,
          "-inf": 0xFF800000}
NANS = ("qnan", "nan7f", "nanff", "snan")
BF16_VALUES = {"qnan": 0x7FC0, "+inf": 0x7F80, "-inf": 0xFF80}   # what a bf16 tensor can hold in memory


def as_float(name: str) -> float:
    """the planted value as the oracle sees it (a NaN's sign and payload mean nothing to it)"""
    return struct.unpack("<f", struct.pack("<I", VALUES[name]))[0]


def signed32(bits: int) -> int:
    return bits - (1 << 32) if bits >= (1 << 31) else bits


def signed16(bits: int) -> int:
    return bits - (1 << 16) if bits >= (1 << 15) else bits


def relu_keep_nan(v: torch.Tensor) -> torch.Tensor:
    """csrc/common.h relu_keep_nan: !(v <= 0) ? v : +0 (torch.relu's values)"""
    return torch.where(~(v <= 0), v, torch.zeros_like(v))


# ------------------------------------------------------------------------------------------------ footprints (pixels)
def footprint_direct(shape, taps: int, pos) -> torch.Tensor:
    """bool [n, h, w]: the output pixels whose 3x3 (taps 9) or 1x1 window holds input pixel pos = (image, y, x)"""
    n, h, w = shape
    b, y, x = pos
    m = torch.zeros(n, h, w, dtype=torch.bool)
    r = 1 if taps == 9 else 0
    m[b, max(0, y - r):min(h, y + r + 1), max(0, x - r):min(w, x + r + 1)] = True
    return m


def footprint_wino(shape, pos) -> torch.Tensor:
    """bool [n, h, w]: Winograd F(2x2,3x3).  Output tile (ty, tx) covers rows 2 ty, 2 ty + 1 and reads input rows
    2 ty - 1 .. 2 ty + 2 (columns alike); tiles start at even coordinates of the image in the lean and in the general
    instantiation (the 256-pixel patches have even origins and even sides).  The input transform mixes the whole 4x4
    tile, so every output of a tile that holds the pixel reads it; outputs of a ragged last tile past the image do not
    exist."""
    n, h, w = shape
    b, y, x = pos
    m = torch.zeros(n, h, w, dtype=torch.bool)
    for ty in range((h + 1) // 2):
        if not 2 * ty - 1 <= y <= 2 * ty + 2:
            continue
        for tx in range((w + 1) // 2):
            if 2 * tx - 1 <= x <= 2 * tx + 2:
                m[b, 2 * ty:min(h, 2 * ty + 2), 2 * tx:min(w, 2 * tx + 2)] = True
    return m


def patches_of(shape, pix: torch.Tensor) -> torch.Tensor:
    """bool [patches]: the 256-pixel patches (rows of BatchNorm partial sums, image-major, then rows of patches) that
    hold a pixel of `pix`"""
    n, h, w = shape
    l2, tx, ty = tile_geom(h, w)
    tw, th = 1 << l2, 256 >> l2
    out = torch.zeros(n, ty, tx, dtype=torch.bool)
    for b, y, x in pix.nonzero().tolist():
        out[b, y // th, x // tw] = True
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------ plants
@dataclass(frozen=True)
class Plant:
    """where: x (element (image, y, x, channel) of input tensor `view`; for deconv_dgrad the tensor at twice the
    resolution), x_off (the same in a channel outside the view's slice: nothing may change), gate_off (an x element whose
    on-load gate is closed: nothing may change), weight (element `at` of the parameter in its torch layout), bias (column
    or channel `at`), scale / shift (coefficient `at` of input view 0)."""
    where: str
    value: str
    at: Tuple[int, ...]
    view: int = 0
    tag: str = ""

    @property
    def id(self):
        return "%s%s-%s" % (self.where, ("-" + self.tag) if self.tag else "", self.value)


def planted(r: go.Row, ops: go.Operands, p: Plant) -> go.Operands:
    """a copy of the operands with the value planted (float64: the oracle's view of it)"""
    o = copy.deepcopy(ops)
    v = as_float(p.value)
    if p.where in ("x", "x_off", "gate_off"):
        # deconv_dgrad: the four phase views share one tensor object in `ops` and must again after the copy
        t = o.ins[p.view].t
        for w_ in o.ins:
            if w_.t is not t and r.form == "deconv_dgrad":
                w_.t = t
        t[p.at] = v
    elif p.where == "weight":
        o.weight[p.at] = v
        o.wt = go.WEIGHT_FORMS[r.form](o.weight).contiguous()
    elif p.where == "bias":
        o.bias_param[p.at] = v
        o.bias = o.bias_param.repeat(4) if r.form == "deconv_fwd" else o.bias_param
    elif p.where == "scale":
        o.ins[0].scale[p.at] = v
    elif p.where == "shift":
        o.ins[0].shift[p.at] = v
    else:
        raise ValueError(p.where)
    return o


def reference(r: go.Row, ops: go.Operands, bf16: bool, roundings: int = 1):
    """gemm_oracle.reference without its finite-only guards and with a ReLU that carries NaN (clamp_min does).
    -> (output tensors float64, stats [Ncols, 2] or None)"""
    n, h, w = r.shape
    x = torch.cat([go.load_view(v, h, w, bf16) for v in ops.ins], 3)
    acc = go.gemm_sum(x, ops.wt)
    res = [t.clone() for t in ops.out_tensors]
    stored_all, c0 = [], 0
    for idx, v, kind in ops.outs:
        cols = slice(c0, c0 + v.width)
        c0 += v.width
        old = v._cut(ops.out_tensors[idx], h, w) if kind in ("acc", "accgate") else None
        gate = v._cut(v.gate, h, w) if v.gate is not None else None
        stored, _ = go.epilogue(acc[..., cols], None if ops.bias is None else ops.bias[cols], r.relu, gate, kind == "accgate",
                                old, roundings, bf16 and bool(torch.isfinite(acc).all()))   # (bf() is stated for finite sums)
        v._cut(res[idx], h, w)[...] = stored
        stored_all.append(stored)
    st = torch.cat(stored_all, 3)
    stats = torch.stack([st.sum((0, 1, 2)), (st * st).sum((0, 1, 2))], 1) if r.stats else None
    return res, stats


def wino_variant(variant: str) -> bool:
    return variant.startswith("wino")


def footprint(r: go.Row, ops: go.Operands, p: Plant, variant: str):
    """-> (bool mask per output tensor, bool [patches, Ncols] of the BatchNorm partial rows, share of the launch's output
    elements outside F)"""
    n, h, w = r.shape
    col = torch.zeros(r.ncols, dtype=torch.bool)
    if p.where in ("x_off", "gate_off"):
        pix = torch.zeros(n, h, w, dtype=torch.bool)
    elif p.where == "x":
        b, y, x = p.at[:3]
        if r.form == "deconv_dgrad":
            y, x = y // 2, x // 2          # the four phases of GEMM pixel (y // 2, x // 2)
        pix = footprint_wino(r.shape, (b, y, x)) if wino_variant(variant) else footprint_direct(r.shape, r.taps, (b, y, x))
        col[:] = True
    else:
        pix = torch.ones(n, h, w, dtype=torch.bool)
        if p.where == "weight":
            probe = torch.zeros(ops.weight.shape, dtype=F64)
            probe[p.at] = 1.0
            col = go.WEIGHT_FORMS[r.form](probe).reshape(-1, r.ncols).sum(0) > 0
        elif p.where == "bias":
            probe = torch.zeros(ops.bias_param.shape, dtype=F64)
            probe[p.at] = 1.0
            col = (probe.repeat(4) if r.form == "deconv_fwd" else probe) > 0
        else:
            col[:] = True
    masks = [torch.zeros(t.shape, dtype=torch.bool) for t in ops.out_tensors]
    c0 = 0
    for idx, v, _ in ops.outs:
        v._cut(masks[idx], h, w)[...] = pix[..., None] & col[c0:c0 + v.width]
        c0 += v.width
    rows = patches_of(r.shape, pix)[:, None] & col[None, :]
    inside = float((pix[..., None] & col).sum())
    return masks, rows, 1.0 - inside / float(n * h * w * r.ncols)


# ------------------------------------------------------------------------------------------------ the GEMM cases
GATED, GATED1 = "nf-gate-on-load", "nf-f1-gate-on-load-stats"
GATED_ROWS = (GATED, GATED1)
F32_VARIANTS = ("wino", "wino_general", "fast", "pix")
PWV = ("pw", "fast", "pix")

F32_ROWS = [
    row("nf-f9-relu-bias-tw16", "f32", G2016, "fwd", [32], [64], relu=True, bias=True, variants=F32_VARIANTS),
    row("nf-f9-slices-stats-tw16", "f32", G2016, "fwd", [(48, 8, 32)], [(72, 8, 64, "store")], stats=True, variants=F32_VARIANTS,
        wmax=1),
    row("nf-f9-cat-fold-stats-tw8", "f32", G57, "fwd", [16, 8], [24], fold="exact", stats=True, variants=F32_VARIANTS, wmax=1),
    row("nf-f9-dgrad-kinds-tw16", "f32", G2016, "dgrad", [32], KINDS4, variants=("wino", "fast", "pix")),
    row("nf-f9-multi-relu", "f32", G4072, "fwd", [32], [64], relu=True, variants=("wino", "fast"), multi=True),
    # A ReLU gate on LOAD exists in gemm_pix_kernel only: fast_args refuses a gated input view ("ReLU gates on load go
    # through the generic kernel", csrc/gemm_units.h), gemm_pw / gemm_pw_bf16 take plain input views, no bf16 kernel has one.
    row(GATED, "f32", G57, "fwd", [12, 20], [20], bias=True, variants=("pix",)),
    row(GATED1, "f32", (2, 5, 16), "fwd", [12], [20], taps=1, stats=True, variants=("pix",)),
    # pointwise launches with a fold on load and statistics: gemm_pw_kernel refuses both (plain input views, no statistics
    # epilogue; csrc/gemm_pw.hip gemm_pw_applies), so such a launch is gemm_fast_kernel<1>'s or gemm_pix_kernel<1>'s
    row("nf-f1-fold-stats-w48", "f32", (2, 5, 48), "fwd", [64], [64], taps=1, fold="exact", stats=True, variants=("fast", "pix"),
        wmax=1),
    row("nf-f1-pw-relu-w48", "f32", (2, 5, 48), "fwd", [64], [64], taps=1, relu=True, bias=True, variants=PWV),
    row("nf-f1-deconv-fwd-w32", "f32", (2, 5, 32), "deconv_fwd", [64], [32], taps=1, bias=True, variants=PWV),
    row("nf-f1-deconv-dgrad-w16", "f32", (2, 12, 16), "deconv_dgrad", [32], [(64, "accgate")], taps=1, variants=PWV),
    row("nf-small-c1-relu-bias", "f32", G57, "fwd", [1], [16], relu=True, bias=True, variants=("small",)),
    row("nf-small-c3-relu-stats", "f32", G2016, "fwd", [3], [32], relu=True, stats=True, variants=("small",)),   # (fp32 C = 4
    # is 4-aligned and takes an MFMA kernel; the bf16 rows below run small_cin_fwd_kernel with C = 4)
]
BF16_ROWS = [
    row("nf-k9-relu-bias-tw16", "k9", G2016, "fwd", [32], [32], relu=True, bias=True, variants=("dma4", "reg")),
    row("nf-k9-stats-tw8", "k9", G57, "fwd", [32], [32], stats=True, variants=("dma4", "reg"), wmax=1),
    row("nf-k9-fold-stats-tw16", "k9", G2016, "fwd", [32], [32], fold="exact", stats=True, variants=("reg",), wmax=1),
    row("nf-k9-multi-relu", "k9", G4072, "fwd", [32], [32], relu=True, variants=("dma4", "dma8", "reg"), multi=True),
    row("nf-k1-deconv-dgrad-accgate", "k1", (2, 12, 20), "deconv_dgrad", [32], [(64, "accgate")], taps=1, variants=("dma4", "reg")),
    # fold on load, bf16: the register kernels only (the LDS-DMA forms and gemm_pw_bf16_kernel take plain input views)
    row("nf-k1-fold-stats", "k1", G2016, "fwd", [32], [64], taps=1, fold="exact", stats=True, variants=("reg",), wmax=1),
    row("nf-k1-deconv-fwd", "k1", (2, 12, 20), "deconv_fwd", [64], [32], taps=1, bias=True, variants=("dma4", "reg")),
    row("nf-pwb-relu-w32", "pw", (2, 3, 32), "fwd", [64], [64], taps=1, relu=True, bias=True, variants=("pw",)),
    row("nf-pwb-rmw-w16", "pw", (2, 3, 16), "dgrad", [64], [(32, "accgate"), (32, "acc")], taps=1, relu=True, variants=("pw",)),
    row("nf-small-bf16-c1", "small", G57, "fwd", [1], [16], relu=True, bias=True, variants=("small",)),
    row("nf-small-bf16-c4-stats", "small", G2016, "fwd", [4], [32], relu=True, stats=True, variants=("small",)),
    row("nf-fld-c2", "fld", G57, "dgrad", [32], [2], variants=("fld",)),
]
ROWS = F32_ROWS + BF16_ROWS


def is_bf16(r: go.Row) -> bool:
    return r.family != "f32"


def operands(r: go.Row) -> go.Operands:
    """gemm_oracle.operands; the gated row gets a ReLU gate (real zeros and negatives) on its first input view"""
    ops = go.operands(r)
    if r.id in GATED_ROWS:
        v = ops.ins[0]
        g = go._gen(r, "gate-on-load")
        v.gate = go._poison(go._ints(g, tuple(v.t.shape), -2, 2, 0.0), v.c_off, v.width)
    return ops


def _channel_with(vec, pred, what):
    for i, s in enumerate(vec.tolist()):
        if pred(s):
            return i
    raise AssertionError("no channel with " + what)


def plants(r: go.Row, ops: go.Operands):
    """The plants of a row, one position each: an interior pixel, the image corner (0, 0), the last pixel of the ragged
    last tile (the last pixel of the last image: no geometry here is a whole number of patches), a pixel of a later unit
    of a persistent workgroup (multi rows, under usable_cus(8)), channels just inside and just outside a slice, an input
    whose gate is closed, one weight, one bias element, one scale and one shift coefficient.  The six values go round
    over the activation plants; bf16 tensors take the values a bf16 tensor can hold, and the four fp32 NaN patterns then
    arrive through the fp32 bias / scale / shift (the bf16 store paths must keep them NaN)."""
    n, h, w = r.shape
    bf = is_bf16(r) and r.family not in ("small",)      # (the 1..4-channel network input stays fp32)
    names = list(BF16_VALUES) if bf else list(VALUES)
    big = 2 if r.form == "deconv_dgrad" else 1            # the x tensor of a deconv_dgrad is at twice the resolution
    _, c_off, c_len = r.ins[0]
    out = []
    fold_scale = ops.ins[0].scale

    def chan(k, value):
        """a slice channel through which `value` reaches the sum: under a fold, one whose scale keeps it above the ReLU"""
        if fold_scale is None:
            return c_off + k % c_len
        if value == "-inf":
            return c_off + _channel_with(fold_scale, lambda s: s < 0, "a negative scale")
        return c_off + _channel_with(fold_scale, lambda s: s > 0, "a positive scale")

    def open_at(at):
        """gated rows: along the image row to an element of view 0 whose gate is open"""
        if r.id not in GATED_ROWS or bool(ops.ins[0].gate[at] > 0):
            return at
        return next((at[0], at[1], xx, at[3]) for xx in range(w) if bool(ops.ins[0].gate[at[0], at[1], xx, at[3]] > 0))

    spots = [("interior", (n - 1, (h * big) // 2, (w * big) // 2)), ("corner", (0, 0, 0)),
             ("last", (n - 1, h * big - 1, w * big - 1))]
    if r.multi:
        spots.append(("unit2", (1, 10, 70)))              # patch 20 of 30 (G4072): a later unit whatever the walk
    for i, (tag, (b, y, x)) in enumerate(spots):
        value = names[i % len(names)]
        out.append(Plant("x", value, open_at((b, y, x, chan(i, value))), 0, tag))
    # the remaining values, at the interior pixel of the LAST input view (a second view where the row concatenates)
    last_view = len(r.ins) - 1
    _, c_off2, c_len2 = r.ins[last_view]
    for j, value in enumerate(names[len(spots) % len(names):] if len(names) > len(spots) else []):
        ch = c_off2 + (c_len2 - 1 - j) % c_len2
        if last_view == 0 and fold_scale is not None:
            ch = chan(j, value)
        at = (0, (h * big) // 2, 1, ch)
        out.append(Plant("x", value, open_at(at) if last_view == 0 else at, last_view, "v%d" % last_view))
    if c_off > 0:                                          # sliced: just inside (first channel), just outside on both sides
        out.append(Plant("x", names[0], (0, 1, 1, c_off), 0, "slice-first"))
        out.append(Plant("x", names[0], (0, 2, 2, c_off + c_len - 1), 0, "slice-last"))
        out.append(Plant("x_off", "+inf", (0, 1, 1, c_off - 1), 0, "below"))
        out.append(Plant("x_off", "+inf", (0, 1, 1, c_off + c_len), 0, "above"))
    if r.id in GATED_ROWS:
        g = ops.ins[0].gate
        closed = [(b, y, x, c_off) for b in range(n) for y in range(h) for x in range(w) if not bool(g[b, y, x, c_off] > 0)]
        out.append(Plant("gate_off", "qnan", closed[len(closed) // 2], 0))
    if r.family != "fld":
        wshape = tuple(ops.weight.shape)
        for j, value in enumerate(("qnan", "+inf")):
            out.append(Plant("weight", value, tuple((s - 1 - j) % s for s in wshape), 0, "w%d" % j))
    if r.bias:
        nb = ops.bias_param.numel()
        for j, value in enumerate(NANS):
            out.append(Plant("bias", value, ((3 + 5 * j) % nb,), 0, "b%d" % j))
    if fold_scale is not None:
        for j, value in enumerate(NANS):
            out.append(Plant("scale" if j % 2 == 0 else "shift", value, ((1 + 3 * j) % c_len,), 0, "c%d" % j))
    return out


# ------------------------------------------------------------------------------------------------ 2x2 max-pool
def pool_reference(act: torch.Tensor):
    """act [N, H, W, C] float64 -> (pooled [N, H/2, W/2, C], winner 2 iy + ix as int64).  The first maximum wins in scan
    order (0,0),(0,1),(1,0),(1,1); a NaN takes the window and the last NaN keeps it (csrc/common.h pool_takes:
    t > best || t != t) -- the values of torch.max_pool2d, which carries NaN."""
    n, h, w, c = act.shape
    cand = torch.stack([act[:, iy::2, ix::2] for iy in (0, 1) for ix in (0, 1)])   # [4, N, H/2, W/2, C]
    best, idx = cand[0].clone(), torch.zeros(cand[0].shape, dtype=torch.int64)
    for q in range(1, 4):
        take = (cand[q] > best) | torch.isnan(cand[q])
        best = torch.where(take, cand[q], best)
        idx = torch.where(take, torch.full_like(idx, q), idx)
    return best, idx
