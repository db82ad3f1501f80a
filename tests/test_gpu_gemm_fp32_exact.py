"""The fp32 forward / input-gradient GEMM kernels on the integer rows of tests/gemm_oracle.py: every element EQUAL.

The oracle does not depend on the storage type; with fp32 storage nothing is rounded at all, so on small-integer
operands gemm_fast_kernel<9/1>, gemm_pw_kernel, gemm_pix_kernel<9/1> (ops.USE_FAST_GEMM = False, with a ReLU gate on
load), small_cin_fwd_kernel and gemm_wino_kernel (lean, and general through WINO_NO_LEAN) must reproduce the float64
sums exactly.  For the Winograd form: B^T d B of integers is integer, G g G^T a multiple of 1/4, A^T . A a sum of those,
all fp32 numbers while helpers.wino_magnitude stays below 2^22 (asserted in tests/test_gemm_oracle_host.py), so it must
equal the direct sum.  The per-element a-priori bounds of tests/test_gpu_persistent.py judge rounding on random data;
this file adds what a bound cannot: a dropped, duplicated or misplaced term fails whatever its size.
"""
import contextlib

import pytest
import torch

from tests import gemm_oracle as go
from tests.gemm_oracle import G57, G2016, G2440, G3721, G4072, KINDS4, row
from tests.helpers import usable_cus
from tests.test_gpu_gemm_bf16_exact import PAD, SENTINEL, _bits, _guarded_host, _mismatch

pytestmark = pytest.mark.gpu

WINO, FAST9, FAST1, PIX9, PIX1, PW32 = ("gemm_wino_kernel", "gemm_fast_kernel<9>", "gemm_fast_kernel<1>", "gemm_pix_kernel<9>",
                                        "gemm_pix_kernel<1>", "gemm_pw_kernel")
# variant -> (label at 9 taps, label at 1 tap, debug switches, direct, USE_FAST_GEMM)
VARIANTS = {
    "wino": (WINO, None, {}, False, True),
    "wino_general": (WINO, None, {"WINO_NO_LEAN": 1}, False, True),
    "fast": (FAST9, FAST1, {"PW_DIRECT": 0}, True, True),
    "pw": (None, PW32, {}, False, True),
    "pix": (PIX9, PIX1, {}, False, False),
    "small": (go.SMALL, None, {}, False, True),
}
W3, D3 = ("wino", "wino_general", "fast", "pix"), ("fast", "pix")

FP32_ROWS = [
    row("f9-32-48-relu-bias", "f32", G2440, "fwd", [32], [48], relu=True, bias=True, variants=W3),
    row("f9-dgrad-kinds", "f32", G3721, "dgrad", [32], KINDS4, variants=W3),
    row("f9-dgrad-kinds-multi", "f32", G4072, "dgrad", [32], KINDS4[1:], variants=("wino", "fast"), multi=True),
    row("f9-slices-stats-tw16", "f32", G2016, "fwd", [(48, 8, 32)], [(72, 8, 64, "store")], stats=True, variants=W3, wmax=1),
    row("f9-cat-fold-stats-tw8", "f32", G57, "fwd", [16, 8], [24], fold="exact", stats=True, variants=W3, wmax=1),
    row("f9-cat-64-multi", "f32", G4072, "fwd", [32, 32], [64], bias=True, variants=W3, multi=True),
    row("f9-gate-on-load", "f32", G3721, "fwd", [12, 20], [20], bias=True, variants=("pix",)),
    row("f9-impulse-w", "f32", G3721, "fwd", [32], [32], data="impulse_w", variants=D3),
    row("f9-impulse-x", "f32", G2016, "fwd", [32], [64], data="impulse_x", variants=D3),
    row("f1-deconv-fwd-w20", "f32", (2, 12, 20), "deconv_fwd", [64], [32], taps=1, bias=True, variants=D3),
    row("f1-deconv-dgrad-w20", "f32", (2, 12, 20), "deconv_dgrad", [32], [(64, "accgate")], taps=1, variants=D3),
    row("f1-pw-64-64-w48", "f32", (2, 5, 48), "fwd", [64], [64], taps=1, relu=True, bias=True, variants=("pw", "fast", "pix")),
    row("f1-pw-deconv-fwd-w32", "f32", (2, 5, 32), "deconv_fwd", [64], [32], taps=1, bias=True, variants=("pw", "fast", "pix")),
    row("f1-pw-deconv-dgrad-w16", "f32", (2, 40, 16), "deconv_dgrad", [32], [(64, "accgate")], taps=1, variants=("pw", "fast", "pix")),
    row("f1-gate-on-load", "f32", G2440, "fwd", [12], [20], taps=1, variants=("pix",)),
    row("f1-impulse-w-pw", "f32", (2, 5, 32), "fwd", [64], [64], taps=1, data="impulse_w", variants=("pw", "fast", "pix")),
    row("small-f32-c3-stats", "f32", G3721, "fwd", [3], [32], relu=True, stats=True, variants=("small",)),
    row("small-f32-c1-bias", "f32", G57, "fwd", [1], [16], bias=True, variants=("small",)),
]
GATED_ON_LOAD = ("f9-gate-on-load", "f1-gate-on-load")
CELLS = [(r, v, g) for r in FP32_ROWS for v in r.variants for g in ((None, 8) if r.multi else (None,))]
SEEN = {}


def fp32_operands(r):
    """gemm_oracle.operands, with a ReLU gate (real zeros and negatives) on the first input view of the gated rows"""
    ops = go.operands(r)
    if r.id in GATED_ON_LOAD:
        v = ops.ins[0]
        g = go._gen(r, "gate-on-load")
        v.gate = go._poison(go._ints(g, tuple(v.t.shape), -2, 2, 0.0), v.c_off, v.width)
    return ops


def label_of(r, variant):
    return VARIANTS[variant][0 if r.taps == 9 else 1]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_REF = {}


def _case(r):
    if r.id not in _REF:
        ops = fp32_operands(r)
        _REF[r.id] = (ops, go.reference(r, ops, 1, bf16=False))
    return _REF[r.id]


def _cell_id(cell):
    r, variant, grid = cell
    return "%s-%s-%s" % (r.id, variant, "full" if grid is None else "cus%d" % grid)


@pytest.mark.parametrize("cell", CELLS, ids=[_cell_id(c) for c in CELLS])
def test_every_element_equals_the_oracle(dev, cell):
    from unet_nested4tiny_objects_keypoints_amd import _lib, engine
    from unet_nested4tiny_objects_keypoints_amd import ops as lib_ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    r, variant, grid = cell
    label, switches, direct, use_fast = label_of(r, variant), VARIANTS[variant][2], VARIANTS[variant][3], VARIANTS[variant][4]
    ops, want = _case(r)
    n, h, w = r.shape
    cache = {}

    def put(t):
        if t is None:
            return None
        if id(t) not in cache:
            cache[id(t)] = t.float().to(dev).contiguous()
        return cache[id(t)]
    ins = [V(put(v.t), v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, scale=put(v.scale), shift=put(v.shift), gate=put(v.gate),
             relu=v.relu) for v in ops.ins]
    bufs = [_guarded_host(t, torch.float32).to(dev) for t in ops.out_tensors]
    tensors = [b[PAD:PAD + t.numel()].view(t.shape) for b, t in zip(bufs, ops.out_tensors)]
    outs = [V(tensors[idx], v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, gate=put(v.gate), relu=r.relu,
              accumulate=kind in ("acc", "accgate"), gate_sum=kind == "accgate") for idx, v, kind in ops.outs]
    pack = {"fwd": engine.pack_conv_fwd, "dgrad": engine.pack_conv_dgrad, "deconv_fwd": engine.pack_deconv_fwd,
            "deconv_dgrad": engine.pack_deconv_dgrad}[r.form]
    bias = None
    if ops.bias is not None:
        bias = engine.tile_bias4(put(ops.bias_param)) if r.form == "deconv_fwd" else put(ops.bias_param)
    blocks = go.fast_geometry(r)["patches"]
    stats = None
    if r.stats:
        stats = torch.full((blocks * r.ncols * 2 + 2 * PAD,), SENTINEL, device=dev)
        stats[PAD:-PAD] = float("nan")
    was = lib_ops.USE_FAST_GEMM
    with contextlib.ExitStack() as stack:
        stack.enter_context(usable_cus(grid))
        for name, value in switches.items():
            stack.enter_context(_lib.debug_switch(name, value))
        lib_ops.USE_FAST_GEMM = use_fast
        try:
            lib_ops.gemm_fwd(n, h, w, r.taps, ins, outs, pack(put(ops.weight)), bias, None if stats is None else stats[PAD:-PAD],
                             direct=direct)
        finally:
            lib_ops.USE_FAST_GEMM = was
        torch.cuda.synchronize()
        ran = _lib.lib().unetpp_last_kernel_name().decode()
    what = "%s %s" % (_cell_id(cell), ran)
    assert ran == label, (what, label)
    for i, (buf, exp) in enumerate(zip(bufs, want.out_tensors)):
        got, exp_buf = buf.cpu(), _guarded_host(exp, torch.float32)
        assert torch.equal(_bits(got), _bits(exp_buf)), "%s output %d: %s" % (what, i, _mismatch(got, exp_buf))
    if r.stats:
        s = stats.cpu()
        assert bool((s[:PAD] == SENTINEL).all()) and bool((s[-PAD:] == SENTINEL).all()), what
        rows = s[PAD:-PAD].view(blocks, r.ncols, 2).double()
        assert not bool(torch.isnan(rows).any()), what + ": rows of partial sums left unwritten"
        assert torch.equal(rows.sum(0), want.stats), what + ": partial sums"
    key = variant if variant.startswith("wino") else ran
    SEEN[key] = SEEN.get(key, 0) + 1


def test_every_fp32_label_ran(dev):
    """(after the cases of this module)"""
    for key in ("wino", "wino_general", FAST9, FAST1, PIX9, PIX1, PW32, go.SMALL):
        assert SEEN.get(key, 0) > 0, key
    print("ran:", SEEN)
