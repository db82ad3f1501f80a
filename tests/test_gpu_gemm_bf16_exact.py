"""The bf16 forward / input-gradient GEMM family, every stored bit, against tests/gemm_oracle.py.

On small-integer operands every product and every fp32 partial sum of these kernels is exact in any order (the margin
of every row is asserted below 2^22 in tests/test_gemm_oracle_host.py), so the only inexact steps are the roundings to
bf16, each a round-to-nearest-even of an exactly known fp32 number: the stored tensors must EQUAL the oracle's, ties
included, and so must the BatchNorm partial sums (sums of the stored values).  Impulse rows turn the output into a
shifted copy of a full-mantissa bf16 tensor (a copy of the weights around an impulse pixel): equality again.

Every case: output tensors start as NaN outside the accumulated slices and sit between sentinels, gates and inputs are
NaN outside their channel slices; the launch runs with the switches of its variant (gemm_oracle.launch_plan) at the full
grid and under usable_cus(8); the label that ran is asserted against the host restatement of the launchers, and the
label decides the rounding rule the oracle applies (gemm_oracle.ROUNDINGS: two roundings for gemm_bf16_kernel /
gemm_bf16_dma_kernel, one for gemm_pw_bf16_kernel).  The last test asserts that every instantiation key of the
restatement ran and prints the table (pytest -s).
"""
import contextlib

import pytest
import torch

from tests import gemm_oracle as go
from tests.helpers import usable_cus

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PAD = 64            # sentinel elements on both sides of every output tensor (128 bytes of bf16: the alignment is kept)
SENTINEL = -776.0   # a bf16 number
SEEN = {}           # instantiation key -> launches that passed
CELLS = go.cells()

SWITCHES = {
    "reg": {"BF16_NO_DMA": 1},
    "dma4": {"BF16_DMA_FORM": 4, "BF16_DMA_ALL": 1},
    "dma8": {"BF16_DMA_FORM": 8, "BF16_DMA_ALL": 1},
    "pw": {}, "small": {}, "fld": {},
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cell_id(cell):
    r, variant, grid = cell
    return "%s-%s-%s" % (r.id, variant, "full" if grid is None else "cus%d" % grid)


_OPS, _REF = {}, {}


def _operands(r):
    if r.id not in _OPS:
        _OPS[r.id] = go.operands(r)
    return _OPS[r.id]


def _reference(r, roundings, bf16):
    """the oracle's result of a row under a rounding rule, computed once and left unchanged"""
    key = (r.id, roundings, bf16)
    if key not in _REF:
        _REF[key] = go.reference(r, _operands(r), roundings, bf16)
    return _REF[key]


def _guarded_host(t64, dtype):
    """flat host buffer: sentinels, the tensor in `dtype`, sentinels"""
    buf = torch.full((t64.numel() + 2 * PAD,), SENTINEL, dtype=dtype)
    buf[PAD:PAD + t64.numel()] = t64.reshape(-1).to(dtype)
    return buf


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _mismatch(got, want):
    bad = (_bits(got) != _bits(want)).nonzero().flatten()
    i = int(bad[0])
    return "%d of %d elements differ (sentinels included), first at %d: got %r want %r" % (
        bad.numel(), want.numel(), i - PAD, float(got[i]), float(want[i]))


class _Launch:
    """device operands of a row: fresh output buffers per launch, inputs / gates / weights shared"""

    def __init__(self, r, dev):
        from unet_nested4tiny_objects_keypoints_amd import engine
        from unet_nested4tiny_objects_keypoints_amd.ops import V
        self.r, self.dev = r, dev
        ops = self.ops = _operands(r)
        self.act = torch.float32 if r.family == "fld" else BF          # storage type of the outputs
        in_dt = torch.float32 if r.family == "small" else BF           # (the 1..4-channel network input stays fp32)
        cache = {}

        def put(t, dt):
            if id(t) not in cache:
                cache[id(t)] = t.to(dt).to(dev).contiguous()
            return cache[id(t)]

        def f32(t):
            return None if t is None else t.float().to(dev)
        self.in_views = [V(put(v.t, in_dt), v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, scale=f32(v.scale), shift=f32(v.shift),
                           relu=v.relu) for v in ops.ins]
        self.gates = [None if v.gate is None else put(v.gate, BF) for _, v, _ in ops.outs]
        self.weight_param = ops.weight.float().to(dev)
        pack = {"fwd": engine.pack_conv_fwd, "dgrad": engine.pack_conv_dgrad, "deconv_fwd": engine.pack_deconv_fwd,
                "deconv_dgrad": engine.pack_deconv_dgrad}[r.form]
        self.weight = pack(self.weight_param)
        self.bias = None
        if ops.bias is not None:
            b = ops.bias_param.float().to(dev)
            self.bias = engine.tile_bias4(b) if r.form == "deconv_fwd" else b
        self.blocks = go.fast_geometry(r)["patches"]

    def run(self):
        """-> (output buffers with their sentinels, statistics buffer or None)"""
        from unet_nested4tiny_objects_keypoints_amd import ops as lib_ops
        from unet_nested4tiny_objects_keypoints_amd.ops import V
        r, ops = self.r, self.ops
        n, h, w = r.shape
        bufs = [_guarded_host(t, self.act).to(self.dev) for t in ops.out_tensors]
        tensors = [b[PAD:PAD + t.numel()].view(t.shape) for b, t in zip(bufs, ops.out_tensors)]
        if r.family == "fld":
            lib_ops.first_layer_dgrad_bf16(self.in_views[0].t, self.weight_param, tensors[0])
            return bufs, None
        out_views = [V(tensors[idx], v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, gate=self.gates[i], relu=r.relu,
                       accumulate=kind in ("acc", "accgate"), gate_sum=kind == "accgate")
                     for i, (idx, v, kind) in enumerate(ops.outs)]
        stats = None
        if r.stats:
            stats = torch.full((self.blocks * r.ncols * 2 + 2 * PAD,), SENTINEL, device=self.dev)
            stats[PAD:-PAD] = float("nan")
        lib_ops.gemm_fwd(n, h, w, r.taps, self.in_views, out_views, self.weight, self.bias,
                         None if stats is None else stats[PAD:-PAD])
        return bufs, stats


_LAUNCH = {}


def _launch(r, dev):
    if r.id not in _LAUNCH:
        _LAUNCH.clear()      # (one row's device operands at a time)
        _LAUNCH[r.id] = _Launch(r, dev)
    return _LAUNCH[r.id]


@pytest.mark.parametrize("cell", CELLS, ids=[_cell_id(c) for c in CELLS])
def test_every_stored_bit_equals_the_oracle(dev, cell):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    r, variant, grid = cell
    launch = _launch(r, dev)
    with contextlib.ExitStack() as stack:
        u = stack.enter_context(usable_cus(grid))
        for name, value in SWITCHES[variant].items():
            stack.enter_context(_lib.debug_switch(name, value))
        if r.family == "k1":
            stack.enter_context(_lib.debug_switch("PW_DIRECT", 0))
        plan = go.launch_plan(r, variant, u.cus)
        bufs, stats = launch.run()
        torch.cuda.synchronize()
        ran = _lib.lib().unetpp_last_kernel_name().decode()
    what = "%s [%s] %s" % (_cell_id(cell), plan["key"], ran)
    if r.family != "fld":      # (the first layer's input gradient has an entry point of its own and leaves no label)
        assert ran == plan["label"], what
    if grid is not None and r.multi:
        assert plan["units"] > plan["workers"], what
    want = _reference(r, go.ROUNDINGS.get(plan["label"], 1), r.family != "fld")
    for i, (buf, exp) in enumerate(zip(bufs, want.out_tensors)):
        got, exp_buf = buf.cpu(), _guarded_host(exp, launch.act)
        assert torch.equal(_bits(got), _bits(exp_buf)), "%s output %d: %s" % (what, i, _mismatch(got, exp_buf))
    if r.stats:
        s = stats.cpu()
        assert bool((s[:PAD] == SENTINEL).all()) and bool((s[-PAD:] == SENTINEL).all()), what + ": a sentinel of the sums was overwritten"
        rows = s[PAD:-PAD].view(launch.blocks, r.ncols, 2).double()
        assert not bool(torch.isnan(rows).any()), what + ": rows of partial sums left unwritten"
        tot = rows.sum(0)
        assert torch.equal(tot, want.stats), "%s sums: %d of %d differ, e.g. got %r want %r" % (
            what, int((tot != want.stats).sum()), tot.numel(), tot[tot != want.stats][:2].tolist(),
            want.stats[tot != want.stats][:2].tolist())
    SEEN[plan["key"]] = SEEN.get(plan["key"], 0) + 1


def test_every_label_and_instantiation_ran(dev):
    """Runs after the cases of this module: every instantiation key the host restatement gives for the rows (and with
    them every label of the family) passed; prints the table (pytest -s)."""
    with usable_cus(None) as u:
        cus = u.cus
    keys = sorted({go.launch_plan(r, v, cus)["key"] for r, v, _ in CELLS})
    missing = [k for k in keys if k not in SEEN]
    for k in keys:
        print("ran: %3d  %s" % (SEEN.get(k, 0), k))
    assert not missing, missing
    for label in (go.REG9, go.REG1, go.DMA9, go.DMA1, go.PWB, go.SMALL, go.FLD):
        assert any(k.startswith(label) for k in SEEN), label
