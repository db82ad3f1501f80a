"""Non-finite values through the layer kernels and through a training step.

One value -- a NaN of one of four bit patterns, +inf or -inf -- is planted in one element of a valid operand of a launch;
the launch runs twice on the same kernel label and grid, without and with the plant, and

    rule 1 (containment)    outside the footprint F every stored bit (output tensors with their sentinels, BatchNorm partial
                            rows, weight-gradient elements) is that of the launch without the plant;
    rule 2 (no laundering)  every element that is non-finite in the float64 reference (R, torch semantics: relu and
                            max_pool2d carry a NaN) is non-finite in the kernel's output;
    rule 3 (step)           when the oracle's training-step loss is non-finite, the HIP step's loss or one of its parameter
                            gradients is, and AdamW(skip_nonfinite=True) skips the step: skipped_steps grows by one,
                            parameters and optimizer state keep their bits.

R, F and the plant list are tests/nonfinite_oracle.py's; tests/test_nonfinite_host.py shows on the CPU that R is never
empty, lies inside F, and that F leaves at least half of the output alone for every activation plant.

NaN where the reference has an inf, per family: the direct and pointwise kernels multiply the planted inf by every weight
of the window, zeros included (inf * 0 = NaN), exactly as the reference's sum does; the Winograd kernels form inf - inf in
the input transform B^T d B, so every output of the tile is NaN whatever the weights.  Rule 2 asks for non-finite only.

Which family runs with which operand (tests/nonfinite_oracle.py ROWS).  Every family runs with an epilogue ReLU and, where
its launcher takes a statistics epilogue, with stats=True (gemm_pw_kernel and gemm_pw_bf16_kernel refuse one).  A fold on
load (scale / shift / relu view) runs where a kernel has one: gemm_wino (lean and general), gemm_fast<9/1>, gemm_pix<9/1>,
gemm_bf16_kernel<9/1>; gemm_pw, gemm_pw_bf16, the LDS-DMA forms and small_cin_fwd take plain input views only and hand
such a launch to those kernels.  A gate on load exists in gemm_pix<9/1> alone (fast_args refuses a gated input view).
Reverting any one operand-load ReLU to fmaxf fails a cell: common.h view_load4 -> nf-f9-cat-fold-stats-tw8-pix,
nf-f1-fold-stats-w48-pix; gemm_fast -> ...-tw8-fast; gemm_wino lean / general -> ...-tw8-wino / -wino_general; gemm_bf16 ->
nf-k9-fold-stats-tw16-reg, nf-k1-fold-stats-reg; wgrad_fast -> nf-wg-fast9-fold; wgrad_bf16 -> nf-wg-pair9-fold,
nf-wg-quad9-fold.

KNOWN_LAUNDERS lists the operand-load sites that still turn a NaN into 0, with the reason; for their cells the test
asserts that the element IS laundered, so the table cannot go stale.  Epilogue, streaming and pool sites are never in it.
"""
import contextlib
import copy

import pytest
import torch

from tests import gemm_oracle as go
from tests import nonfinite_oracle as nf
from tests import wgrad_oracle as wo
from tests.helpers import usable_cus

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PAD, SENTINEL = 64, -776.0

# kernel label -> (site, why it stays, measured cost of changing it)
KNOWN_LAUNDERS = {
    "wgrad_wino_kernel folded": (
        "csrc/wgrad_wino.hip compute() fold: fmaxf(fmaf(x, scale, shift), 0) on the x operand read",
        "the zero padding of a folded x view is staged as NaN and cleared by exactly this fmaxf; the read has no mask, and a "
        "mask costs a compare and a select per operand element inside the MFMA loop",
        "the alternative (marker payload in the padding, compare + select in the fold) costs +0.6 % of the kernel (4.484-4.498 "
        "-> 4.507-4.520 ms per step) and is incomplete: the same fmaxf clears what the channel quads past a narrow view read "
        "(profiles/nonfinite/speed.txt, table 3)"),
}

WINO, FAST9, FAST1, PIX9, PIX1, PW32 = ("gemm_wino_kernel", "gemm_fast_kernel<9>", "gemm_fast_kernel<1>", "gemm_pix_kernel<9>",
                                        "gemm_pix_kernel<1>", "gemm_pw_kernel")
# fp32 variant -> (label at 9 taps, label at 1 tap, debug switches, direct, USE_FAST_GEMM)
F32_VARIANTS = {
    "wino": (WINO, None, {}, False, True),
    "wino_general": (WINO, None, {"WINO_NO_LEAN": 1}, False, True),
    "fast": (FAST9, FAST1, {"PW_DIRECT": 0}, True, True),
    "pw": (None, PW32, {}, False, True),
    "pix": (PIX9, PIX1, {}, False, False),
    "small": (go.SMALL, go.SMALL, {}, False, True),
}
BF16_SWITCHES = {"reg": {"BF16_NO_DMA": 1}, "dma4": {"BF16_DMA_FORM": 4, "BF16_DMA_ALL": 1},
                 "dma8": {"BF16_DMA_FORM": 8, "BF16_DMA_ALL": 1}, "pw": {}, "small": {}, "fld": {}}
SEEN = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _poke(t, at, value):
    """the exact bit pattern into element `at` of a device tensor (fp32 or bf16)"""
    if t.dtype == BF:
        _bits(t)[at] = nf.signed16(nf.BF16_VALUES[value])
    else:
        _bits(t)[at] = nf.signed32(nf.VALUES[value])


def _ran():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib.lib().unetpp_last_kernel_name().decode()


def _guarded(t64, dtype, dev):
    buf = torch.full((t64.numel() + 2 * PAD,), SENTINEL, dtype=dtype)
    buf[PAD:PAD + t64.numel()] = t64.reshape(-1).to(dtype)
    return buf.to(dev)


# ------------------------------------------------------------------------------------------------ forward / dgrad GEMMs
def _gemm_launch(r, variant, ops64, plant, dev):
    """One launch of row r on the operands ops64 (the plant already in them as the oracle sees it); the plant's exact bit
    pattern is written into the device tensor.  -> (output buffers on the host, sentinels included; partial rows
    [patches, Ncols, 2] or None; the label that ran)"""
    from unet_nested4tiny_objects_keypoints_amd import engine
    from unet_nested4tiny_objects_keypoints_amd import ops as lib_ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    bf = nf.is_bf16(r)
    act = torch.float32 if (not bf or r.family == "fld") else BF
    in_dt = torch.float32 if (not bf or r.family == "small") else BF
    gate_dt = torch.float32 if not bf else BF
    n, h, w = r.shape
    cache = {}

    def put(t, dt):
        if t is None:
            return None
        if id(t) not in cache:
            cache[id(t)] = t.to(dt).to(dev).contiguous()
        return cache[id(t)]
    xs = [put(v.t, in_dt) for v in ops64.ins]
    scales = [put(v.scale, torch.float32) for v in ops64.ins]
    shifts = [put(v.shift, torch.float32) for v in ops64.ins]
    weight = ops64.weight.float().to(dev)
    bias_param = None if ops64.bias is None else ops64.bias_param.float().to(dev)
    if plant is not None:
        target = {"x": xs[plant.view], "x_off": xs[plant.view], "gate_off": xs[plant.view], "weight": weight, "bias": bias_param,
                  "scale": scales[0], "shift": shifts[0]}[plant.where]
        _poke(target, plant.at, plant.value)
    ins = [V(xs[i], v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, scale=scales[i], shift=shifts[i], gate=put(v.gate, gate_dt),
             relu=v.relu) for i, v in enumerate(ops64.ins)]
    bufs = [_guarded(t, act, dev) for t in ops64.out_tensors]
    tensors = [b[PAD:PAD + t.numel()].view(t.shape) for b, t in zip(bufs, ops64.out_tensors)]
    if r.family == "fld":
        lib_ops.first_layer_dgrad_bf16(xs[0], weight, tensors[0])
        torch.cuda.synchronize()
        return [b.cpu() for b in bufs], None, go.FLD
    outs = [V(tensors[idx], v.c_off, v.c_len, v.sy, v.sx, v.oy, v.ox, gate=put(v.gate, gate_dt), relu=r.relu,
              accumulate=kind in ("acc", "accgate"), gate_sum=kind == "accgate") for idx, v, kind in ops64.outs]
    pack = {"fwd": engine.pack_conv_fwd, "dgrad": engine.pack_conv_dgrad, "deconv_fwd": engine.pack_deconv_fwd,
            "deconv_dgrad": engine.pack_deconv_dgrad}[r.form]
    bias = None
    if bias_param is not None:
        bias = engine.tile_bias4(bias_param) if r.form == "deconv_fwd" else bias_param
    blocks = go.fast_geometry(r)["patches"]
    stats = None
    if r.stats:
        stats = torch.full((blocks * r.ncols * 2 + 2 * PAD,), SENTINEL, device=dev)
        stats[PAD:-PAD] = float("nan")
    direct, use_fast = (F32_VARIANTS[variant][3], F32_VARIANTS[variant][4]) if not bf else (False, lib_ops.USE_FAST_GEMM)
    was = lib_ops.USE_FAST_GEMM
    lib_ops.USE_FAST_GEMM = use_fast
    try:
        lib_ops.gemm_fwd(n, h, w, r.taps, ins, outs, pack(weight), bias, None if stats is None else stats[PAD:-PAD], direct=direct)
    finally:
        lib_ops.USE_FAST_GEMM = was
    torch.cuda.synchronize()
    return [b.cpu() for b in bufs], None if stats is None else stats.cpu(), _ran()


def _expected_label(r, variant, cus):
    if not nf.is_bf16(r):
        return F32_VARIANTS[variant][0 if r.taps == 9 else 1]
    return go.launch_plan(r, variant, cus)["label"]


GEMM_CELLS = [(r, v) for r in nf.ROWS for v in r.variants]
_OPS, _REF = {}, {}


def _operands(r):
    if r.id not in _OPS:
        _OPS[r.id] = nf.operands(r)
    return _OPS[r.id]


def _added_nonfinite(r, ops, p, roundings):
    """(R per output tensor: non-finite in the reference WITH the plant and finite without it; the columns whose BatchNorm
    sums are non-finite in the reference), computed once per (row, plant)"""
    key = (r.id, p.id, roundings)
    if key not in _REF:
        bf = nf.is_bf16(r) and r.family != "fld"
        base, _ = nf.reference(r, ops, bf, roundings)
        res, stats = nf.reference(r, nf.planted(r, ops, p), bf, roundings)
        cols = None if stats is None else ~torch.isfinite(stats).all(1)
        _REF[key] = ([~torch.isfinite(a) & torch.isfinite(b) for a, b in zip(res, base)], cols)
    return _REF[key]


@pytest.mark.parametrize("cell", GEMM_CELLS, ids=["%s-%s" % (r.id, v) for r, v in GEMM_CELLS])
def test_gemm_plants_stay_in_their_footprint_and_reach_the_output(dev, cell):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    r, variant = cell
    ops = _operands(r)
    switches = dict(BF16_SWITCHES[variant] if nf.is_bf16(r) else F32_VARIANTS[variant][2])
    if r.family == "k1":
        switches["PW_DIRECT"] = 0
    failures = []
    with contextlib.ExitStack() as stack:
        u = stack.enter_context(usable_cus(8 if r.multi else None))   # multi rows: several units per persistent workgroup
        for name, value in switches.items():
            stack.enter_context(_lib.debug_switch(name, value))
        label = _expected_label(r, variant, u.cus)
        base_out, base_stats, ran = _gemm_launch(r, variant, ops, None, dev)
        assert ran == label, (r.id, variant, ran, label)
        base_ref, _ = nf.reference(r, ops, nf.is_bf16(r) and r.family != "fld", go.ROUNDINGS.get(label, 1))
        for b, t in zip(base_out, base_ref):
            assert bool((b[:PAD] == SENTINEL).all()) and bool((b[-PAD:] == SENTINEL).all())
            body = b[PAD:-PAD].view(t.shape).double()
            assert torch.equal(body[~torch.isnan(t)], t[~torch.isnan(t)]), "the launch without a plant equals the oracle"
            assert bool(torch.isnan(body[torch.isnan(t)]).all()), "elements outside the launch's views are left alone"
        for p in nf.plants(r, ops):
            what = "%s %s %s" % (r.id, variant, p.id)
            got_out, got_stats, ran_p = _gemm_launch(r, variant, nf.planted(r, ops, p), p, dev)
            assert ran_p == label, (what, ran_p)
            R, stat_cols = _added_nonfinite(r, ops, p, go.ROUNDINGS.get(label, 1))
            F, rows_f, _ = nf.footprint(r, ops, p, variant)
            for i, (g, b, t) in enumerate(zip(got_out, base_out, ops.out_tensors)):
                same = _bits(g) == _bits(b)
                if not bool(same[:PAD].all() and same[-PAD:].all()):
                    failures.append(what + ": a sentinel of output %d changed" % i)
                same = same[PAD:-PAD].view(t.shape)
                leaked = ~same & ~F[i]
                if bool(leaked.any()):
                    failures.append("%s: rule 1, output %d: %d elements outside the footprint changed, first %s" % (
                        what, i, int(leaked.sum()), leaked.nonzero()[0].tolist()))
                finite = torch.isfinite(g[PAD:-PAD].view(t.shape).float())
                laundered = R[i] & finite
                if bool(laundered.any()):
                    failures.append("%s: rule 2, output %d: %d of the reference's %d non-finite elements are finite, first %s" % (
                        what, i, int(laundered.sum()), int(R[i].sum()), laundered.nonzero()[0].tolist()))
            if r.stats:
                gs, bs = got_stats[PAD:-PAD].view(-1, r.ncols, 2), base_stats[PAD:-PAD].view(-1, r.ncols, 2)
                if not torch.equal(_bits(got_stats[:PAD]), _bits(base_stats[:PAD])) or not torch.equal(
                        _bits(got_stats[-PAD:]), _bits(base_stats[-PAD:])):
                    failures.append(what + ": a sentinel of the partial sums changed")
                leaked = (_bits(gs) != _bits(bs)).any(2) & ~rows_f
                if bool(leaked.any()):
                    failures.append("%s: rule 1, partial sums: %d rows outside the footprint changed, first %s" % (
                        what, int(leaked.sum()), leaked.nonzero()[0].tolist()))
                quiet = stat_cols & torch.isfinite(gs).all(2).all(0)
                if bool(quiet.any()):
                    failures.append("%s: rule 2, partial sums: columns %s are non-finite in the reference only" % (
                        what, quiet.nonzero().flatten().tolist()))
    assert not failures, "\n".join(failures)
    key = variant if variant.startswith("wino") else label
    SEEN[key] = SEEN.get(key, 0) + 1


# ------------------------------------------------------------------------------------------------ weight gradients
WG_SHAPE = (2, 9, 40)     # 32-wide patches (the Winograd kernel's), a ragged second patch per image
WG_CASES = [
    wo.case("nf-wg-wino", "wgrad_wino_kernel", WG_SHAPE, [8], 8, (1, 4)),
    wo.case("nf-wg-wino-fold", "wgrad_wino_kernel", WG_SHAPE, [8], 8, (1, 4), fold=True),
    wo.case("nf-wg-fast9-fold", "wgrad_fast_kernel<9>", WG_SHAPE, [8], 8, (1, 4), fold=True, direct=True),
    wo.case("nf-wg-dma9", "wgrad_dma_kernel<9>", WG_SHAPE, [8], 8, (1, 4), direct=True),
    wo.case("nf-wg-pw", "wgrad_pw_kernel", (2, 16, 32), [64], 32, (1, 4), taps=1, deconv=True),
    wo.case("nf-wg-first-c1", "small_cin_wgrad_kernel", WG_SHAPE, [1], 8, (1, 4)),
    wo.case("nf-wg-pair9-fold", "wgrad_bf16_kernel<9>", WG_SHAPE, [8], 8, (1, 4), bf16=True, fold=True),
    wo.case("nf-wg-quad9-fold", "wgrad_bf16_quad_kernel<9>", WG_SHAPE, [64], 64, (1, 4), bf16=True, fold=True),
]


def _wg_reference(c, ops):
    n, h, w = c.shape
    x, dy = wo.concat(ops.xs, h, w), wo.concat(ops.dys, h, w)
    numel = 1
    for s in c.dw_shape:
        numel *= s
    dw = wo.scatter_dw(wo.shifted_sums(x, dy, c.taps), c.dw_strides, c.n_inner, numel)
    db = dy.sum((0, 1, 2)).view(dy.shape[3] // c.n_inner, c.n_inner).sum(0)
    return dw, db


def _wg_footprint(c, where, ch):
    """(dw mask flat in the destination layout, db mask): an x element of channel k reaches row k of every plane, a dy
    element of column n reaches column n of every plane and db[n]"""
    planes = torch.zeros(c.taps, c.k, c.ncols, dtype=wo.F64)
    db = torch.zeros(c.n_inner, dtype=torch.bool)
    if where == "x":
        planes[:, ch, :] = 1.0
    else:
        planes[:, :, ch] = 1.0
        db[ch % c.n_inner] = True
    numel = 1
    for s in c.dw_shape:
        numel *= s
    return wo.scatter_dw(planes, c.dw_strides, c.n_inner, numel) > 0, db


def _wg_launch(c, ops, plant, n_split, dev):
    from tests.test_gpu_wgrad_exact import _device_views, _guarded as guarded, _intact, _launch
    xv, dv = _device_views(c, ops, dev)
    if plant is not None:
        where, at, value = plant
        _poke((xv if where == "x" else dv)[0].t, at, value)
    numel = 1
    for s in c.dw_shape:
        numel *= s
    dw_buf, dw = guarded(numel, dev)
    db_buf, db = guarded(c.n_inner, dev)
    plan = _launch(c, xv, dv, n_split, dw, db)
    torch.cuda.synchronize()
    assert plan.kernel.decode() == _ran() == c.label, (c.id, plan.kernel.decode(), _ran())
    assert plan.n_split == n_split
    assert _intact(dw_buf, numel) and _intact(db_buf, c.n_inner), c.id + ": a sentinel was overwritten"
    return dw.cpu(), db.cpu()


@pytest.mark.parametrize("c", WG_CASES, ids=[c.id for c in WG_CASES])
def test_wgrad_plants_stay_in_their_row_or_column(dev, c):
    ops = wo.integer_operands(c)
    n, h, w = c.shape
    base_ref = _wg_reference(c, ops)
    assert bool(torch.isfinite(base_ref[0]).all())
    failures = []
    x_values = ["qnan", "+inf"] if (c.bf16 and not c.first_layer) else ["snan", "nanff", "+inf"]
    dy_values = ["qnan", "-inf"] if c.bf16 else ["nan7f", "-inf"]
    scale = ops.xs[0].scale
    kx = 2 if scale is not None else c.xs[0][2] - 1     # fold_parameters: channel 2 has scale 2 (a positive one)
    hd, wd = (2 * h, 2 * w) if c.deconv else (h, w)
    plants = [("x", (n - 1, h - 1, w - 1, c.xs[0][1] + kx), v) for v in x_values[:1]] + \
             [("x", (0, 0, 0, c.xs[0][1] + kx), v) for v in x_values[1:2]] + \
             [("x", (0, h // 2, w // 2, c.xs[0][1] + kx), v) for v in x_values[2:]] + \
             [("dy", (n - 1, hd - 1, wd - 1, c.dy[1] + c.dy[2] - 1), dy_values[0]), ("dy", (0, 0, 0, c.dy[1]), dy_values[1])]
    folded = any(c.fold)
    launder = KNOWN_LAUNDERS.get(c.cover) if folded else None
    for n_split in c.splits:
        base_dw, base_db = _wg_launch(c, ops, None, n_split, dev)
        for where, at, value in plants:
            what = "%s split %d %s %s %s" % (c.id, n_split, where, at, value)
            o2 = copy.deepcopy(ops)
            if c.deconv:
                for v in o2.dys:
                    v.t = o2.dys[0].t
            (o2.xs if where == "x" else o2.dys)[0].t[at] = nf.as_float(value)
            ref_dw, ref_db = _wg_reference(c, o2)
            r_dw, r_db = ~torch.isfinite(ref_dw), ~torch.isfinite(ref_db)
            assert bool(r_dw.any()), what + ": R is empty"
            got_dw, got_db = _wg_launch(c, o2, (where, at, value), n_split, dev)
            ch = at[3] - (c.xs[0][1] if where == "x" else c.dy[1])
            if c.deconv and where == "dy":
                ch = (2 * (at[1] % 2) + (at[2] % 2)) * c.n_inner + ch
            f_dw, f_db = _wg_footprint(c, where, ch)
            assert not bool((r_dw & ~f_dw).any()) and not bool((r_db & ~f_db).any()), what + ": R leaves F"
            leaked = (_bits(got_dw) != _bits(base_dw)) & ~f_dw
            if bool(leaked.any()):
                failures.append("%s: rule 1: %d dw elements outside the footprint changed" % (what, int(leaked.sum())))
            if bool(((_bits(got_db) != _bits(base_db)) & ~f_db).any()):
                failures.append(what + ": rule 1: db outside the footprint changed")
            quiet = r_dw & torch.isfinite(got_dw)
            nan_plant = value in nf.NANS
            if launder is not None and where == "x" and nan_plant:
                if not bool(torch.isfinite(got_dw).all()):
                    failures.append(what + ": KNOWN_LAUNDERS is stale: this site no longer turns the NaN into 0")
            elif bool(quiet.any()):
                failures.append("%s: rule 2: %d of %d non-finite dw elements are finite" % (what, int(quiet.sum()), int(r_dw.sum())))
            if bool((r_db & torch.isfinite(got_db)).any()):
                failures.append(what + ": rule 2: db")
    assert not failures, "\n".join(failures)
    SEEN[c.cover] = SEEN.get(c.cover, 0) + 1


# ------------------------------------------------------------------------------------------------ streaming kernels
POOL_CASES = [(2, 6, 16, 32, False, "affine_relu_pool_rows"), (2, 6, 10, 8, False, "affine_relu_pool<4>"),
              (2, 6, 10, 3, False, "affine_relu_pool<1>"), (2, 6, 16, 32, True, "affine_relu_pool_bf16")]


@pytest.mark.parametrize("case", POOL_CASES, ids=[c[5] for c in POOL_CASES])
def test_pool_nan_wins_its_window_and_takes_the_gradient(dev, case):
    """affine + ReLU + 2x2 max-pool with winners, and maxpool_bwd: a NaN (and a NaN the affine makes of an inf: inf * 0)
    is stored in act, wins its window, the winner index is the reference's (the LAST NaN of a window), and backward routes
    the window's gradient to that element; every other element of act, pooled, the winners and d_act keeps its bits."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, h, w, c, bf, label = case
    dt = BF if bf else torch.float32
    g = torch.Generator().manual_seed(7)
    y = torch.randint(-3, 4, (n, h, w, c), generator=g).double()
    scale = torch.tensor([1.0, 0.0, -1.0, 2.0, 0.5, 1.0, 1.0, -0.5], dtype=torch.float64).repeat((c + 7) // 8)[:c].contiguous()
    shift = torch.randint(-2, 3, (c,), generator=g).double()
    plants = [((0, 0, 0, 0), "qnan"), ((0, 1, 3, 2), "nanff"), ((1, 2, 4, 0), "snan"), ((1, 3, 5, 0), "nan7f"),
              ((n - 1, h - 1, w - 1, c - 1), "qnan"), ((0, 4, 6, 1), "+inf"), ((1, 0, 8, 2), "-inf"), ((0, 5, 9, 0), "-inf")]
    if bf:
        plants = [(at, v if v in nf.BF16_VALUES else "qnan") for at, v in plants]

    def run(with_plants):
        yd = y.to(dt).to(dev)
        y64 = y.clone()
        if with_plants:
            for at, v in plants:
                _poke(yd, at, v)
                y64[at] = nf.as_float(v)
        act = torch.full_like(yd, float("nan"))
        pooled = torch.full((n, h // 2, w // 2, c), float("nan"), dtype=dt, device=dev)
        idx = torch.full((n, h // 2, w // 2, c), 9, dtype=torch.uint8, device=dev)
        ops.affine_relu_pool(yd, scale.float().to(dev), shift.float().to(dev), True, act, pooled, idx)
        assert _ran() == label, (_ran(), label)
        want_act = nf.relu_keep_nan(y64 * scale + shift)
        want_pool, want_idx = nf.pool_reference(want_act)
        d_pooled = torch.randint(1, 5, (n, h // 2, w // 2, c), generator=torch.Generator().manual_seed(9)).to(dt).to(dev)
        d_act = torch.zeros(n, h, w, c, dtype=dt, device=dev)
        ops.maxpool_bwd(d_pooled, idx, d_act)
        torch.cuda.synchronize()
        return act.cpu(), pooled.cpu(), idx.cpu(), d_act.cpu(), want_act, want_pool, want_idx, d_pooled.cpu()
    a0, p0, i0, d0, wa0, wp0, wi0, _ = run(False)
    assert torch.equal(a0.double(), wa0) and torch.equal(p0.double(), wp0) and torch.equal(i0.long(), wi0)
    a1, p1, i1, d1, wa1, wp1, wi1, dp = run(True)
    nan_act, nan_pool = torch.isnan(wa1), torch.isnan(wp1)
    assert int(nan_act.sum()) >= 6 and int(nan_pool.sum()) >= 5           # (the 0-scale channel turns an inf into a NaN)
    assert bool(torch.isnan(a1.double())[nan_act].all()), "rule 2: act"
    assert bool(torch.isnan(p1.double())[nan_pool].all()), "rule 2: pooled"
    assert torch.equal(a1.double()[~nan_act], wa1[~nan_act]) and torch.equal(p1.double()[~nan_pool], wp1[~nan_pool])
    assert torch.equal(i1.long(), wi1), "winner indices, NaN windows included"
    changed_act = wa1 != wa0
    changed_act |= nan_act
    assert torch.equal(_bits(a1)[~changed_act], _bits(a0)[~changed_act]), "rule 1: act"
    changed_pool = (wp1 != wp0) | nan_pool
    assert torch.equal(_bits(p1)[~changed_pool], _bits(p0)[~changed_pool]), "rule 1: pooled"
    assert torch.equal(i1[~changed_pool], i0[~changed_pool]), "rule 1: winners"
    # backward: the window's gradient lands on the winner, the NaN element included
    want_d = torch.zeros(n, h, w, c, dtype=torch.float64)
    oy = 2 * torch.arange(h // 2).view(1, -1, 1, 1) + wi1 // 2
    ox = 2 * torch.arange(w // 2).view(1, 1, -1, 1) + wi1 % 2
    bi = torch.arange(n).view(-1, 1, 1, 1).expand_as(wi1)
    ci = torch.arange(c).view(1, 1, 1, -1).expand_as(wi1)
    want_d[bi, oy, ox, ci] = dp.double()
    assert torch.equal(d1.double(), want_d)
    for at, v in plants[:5]:
        if at != (1, 2, 4, 0):      # (shares its window with (1, 3, 5, 0): the last NaN of a window keeps it)
            assert float(d1[at]) > 0, ("the NaN element did not receive its window's gradient", at)
    SEEN[label] = SEEN.get(label, 0) + 1
    SEEN["maxpool_bwd"] = SEEN.get("maxpool_bwd", 0) + 1


def test_bn_finalize_nan_row_poisons_its_channel_only(dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    rows, c, count = 37, 24, 37 * 64
    g = torch.Generator().manual_seed(3)
    part = torch.rand(rows, c, 2, generator=g) * 4
    part[..., 1] += 16
    gam, bet = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)

    def run(plants):
        p = part.clone().to(dev)
        for at, v in plants:
            _poke(p, at, v)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        out = ops.bn_finalize(p.view(-1), rows, c, count, gam.to(dev), bet.to(dev), 1e-5, 0.1, rm, rv)
        torch.cuda.synchronize()
        return [t.cpu() for t in out] + [rm.cpu(), rv.cpu()]
    base = run([])
    assert all(bool(torch.isfinite(t).all()) for t in base)
    plants = [((0, 3, 0), "qnan"), ((rows - 1, 7, 1), "snan"), ((5, 11, 0), "+inf"), ((20, c - 1, 1), "nanff"), ((9, 0, 0), "-inf")]
    got = run(plants)
    hit = torch.zeros(c, dtype=torch.bool)
    hit[[3, 7, 11, c - 1, 0]] = True
    for name, t, b in zip(("mean", "invstd", "scale", "shift", "running_mean", "running_var"), got, base):
        assert torch.equal(_bits(t)[~hit], _bits(b)[~hit]), "rule 1: " + name
    # a NaN sum: every output of the channel; an infinite sum of values: the mean and everything after it; of squares: the variance
    assert all(not bool(torch.isfinite(t[3])) for t in got), "a NaN sum of values reaches every output of its channel"
    for ch, names in ((7, (1, 2, 3, 5)), (c - 1, (1, 2, 3, 5)), (11, (0, 3, 4)), (0, (0, 3, 4))):
        for k in names:
            assert not bool(torch.isfinite(got[k][ch])), (ch, k)
    SEEN["bn_finalize"] = 1


BN_BWD_CASES = [("plain", (2, 6, 10, 8), False, "bn_bwd_apply<4>"), ("pool", (2, 8, 16, 32), False, "bn_bwd_apply_pool"),
                ("bf16", (2, 8, 16, 32), True, "bn_bwd_apply_bf16"), ("bf16-pool", (2, 8, 16, 32), True, "bn_bwd_apply_bf16/pool")]


@pytest.mark.parametrize("case", BN_BWD_CASES, ids=[c[0] for c in BN_BWD_CASES])
def test_bn_backward_nan_statistics_reach_dgamma(dev, case):
    """bn_bwd_reduce / finalize / apply, plain, fused-pool and bf16: a channel whose mean (or invstd) is NaN -- what
    bn_finalize writes for a channel with a NaN in its sums -- gets a NaN dgamma although every gated gradient of the
    channel may be zero (0 * NaN), and a NaN gradient element gives a NaN dbeta and dgamma; the other channels keep their
    bits in dgamma, dbeta and dy.  Rule 3 rests on this for BatchNorm networks."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    name, (n, h, w, c), bf, label = case
    dt = BF if bf else torch.float32
    pool = name.endswith("pool")
    g = torch.Generator().manual_seed(11)
    y = torch.randint(-3, 4, (n, h, w, c), generator=g).float()
    d_act = torch.randint(-2, 3, (n, h, w, c), generator=g).float()
    scale, shift = 1 + 0.25 * torch.randint(-2, 3, (c,), generator=g).float(), 0.5 * torch.randint(-2, 3, (c,), generator=g).float()
    mean, invstd = 0.25 * torch.randint(-4, 5, (c,), generator=g).float(), 0.5 + 0.25 * torch.randint(0, 4, (c,), generator=g).float()
    gamma = scale / invstd
    d_pooled = torch.randint(-2, 3, (n, h // 2, w // 2, c), generator=g).float()
    idx = torch.randint(0, 4, (n, h // 2, w // 2, c), generator=g).to(torch.uint8)

    def run(poke):
        t = dict(y=y.to(dt).to(dev), d_act=d_act.to(dt).to(dev), scale=scale.to(dev), shift=shift.to(dev), mean=mean.to(dev),
                 invstd=invstd.to(dev), gamma=gamma.to(dev))
        for key, at, v in poke:
            _poke(t[key], at, v)
        dy = torch.full((n, h, w, c), float("nan"), dtype=dt, device=dev)
        p = (d_pooled.to(dt).to(dev), idx.to(dev)) if pool else None
        dgamma, dbeta = ops.bn_backward(t["d_act"], t["y"], t["scale"], t["shift"], t["mean"], t["invstd"], t["gamma"], dy, pool=p)
        torch.cuda.synchronize()
        return dgamma.cpu(), dbeta.cpu(), dy.cpu(), _ran()
    base = run([])
    assert all(bool(torch.isfinite(t.float()).all()) for t in base[:3])
    # channel 1: NaN mean and shift (the whole channel gated shut: fma(y, scale, NaN) > 0 is false); channel 2: NaN invstd;
    # channel 5: one NaN gradient element behind an open gate
    open_at = (((y * scale + shift) > 0)[..., 5]).nonzero()[0].tolist()
    poke = [("mean", (1,), "qnan"), ("shift", (1,), "qnan"), ("invstd", (2,), "snan" if not bf else "qnan"),
            ("d_act", tuple(open_at) + (5,), "qnan")]
    got = run(poke)
    hit = torch.zeros(c, dtype=torch.bool)
    hit[[1, 2, 5]] = True
    assert torch.equal(_bits(got[0])[~hit], _bits(base[0])[~hit]), "rule 1: dgamma"
    assert torch.equal(_bits(got[1])[~hit], _bits(base[1])[~hit]), "rule 1: dbeta"
    assert torch.equal(_bits(got[2])[..., ~hit], _bits(base[2])[..., ~hit]), "rule 1: dy"
    assert not bool(torch.isfinite(got[0][1])), "dgamma of a channel with a NaN mean (0 * NaN over gated-off elements)"
    assert not bool(torch.isfinite(got[0][2])), "dgamma of a channel with a NaN invstd"
    assert not bool(torch.isfinite(got[0][5])) and not bool(torch.isfinite(got[1][5])), "a NaN gradient element"
    assert not bool(torch.isfinite(got[2][..., 2].float()).any()), "dy of a channel with a NaN invstd"
    assert got[3] == base[3] == label, (got[3], label)      # (the last launch of bn_backward: the apply twin of the case)
    SEEN["bn_bwd " + name] = 1


AFFINE_CASES = [((2, 5, 7, 8), False, "affine_relu<4>"), ((2, 5, 7, 3), False, "affine_relu<1>"), ((2, 5, 7, 8), True, "affine_relu_bf16")]


@pytest.mark.parametrize("case", AFFINE_CASES, ids=[c[2] for c in AFFINE_CASES])
def test_affine_relu_keeps_nan_and_nothing_else_moves(dev, case):
    """the plain apply pass (no pool): relu(fma(y, scale, shift)) stores a NaN for a NaN and for inf * 0, +0 for -inf"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    (n, h, w, c), bf, label = case
    dt = BF if bf else torch.float32
    g = torch.Generator().manual_seed(17)
    y = torch.randint(-3, 4, (n, h, w, c), generator=g).double()
    scale = torch.tensor([1.0, 0.0, -1.0, 2.0, 0.5, 1.0, 1.0, -0.5], dtype=torch.float64)[:c].contiguous()
    shift = torch.randint(-2, 3, (c,), generator=g).double()
    plants = [((0, 0, 0, 0), "qnan"), ((1, 4, 6, c - 1), "nanff"), ((0, 2, 3, 2), "snan"), ((1, 1, 1, 0), "nan7f"),
              ((0, 3, 2, 1), "+inf"), ((1, 2, 5, 0), "-inf"), ((0, 4, 4, 2), "-inf")]
    if bf:
        plants = [(at, v if v in nf.BF16_VALUES else "qnan") for at, v in plants]

    def run(with_plants):
        yd, y64 = y.to(dt).to(dev), y.clone()
        if with_plants:
            for at, v in plants:
                _poke(yd, at, v)
                y64[at] = nf.as_float(v)
        act = torch.full_like(yd, float("nan"))
        ops.affine_relu_pool(yd, scale.float().to(dev), shift.float().to(dev), True, act, None, None)
        assert _ran() == label, (_ran(), label)
        torch.cuda.synchronize()
        return act.cpu(), nf.relu_keep_nan(y64 * scale + shift)
    a0, w0 = run(False)
    a1, w1 = run(True)
    assert torch.equal(a0.double(), w0)
    nan = torch.isnan(w1)
    assert int(nan.sum()) == 5, "four NaN plants and inf * 0"
    assert bool(torch.isnan(a1.double())[nan].all()), "rule 2"
    assert torch.equal(a1.double()[~nan], w1[~nan]), "-inf through a positive scale is +0, through a negative one +inf"
    touched = torch.zeros_like(nan)
    for at, _ in plants:
        touched[at] = True
    assert torch.equal(_bits(a1)[~touched], _bits(a0)[~touched]), "rule 1"
    SEEN[label] = 1


def _bilinear_rows(size, y):
    """destination indices of the doubled axis whose two taps (align_corners=True) include source index y"""
    out = []
    for o in range(2 * size):
        src = o * (size - 1) / (2 * size - 1)
        i0 = min(int(src), size - 1)
        if y in (i0, min(i0 + 1, size - 1)):
            out.append(o)
    return out


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_bilinear2x_plants_stay_in_their_stencil(dev, bf):
    """bilinear2x_fwd: a planted source element reaches the destinations whose two taps include it, in its channel, as in
    torch's interpolate (align_corners=True); bilinear2x_bwd: a planted gradient element reaches its (up to) four sources"""
    import torch.nn.functional as F
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, h, w, c = 2, 5, 6, 8
    dt = BF if bf else torch.float32
    g = torch.Generator().manual_seed(19)
    x = torch.randint(-3, 4, (n, h, w, c), generator=g).double()
    dy = torch.randint(-2, 3, (n, 2 * h, 2 * w, c), generator=g).double()
    values = ["qnan", "+inf", "-inf"] if bf else ["snan", "nanff", "+inf", "-inf", "nan7f"]
    spots = [(1, 2, 3, 5), (0, 0, 0, 0), (n - 1, h - 1, w - 1, c - 1), (0, 4, 2, 2), (1, 0, 5, 7)]

    def fwd(plant):
        xd, x64 = x.to(dt).to(dev), x.clone()
        if plant:
            _poke(xd, plant[0], plant[1])
            x64[plant[0]] = nf.as_float(plant[1])
        yd = torch.full((n, 2 * h, 2 * w, c), float("nan"), dtype=dt, device=dev)
        ops.bilinear2x_fwd(xd, yd)
        assert _ran() == ("bilinear2x_fwd_bf16" if bf else "bilinear2x_fwd")
        torch.cuda.synchronize()
        ref = F.interpolate(x64.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        return yd.cpu(), ref

    def bwd(plant):
        dyd, dy64 = dy.to(dt).to(dev), dy.clone()
        if plant:
            _poke(dyd, plant[0], plant[1])
            dy64[plant[0]] = nf.as_float(plant[1])
        dxd = torch.full((n, h, w, c), float("nan"), dtype=dt, device=dev)
        ops.bilinear2x_bwd(dyd, dxd, False)
        assert _ran() == ("bilinear2x_bwd_bf16" if bf else "bilinear2x_bwd")
        torch.cuda.synchronize()
        return dxd.cpu()
    y0, _ = fwd(None)
    d0 = bwd(None)
    assert bool(torch.isfinite(y0.float()).all()) and bool(torch.isfinite(d0.float()).all())
    for (b, sy, sx, ch), v in zip(spots, values):
        y1, ref = fwd(((b, sy, sx, ch), v))
        fmask = torch.zeros(n, 2 * h, 2 * w, c, dtype=torch.bool)
        for oy in _bilinear_rows(h, sy):
            for ox in _bilinear_rows(w, sx):
                fmask[b, oy, ox, ch] = True
        r = ~torch.isfinite(ref)
        assert bool(r.any()) and not bool((r & ~fmask).any()), "R is not empty and lies inside F"
        assert torch.equal(_bits(y1)[~fmask], _bits(y0)[~fmask]), ("rule 1 forward", v)
        assert not bool(torch.isfinite(y1.float())[r].any()), ("rule 2 forward", v)
        # backward: the gradient element at a destination that reads the source with a non-zero weight
        oy, ox = _bilinear_rows(h, sy)[-1], _bilinear_rows(w, sx)[-1]
        d1 = bwd(((b, oy, ox, ch), v))
        srcs = torch.zeros(n, h, w, c, dtype=torch.bool)
        for yy in range(h):
            for xx in range(w):
                srcs[b, yy, xx, ch] = oy in _bilinear_rows(h, yy) and ox in _bilinear_rows(w, xx)
        assert 1 <= int(srcs.sum()) <= 4
        assert torch.equal(_bits(d1)[~srcs], _bits(d0)[~srcs]), ("rule 1 backward", v)
        assert not bool(torch.isfinite(d1.float())[srcs].all()), ("rule 2 backward", v)
    SEEN["bilinear2x_fwd" + ("_bf16" if bf else "")] = SEEN["bilinear2x_bwd" + ("_bf16" if bf else "")] = 1


def _head_operands(bf, n_heads=1):
    g = torch.Generator().manual_seed(23)
    n, h, w, c, k = 2, 6, 8, 16, 2
    xs = [torch.randint(-2, 3, (n, h, w, c), generator=g).double() * 0.25 for _ in range(n_heads)]
    wts = [torch.randint(-2, 3, (k, c), generator=g).double() * 0.25 for _ in range(n_heads)]
    bs = [torch.randint(-2, 3, (k,), generator=g).double() * 0.25 for _ in range(n_heads)]
    d_out = torch.randint(-2, 3, (n, k, h, w), generator=g).double() * 0.25
    return (n, h, w, c, k), xs, wts, bs, d_out


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_head_plants_stay_in_their_pixel_or_class(dev, bf):
    """head_fwd (sigmoid(bias + x . w), no dropout) and head_bwd: an x element reaches its pixel's maps, a weight element
    its class's map; in backward a gradient element reaches dx of its pixel and dW / db of its class"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    (n, h, w, c, k), xs, wts, bs, d_out = _head_operands(bf)
    dt = BF if bf else torch.float32
    xv = "qnan" if bf else "nanff"

    def run(plant):
        t = dict(x=xs[0].to(dt).to(dev), w=wts[0].float().to(dev), b=bs[0].float().to(dev), d=d_out.float().to(dev))
        x64, w64, d64 = xs[0].clone(), wts[0].clone(), d_out.clone()
        if plant:
            key, at, v = plant
            _poke(t[key], at, v)
            {"x": x64, "w": w64, "d": d64}[key][at] = nf.as_float(v)
        out = torch.full((n, k, h, w), float("nan"), device=dev)
        ops.head_fwd(t["x"], t["w"], t["b"], 0.0, 0, None, out)
        fwd_label = _ran()
        dx = torch.full((n, h, w, c), float("nan"), dtype=dt, device=dev)
        dw, db = ops.head_bwd(t["d"], out, t["x"], t["w"], 0.0, 0, None, dx, False)
        bwd_label = _ran()
        torch.cuda.synchronize()
        assert fwd_label.startswith("head_fwd") and bwd_label.startswith("head_bwd"), (fwd_label, bwd_label)
        z = torch.einsum("nhwc,kc->nkhw", x64, w64) + bs[0].view(1, -1, 1, 1)
        s = torch.sigmoid(z)
        dl = d64 * s * (1 - s)
        ref = dict(out=s, dx=torch.einsum("nkhw,kc->nhwc", dl, w64), dw=torch.einsum("nkhw,nhwc->kc", dl, x64), db=dl.sum((0, 2, 3)))
        return dict(out=out.cpu(), dx=dx.cpu(), dw=dw.reshape(k, c).cpu().clone(), db=db.cpu().clone()), ref, (fwd_label, bwd_label)
    base, ref0, labels = run(None)
    assert all(bool(torch.isfinite(v.float()).all()) for v in base.values())
    plants = [("x", (1, 3, 5, 7), xv), ("x", (0, 0, 0, 0), "+inf"), ("w", (1, 9), "snan"), ("d", (1, 0, 5, 7), "nan7f"),
              ("d", (0, 1, 0, 0), "-inf")]
    for key, at, v in plants:
        got, ref, labels_p = run((key, at, v))
        assert labels_p == labels
        f = {name: torch.zeros(t.shape, dtype=torch.bool) for name, t in base.items()}
        if key == "x":
            b, y, x, ch = at
            f["out"][b, :, y, x] = True
            f["dx"][b, y, x, :] = True
            f["dw"][:, :] = True                # (dl of the pixel is non-finite in every class, x of the pixel in one channel)
            f["db"][:] = True
        elif key == "w":
            f["out"][:, at[0]] = True
            f["dx"][:] = True
            f["dw"][at[0], :] = True
            f["db"][at[0]] = True
        else:
            b, cls, y, x = at
            f["dx"][b, y, x, :] = True
            f["dw"][cls, :] = True
            f["db"][cls] = True
        for name in base:
            r = ~torch.isfinite(ref[name])
            assert not bool((r & ~f[name]).any()), (key, at, v, name, "R leaves F")
            assert torch.equal(_bits(got[name])[~f[name]], _bits(base[name])[~f[name]]), ("rule 1", key, at, v, name)
            assert not bool(torch.isfinite(got[name].float())[r].any()), ("rule 2", key, at, v, name)
        assert any(bool((~torch.isfinite(t)).any()) for t in ref.values()), "R is not empty"
    SEEN["head_fwd" + ("_bf16" if bf else "")] = SEEN["head_bwd" + ("_bf16" if bf else "")] = 1


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_heads_mean_plants_stay_in_their_pixel(dev, bf):
    """heads_mean_fwd / heads_mean_bwd over three heads: a feature element of ONE head reaches the mean at its pixel; a
    gradient element of the mean reaches dx of that pixel and dW / db of that class in every head"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    (n, h, w, c, k), xs, wts, bs, d_out = _head_operands(bf, 3)
    dt = BF if bf else torch.float32

    def run(plant):
        xd = [x.to(dt).to(dev) for x in xs]
        dd = d_out.float().to(dev)
        x64, d64 = [x.clone() for x in xs], d_out.clone()
        if plant:
            key, at, v = plant
            if key == "d":
                _poke(dd, at, v)
                d64[at] = nf.as_float(v)
            else:
                _poke(xd[key], at, v)
                x64[key][at] = nf.as_float(v)
        wd, bd = [t.float().to(dev) for t in wts], [t.float().to(dev) for t in bs]
        out = torch.full((n, k, h, w), float("nan"), device=dev)
        ops.heads_mean_fwd(xd, wd, bd, out)
        fl = _ran()
        dxs = [torch.full((n, h, w, c), float("nan"), dtype=dt, device=dev) for _ in xs]
        grads = ops.heads_mean_bwd(xd, wd, bd, dd, dxs, [False] * 3, [False] * 3)
        bl = _ran()
        torch.cuda.synchronize()
        assert fl.startswith("heads_mean") and bl.startswith("heads_mean_bwd"), (fl, bl)
        s = [torch.sigmoid(torch.einsum("nhwc,kc->nkhw", a, b) + cc.view(1, -1, 1, 1)) for a, b, cc in zip(x64, wts, bs)]
        ref_out = ((s[0] + s[1]) + s[2]) / 3.0
        ref_dx = [torch.einsum("nkhw,kc->nhwc", (d64 / 3.0) * si * (1 - si), wi) for si, wi in zip(s, wts)]
        return out.cpu(), [t.cpu() for t in dxs], [(a.reshape(k, c).cpu().clone(), b.cpu().clone()) for a, b in grads], ref_out, ref_dx
    o0, dx0, g0, _, _ = run(None)
    assert bool(torch.isfinite(o0).all())
    for plant in [(1, (1, 2, 3, 4), "qnan"), (2, (0, 5, 7, 15), "qnan" if bf else "nan7f"), ("d", (1, 1, 4, 6), "snan")]:
        o1, dx1, g1, ref_out, ref_dx = run(plant)
        key, at, v = plant
        if key == "d":
            b, cls, y, x = at
            assert torch.equal(_bits(o1), _bits(o0)), "the forward does not read the gradient"
            for hd in range(3):
                m = torch.zeros(n, h, w, c, dtype=torch.bool)
                m[b, y, x, :] = True
                assert torch.equal(_bits(dx1[hd])[~m], _bits(dx0[hd])[~m]), ("rule 1 dx", hd)
                r = ~torch.isfinite(ref_dx[hd])
                assert bool(r.any()) and not bool(torch.isfinite(dx1[hd].float())[r].any()), ("rule 2 dx", hd)
                rows = torch.ones(k, dtype=torch.bool)
                rows[cls] = False
                assert torch.equal(_bits(g1[hd][0])[rows], _bits(g0[hd][0])[rows]) and torch.equal(_bits(g1[hd][1])[rows], _bits(g0[hd][1])[rows])
                assert not bool(torch.isfinite(g1[hd][1][cls])), "db of the class"
        else:
            b, y, x, ch = at
            m = torch.zeros(n, k, h, w, dtype=torch.bool)
            m[b, :, y, x] = True
            r = ~torch.isfinite(ref_out)
            assert bool(r.any()) and not bool((r & ~m).any())
            assert torch.equal(_bits(o1)[~m], _bits(o0)[~m]), "rule 1 mean"
            assert not bool(torch.isfinite(o1)[r].any()), "rule 2 mean"
            for hd in range(3):
                pm = torch.zeros(n, h, w, c, dtype=torch.bool)
                if hd == key:
                    pm[b, y, x, :] = True
                assert torch.equal(_bits(dx1[hd])[~pm], _bits(dx0[hd])[~pm]), ("rule 1 dx: the other heads' gradients do not move", hd)
    SEEN["heads_mean_fwd" + ("_bf16" if bf else "")] = SEEN["heads_mean_bwd" + ("_bf16" if bf else "")] = 1


FROZEN_CASES = [("plain", (2, 6, 10, 8), False, False, "bn_frozen_bwd<4>"), ("pool", (2, 8, 16, 32), False, True, "bn_frozen_bwd_pool"),
                ("bf16", (2, 8, 16, 32), True, False, "bn_frozen_bwd_bf16"), ("bf16-pool", (2, 8, 16, 32), True, True, "bn_frozen_bwd_bf16/pool")]


@pytest.mark.parametrize("case", FROZEN_CASES, ids=[c[0] for c in FROZEN_CASES])
def test_bn_frozen_backward_nan(dev, case):
    """bn_frozen_bwd with sums: a NaN gradient element behind an open gate is NaN in dy at that element and in dgamma /
    dbeta of its channel; a NaN mean reaches dgamma of its channel; every other channel keeps its bits"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    name, (n, h, w, c), bf, pool, label = case
    dt = BF if bf else torch.float32
    g = torch.Generator().manual_seed(29)
    y = torch.randint(-3, 4, (n, h, w, c), generator=g).float()
    d_act = torch.randint(-2, 3, (n, h, w, c), generator=g).float()
    scale, shift = 1 + 0.25 * torch.randint(-2, 3, (c,), generator=g).float(), 0.5 * torch.randint(-2, 3, (c,), generator=g).float()
    mean, invstd = 0.25 * torch.randint(-4, 5, (c,), generator=g).float(), 0.5 + 0.25 * torch.randint(0, 4, (c,), generator=g).float()
    d_pooled = torch.randint(-2, 3, (n, h // 2, w // 2, c), generator=g).float()
    idx = torch.randint(0, 4, (n, h // 2, w // 2, c), generator=g).to(torch.uint8)

    def run(poke):
        t = dict(y=y.to(dt).to(dev), d_act=d_act.to(dt).to(dev), scale=scale.to(dev), shift=shift.to(dev), mean=mean.to(dev),
                 invstd=invstd.to(dev))
        for key, at, v in poke:
            _poke(t[key], at, v)
        dy = torch.full((n, h, w, c), float("nan"), dtype=dt, device=dev)
        p = (d_pooled.to(dt).to(dev), idx.to(dev)) if pool else None
        dgamma, dbeta = ops.bn_frozen_backward(t["d_act"], t["y"], t["scale"], t["shift"], t["mean"], t["invstd"], dy, pool=p)
        torch.cuda.synchronize()
        return dgamma.cpu(), dbeta.cpu(), dy.cpu()
    base = run([])
    assert all(bool(torch.isfinite(t.float()).all()) for t in base)
    # the same launch without the sums leaves its own label behind (with them the finalize kernel's is the last one)
    dy2 = torch.full((n, h, w, c), float("nan"), dtype=dt, device=dev)
    ops.bn_frozen_backward(d_act.to(dt).to(dev), y.to(dt).to(dev), scale.to(dev), shift.to(dev), None, None, dy2,
                           pool=(d_pooled.to(dt).to(dev), idx.to(dev)) if pool else None, want_sums=False)
    assert _ran() == label, (_ran(), label)
    assert torch.equal(_bits(dy2.cpu()), _bits(base[2]))
    open_at = tuple((((y * scale + shift) > 0)[..., 5]).nonzero()[0].tolist()) + (5,)
    got = run([("mean", (1,), "qnan"), ("d_act", open_at, "qnan")])
    hit = torch.zeros(c, dtype=torch.bool)
    hit[[1, 5]] = True
    for k_, nm in enumerate(("dgamma", "dbeta")):
        assert torch.equal(_bits(got[k_])[~hit], _bits(base[k_])[~hit]), "rule 1: " + nm
    touched = torch.zeros(n, h, w, c, dtype=torch.bool)
    touched[open_at] = True
    assert torch.equal(_bits(got[2])[~touched], _bits(base[2])[~touched]), "rule 1: dy (the mean is not read for dy)"
    assert not bool(torch.isfinite(got[2][open_at].float())), "dy at the NaN gradient element"
    assert not bool(torch.isfinite(got[0][1])), "dgamma of a channel with a NaN mean"
    assert not bool(torch.isfinite(got[0][5])) and not bool(torch.isfinite(got[1][5])), "dgamma / dbeta of the NaN gradient's channel"
    SEEN["bn_frozen_bwd " + name] = 1


def test_focal_bce_nan_pred(dev):
    """focal_bce and focal_bce_heads: a NaN prediction gives a NaN loss; the gradient elements elsewhere keep their bits"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    g = torch.Generator().manual_seed(13)
    rows, n = 2, 2 * 3 * 9 * 7
    pred = torch.rand(2, 3, 9, 7, generator=g) * 0.98 + 0.01
    target = torch.rand(2, 3, 9, 7, generator=g)
    at = (1, 2, 8, 6)
    for value in ("qnan", "nanff", "snan"):
        p0, p1 = pred.to(dev), pred.to(dev)
        _poke(p1, at, value)
        l0, g0 = ops.focal_bce(p0, target.to(dev), rows, 3.0)
        l1, g1 = ops.focal_bce(p1, target.to(dev), rows, 3.0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(l0).all()) and not bool(torch.isfinite(l1).any()), value
        same = _bits(g0.cpu()) == _bits(g1.cpu())
        same[at] = True
        assert bool(same.all()), value
        assert not bool(torch.isfinite(g1[at])), "the gradient at the NaN prediction"
    heads0 = [pred.to(dev), (pred * 0.5 + 0.2).to(dev)]
    heads1 = [h.clone() for h in heads0]
    _poke(heads1[1], at, "qnan")
    out0 = ops.focal_bce_heads(heads0, target.to(dev), rows, 3.0)
    out1 = ops.focal_bce_heads(heads1, target.to(dev), rows, 3.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out0[0]).all()) and not bool(torch.isfinite(out1[0]).all())
    for k, (a, b) in enumerate(zip(out0[1], out1[1])):
        same = _bits(a.cpu()) == _bits(b.cpu())
        if k == 1:
            same[at] = True
        assert bool(same.all()), k
    SEEN["focal_bce"] = SEEN["focal_bce_heads"] = 1


# ------------------------------------------------------------------------------------------------ model level
CTOR = dict(in_channels=1, n_classes=2, feature_scale=8)    # widths 4, 8, 16, 32


def _ctor(bf):
    """bf16 storage needs channel counts 8 * 2^k (the library refuses feature_scale=8 with it): widths 8, 16, 32, 64"""
    return dict(CTOR, feature_scale=4) if bf else CTOR


MODEL_CELLS = [(dc, bn, bf, pruned) for dc in (True, False) for bn in (True, False) for bf in (False, True) for pruned in (False, True)]
MODEL_PLANTS = ["x-nan", "x-inf", "w-conv00", "w-decoder", "w-head", "gamma"]
_ORACLE = {}


def _model_data():
    g = torch.Generator().manual_seed(21)
    return torch.randn(2, 1, 32, 32, generator=g), torch.rand(2, 2, 32, 32, generator=g)


def _plant_model(model, x, plant):
    """-> the input to use; parameters are edited in place (the same element on either side)"""
    x = x.clone()
    p = dict(model.named_parameters())
    with torch.no_grad():
        if plant == "x-nan":
            x[1, 0, 17, 9] = float("nan")
        elif plant == "x-inf":
            x[0, 0, 0, 0] = float("inf")
        elif plant == "w-conv00":
            p["conv00.conv1.0.weight"][3, 0, 1, 1] = float("nan")
        elif plant == "w-decoder":
            p["up_concat01.conv.conv2.0.weight"][2, 1, 0, 2] = float("nan")
        elif plant == "w-head":
            p["final_1.weight"][1, 3, 0, 0] = float("nan")
        elif plant == "gamma":
            p["conv00.conv2.1.weight"][2] = float("nan")
    return x


def _oracle_loss(dc, bn, bf, pruned, plant, state):
    """float64 oracle: (training-step loss, eval maps) with the plant"""
    from oracle.step_oracle import focal_bce_2d_oracle
    from oracle.unet_nested_oracle import UNetNestedOracle
    key = (dc, bn, _ctor(bf)["feature_scale"], pruned, plant)
    if key not in _ORACLE:
        x, target = _model_data()
        ref = UNetNestedOracle(is_deconv=dc, is_batchnorm=bn, **_ctor(bf))
        ref.load_state_dict(state)
        ref = ref.double().train()
        ref.drop_out.eval()
        xp = _plant_model(ref, x, plant).double()
        with torch.no_grad():
            outs = ref(xp)
            outs = outs[:1] if pruned else outs
            loss = sum(focal_bce_2d_oracle(o, target.double()) for o in outs) / len(outs)
            ref.load_state_dict(state)          # the training forward above moved the BatchNorm buffers
            ref = ref.double()
            _plant_model(ref, x, plant)
            maps = ref.eval()(xp)
        _ORACLE[key] = (float(loss), [m.clone() for m in (maps[:1] if pruned else maps)])
    return _ORACLE[key]


def _snapshot(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        out += [v.clone() for _, v in sorted(opt.state.get(p, {}).items()) if torch.is_tensor(v)]
    return out


def _same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(_bits(x.contiguous()), _bits(y.contiguous())) for x, y in zip(a, b))


@pytest.mark.parametrize("cell", MODEL_CELLS, ids=["%s-%s-%s-%s" % ("deconv" if c[0] else "bilinear", "bn" if c[1] else "nobn",
                                                                    "bf16" if c[2] else "f32", "head1" if c[3] else "full")
                                                   for c in MODEL_CELLS])
def test_poisoned_step_is_seen_and_skipped(dev, cell):
    """Rule 3 for every plant of MODEL_PLANTS, and rule 2 on the eval maps of model.eval()(x) and infer(x, 1)."""
    import unet_nested4tiny_objects_keypoints_amd as pkg
    from tests.helpers import seeded_state
    dc, bn, bf, pruned = cell
    x, target = _model_data()
    net = pkg.UNet_Nested(is_deconv=dc, is_batchnorm=bn, **_ctor(bf))
    state = seeded_state(net, 4)
    net.load_state_dict(state)
    net = net.to(dev).train()
    net.drop_out.eval()
    if bf:
        net.set_activation_dtype(BF)
    crit = pkg.FocalLoss_BCE_2d(gamma=3, size_average=False)
    opt = pkg.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-2, capturable=True, skip_nonfinite=True)
    td = target.to(dev)

    def step(xin):
        opt.zero_grad(set_to_none=True)
        outs = net.forward_pruned(xin.to(dev), 1) if pruned else net(xin.to(dev))
        loss = sum(crit(o, td) for o in outs) / len(outs)
        loss.backward()
        grads = [p.grad for p in net.parameters() if p.grad is not None]
        return loss.detach(), grads
    loss, grads = step(x)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads)
    opt.step()                                  # a clean step first: the optimizer state exists
    torch.cuda.synchronize()
    assert int(opt.skipped_steps) == 0
    failures = []
    skipped = 0
    for plant in MODEL_PLANTS:
        if plant == "gamma" and not bn:
            continue
        want_loss, want_maps = _oracle_loss(dc, bn, bf, pruned, plant, state)
        net.load_state_dict(state)
        net.train()
        net.drop_out.eval()
        xp = _plant_model(net, x, plant)
        net.invalidate_weight_images()
        before = _snapshot(net, opt)
        loss, grads = step(xp)
        seen = (not bool(torch.isfinite(loss))) or any(not bool(torch.isfinite(g).all()) for g in grads)
        assert not bool(torch.isfinite(torch.tensor(want_loss))), (plant, "the oracle's loss is finite: the plant is not read", want_loss)
        if not seen:
            failures.append("%s: rule 3: the oracle's loss is %r, the HIP loss %r and every gradient is finite" % (
                plant, want_loss, float(loss)))
            continue
        opt.step()
        torch.cuda.synchronize()
        skipped += 1
        if int(opt.skipped_steps) != skipped:
            failures.append("%s: skipped_steps is %d, not %d" % (plant, int(opt.skipped_steps), skipped))
        if not _same_bits(_snapshot(net, opt), before):
            failures.append(plant + ": a skipped step changed parameters or optimizer state")
        # rule 2 on the inference paths
        net.eval()
        with torch.no_grad():
            maps = [net.infer(xp.to(dev), 1)] if pruned else list(net(xp.to(dev)))
            first = net.infer(xp.to(dev), 1)
        torch.cuda.synchronize()
        for k, (m, wm) in enumerate(zip(maps, want_maps)):
            quiet = ~torch.isfinite(wm) & torch.isfinite(m.float().cpu())
            if bool(quiet.any()):
                failures.append("%s: rule 2: eval map %d: %d of %d non-finite elements are finite" % (
                    plant, k, int(quiet.sum()), int((~torch.isfinite(wm)).sum())))
        quiet = ~torch.isfinite(want_maps[0]) & torch.isfinite(first.float().cpu())
        if bool(quiet.any()):
            failures.append("%s: rule 2: infer(x, 1): %d elements" % (plant, int(quiet.sum())))
    assert not failures, "\n".join(failures)
    SEEN["model"] = SEEN.get("model", 0) + 1


def test_poisoned_step_destroys_batchnorm_buffers_as_in_torch(dev):
    """What skip_nonfinite does NOT protect: the forward of a poisoned step has already folded its batch statistics into
    running_mean / running_var.  The affected channels' buffers are NaN exactly where the oracle's are."""
    import unet_nested4tiny_objects_keypoints_amd as pkg
    from oracle.unet_nested_oracle import UNetNestedOracle
    from tests.helpers import seeded_state
    x, target = _model_data()
    net = pkg.UNet_Nested(is_deconv=True, is_batchnorm=True, **CTOR)
    state = seeded_state(net, 4)
    for plant in ("x-nan", "w-conv00"):
        net.load_state_dict(state)
        net = net.to(dev).train()
        net.drop_out.eval()
        ref = UNetNestedOracle(is_deconv=True, is_batchnorm=True, **CTOR)
        ref.load_state_dict(state)
        ref = ref.double().train()
        ref.drop_out.eval()
        with torch.no_grad():
            ref(_plant_model(ref, x, plant).double())
        xp = _plant_model(net, x, plant)
        net.invalidate_weight_images()
        net(xp.to(dev))
        torch.cuda.synchronize()
        got, want = dict(net.named_buffers()), dict(ref.named_buffers())
        poisoned = 0
        for k, wv in want.items():
            if k.endswith("num_batches_tracked"):
                continue
            bad = ~torch.isfinite(wv)
            poisoned += int(bad.sum())
            assert torch.equal(~torch.isfinite(got[k].cpu()), bad), (plant, k)
        assert poisoned > 0, plant
        if plant == "w-conv00":     # one output channel of the first convolution: that channel's buffers, and everything behind it
            assert (~torch.isfinite(want["conv00.conv1.1.running_mean"])).nonzero().flatten().tolist() == [3]


# ------------------------------------------------------------------------------------------------ coverage
def test_every_listed_label_ran(dev):
    """(after the cases of this module)"""
    wanted = ["wino", "wino_general", FAST9, FAST1, PIX9, PIX1, PW32, go.SMALL, go.REG9, go.DMA9, go.REG1, go.DMA1, go.PWB, go.FLD,
              "wgrad_wino_kernel plain", "wgrad_wino_kernel folded", "wgrad_fast_kernel<9>", "wgrad_dma_kernel<9>",
              "wgrad_pw_kernel", "small_cin_wgrad_kernel C=1 fp32", "wgrad_bf16_kernel<9>", "wgrad_bf16_quad_kernel<9>",
              "affine_relu_pool_rows", "affine_relu_pool<4>", "affine_relu_pool<1>", "affine_relu_pool_bf16", "maxpool_bwd",
              "bn_finalize", "bn_bwd plain", "bn_bwd pool", "bn_bwd bf16", "bn_bwd bf16-pool", "focal_bce", "focal_bce_heads",
              "affine_relu<4>", "affine_relu<1>", "affine_relu_bf16", "bilinear2x_fwd", "bilinear2x_bwd", "bilinear2x_fwd_bf16",
              "bilinear2x_bwd_bf16", "head_fwd", "head_bwd", "head_fwd_bf16", "head_bwd_bf16", "heads_mean_fwd", "heads_mean_bwd",
              "heads_mean_fwd_bf16", "heads_mean_bwd_bf16", "bn_frozen_bwd plain", "bn_frozen_bwd pool", "bn_frozen_bwd bf16",
              "bn_frozen_bwd bf16-pool", "model"]
    missing = [k for k in wanted if not SEEN.get(k)]
    print("ran:", SEEN)
    assert not missing, missing
