"""tests/gemm_oracle.py against F.conv2d / F.conv_transpose2d / autograd, its two epilogue sequences against a literal
restatement with torch.bfloat16 casts, the exactness margin and the data preconditions of every GPU row of
tests/test_gpu_gemm_bf16_exact.py, and the host restatement of the launchers' choices.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_oracle as go
from tests.gemm_oracle import row

F64 = torch.float64
BF = torch.bfloat16

# every form and view kind, at sizes no kernel would take (nothing is aligned)
HOST_ROWS = [
    row("fwd9", "-", (2, 9, 11), "fwd", [5], [6], variants=()),
    row("fwd1", "-", (2, 9, 11), "fwd", [5], [6], taps=1, variants=()),
    row("fwd9-sliced-concatenated", "-", (2, 7, 10), "fwd", [(12, 4, 5), 3, (9, 2, 6)], [(9, 2, 6, "store"), 4], variants=()),
    row("fwd9-folded", "-", (1, 8, 9), "fwd", [8, 4], [5], fold="exact", variants=()),
    row("dgrad9", "-", (2, 9, 11), "dgrad", [6], [(5, "acc"), (3, "gate")], variants=()),
    row("dgrad1-sliced", "-", (2, 7, 10), "dgrad", [(9, 2, 6)], [(12, 4, 5, "accgate")], taps=1, variants=()),
    row("deconv-fwd", "-", (2, 5, 6), "deconv_fwd", [7], [3], taps=1, variants=()),
    row("deconv-fwd-sliced", "-", (2, 5, 6), "deconv_fwd", [(9, 1, 7)], [(8, 2, 3, "store")], taps=1, variants=()),
    row("deconv-dgrad", "-", (2, 5, 6), "deconv_dgrad", [3], [7], taps=1, variants=()),
    row("deconv-dgrad-sliced", "-", (2, 5, 6), "deconv_dgrad", [(8, 2, 3)], [(9, 1, 7, "acc")], taps=1, variants=()),
]


def _randomised(r, seed):
    """the row's operands over full-mantissa random data (NaN poison kept where it was)"""
    ops = go.operands(r)
    g = torch.Generator().manual_seed(seed)
    new = {}

    def rnd(t):
        if id(t) not in new:
            new[id(t)] = torch.where(torch.isnan(t), t, torch.randn(t.shape, generator=g, dtype=F64))
        return new[id(t)]
    for v in ops.ins:
        v.t = rnd(v.t)
    ops.weight = torch.randn(ops.weight.shape, generator=g, dtype=F64)
    ops.wt = go.WEIGHT_FORMS[r.form](ops.weight).contiguous()
    return ops


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _functional(r, ops):
    """the launch's sum [N, h, w, Ncols] by torch's own convolutions / autograd in float64, from the raw tensors"""
    n, h, w = r.shape
    pad = r.taps // 9
    if r.form in ("fwd", "deconv_fwd"):
        parts = []
        for v in ops.ins:
            t = v.t[..., v.c_off:v.c_off + v.width]
            if v.scale is not None:
                t = t * v.scale + v.shift
            parts.append(F.relu(t) if v.relu else t)
        x = _nchw(torch.cat(parts, 3))
        if r.form == "fwd":
            return F.conv2d(x, ops.weight, None, padding=pad).permute(0, 2, 3, 1)
        y = F.conv_transpose2d(x, ops.weight, None, stride=2)   # [n, co, 2h, 2w] -> column (2 a + b) co + c
        return torch.cat([y[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], 1).permute(0, 2, 3, 1)
    v0 = ops.ins[0]
    if r.form == "dgrad":
        dy = _nchw(v0.t[..., v0.c_off:v0.c_off + v0.width])
        x = torch.zeros(n, r.ncols, h, w, dtype=F64, requires_grad=True)
        F.conv2d(x, ops.weight, None, padding=pad).backward(dy)
        return x.grad.permute(0, 2, 3, 1)
    d_up = _nchw(v0.t[..., v0.c_off:v0.c_off + v0.width])
    x = torch.zeros(n, r.ncols, h, w, dtype=F64, requires_grad=True)
    F.conv_transpose2d(x, ops.weight, None, stride=2).backward(d_up)
    return x.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("r", HOST_ROWS, ids=[r.id for r in HOST_ROWS])
def test_the_sum_against_torch(r):
    ops = _randomised(r, 11)
    n, h, w = r.shape
    x = torch.cat([go.load_view(v, h, w, bf16=False) for v in ops.ins], 3)
    got = go.gemm_sum(x, ops.wt)
    want = _functional(r, ops)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("r", HOST_ROWS, ids=[r.id for r in HOST_ROWS])
def test_reference_writes_the_views_and_nothing_else(r):
    """fp32 storage (no rounding): every output view holds epilogue(sum) of its columns, NaN stays NaN elsewhere"""
    ops = go.operands(r)
    n, h, w = r.shape
    e = go.reference(r, ops, 1, bf16=False)
    c0 = 0
    written = [torch.zeros_like(t, dtype=torch.bool) for t in ops.out_tensors]
    for idx, v, kind in ops.outs:
        acc = e.acc[..., c0:c0 + v.width]
        c0 += v.width
        want = acc.clone()
        old = v._cut(ops.out_tensors[idx], h, w)
        gate = None if v.gate is None else v._cut(v.gate, h, w)
        if kind == "gate":
            want = want * (gate > 0)
        if kind in ("acc", "accgate"):
            want = want + old
        if kind == "accgate":
            want = want * (gate > 0)
        assert torch.equal(v._cut(e.out_tensors[idx], h, w), want + 0.0), (r.id, kind)
        v._cut(written[idx], h, w)[...] = True
    for t0, t1, m in zip(ops.out_tensors, e.out_tensors, written):
        assert bool(torch.isnan(t1[~m]).all()) and bool(torch.isnan(t0[~m]).all())
        assert not bool(torch.isnan(t1[m]).any())


def test_bf_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(20000, generator=g) * 300, torch.arange(-1100, 1100).float(), torch.arange(-600, 600).float() / 4,
                   torch.tensor([0.0, -0.0, 255.5, 257.0, 259.0, 463.0, 3.3895e38, 1e-40])])
    want = x.to(BF).to(F64)
    got = go.bf(x.to(F64))
    assert torch.equal(got, want)
    assert float(go.bf(torch.tensor([257.0], dtype=F64))) == 256.0 and float(go.bf(torch.tensor([259.0], dtype=F64))) == 260.0
    ties = go.is_tie(torch.tensor([257.0, 258.0, 259.0, 255.5, 255.0, 513.0, 514.0], dtype=F64))
    assert ties.tolist() == [True, False, True, True, False, False, True]
    with pytest.raises(AssertionError):
        go.bf(torch.tensor([1.0 + 2.0 ** -30], dtype=F64))


def _literal(acc, bias, relu, gate, gate_sum, old, roundings):
    """the kernels' epilogues in fp32 with torch.bfloat16 casts (gemm_bf16.hip epilogue_direct / gemm_pw_bf16.hip EPI 1)"""
    v = acc.float()
    if bias is not None:
        v = v + bias.float()
    if relu:
        v = torch.clamp_min(v, 0.0)
    rmw = gate is not None or old is not None
    if roundings == 2:
        v = v.to(BF).float()
        if not rmw:
            return v.to(F64)
    if gate is not None and not gate_sum:
        v = torch.where(gate.to(BF).float() > 0, v, torch.zeros_like(v))
    if old is not None:
        v = v + old.to(BF).float()
    if gate is not None and gate_sum:
        v = torch.where(gate.to(BF).float() > 0, v, torch.zeros_like(v))
    return v.to(BF).to(F64)


@pytest.mark.parametrize("roundings", [1, 2])
def test_epilogue_sequences_against_bfloat16_casts(roundings):
    g = torch.Generator().manual_seed(9)
    shape = (4, 50, 16)
    acc = torch.randint(-600, 601, shape, generator=g).to(F64)
    bias = go.tie_bias(g, 16)
    old = torch.randint(-3, 4, shape, generator=g).to(F64)
    gate = torch.randint(-2, 3, shape, generator=g).to(F64)
    differ = 0
    for relu in (False, True):
        for gt, gs, od in ((None, False, None), (gate, False, None), (None, False, old), (gate, False, old), (gate, True, old),
                           (gate, True, None)):
            got, first = go.epilogue(acc, bias, relu, gt, gs, od, roundings)
            assert torch.equal(got, _literal(acc, bias, relu, gt, gs, od, roundings)), (relu, gs, roundings)
            other, _ = go.epilogue(acc, bias, relu, gt, gs, od, 3 - roundings)
            if od is None:
                assert torch.equal(got, other)        # without an accumulate the two rules store the same bits
            else:
                differ += int((got != other).sum())
            want_first = (acc + bias).clamp_min(0) if relu else acc + bias
            assert torch.equal(first, want_first)
    assert differ > 0
    one, _ = go.epilogue(torch.tensor([257.0], dtype=F64), None, False, None, False, torch.tensor([1.0], dtype=F64), 1)
    two, _ = go.epilogue(torch.tensor([257.0], dtype=F64), None, False, None, False, torch.tensor([1.0], dtype=F64), 2)
    assert float(one) == 258.0 and float(two) == 256.0


def test_weight_forms_are_permutations():
    for r in HOST_ROWS:
        ops = go.operands(r)
        assert ops.wt.shape == (r.taps, r.k, r.ncols)
        assert sorted(ops.wt.reshape(-1).tolist()) == sorted(ops.weight.reshape(-1).tolist())


# ------------------------------------------------------------------------------------------------ the GPU rows
MARGINS = {}


@pytest.mark.parametrize("r", go.ROWS, ids=[r.id for r in go.ROWS])
def test_row_preconditions(r):
    """Conditions of the data, not measurements: the margin (and with it exact sums of squares for statistics rows and an
    fp32 fma for fold rows, which `load_view` asserts), roundings / ties / discriminating accumulates / roundings on load
    where the row claims them, no all-zero output column, a single product per element for impulse rows, more units than
    workgroups at 8 CUs for multi rows."""
    ops = go.operands(r)
    n, h, w = r.shape
    m = go.exactness_margin(r, ops)
    MARGINS[r.id] = m
    assert m < go.EXACT_LIMIT, (r.id, m)
    bf16 = r.family != "fld"
    two, one = go.reference(r, ops, 2, bf16), go.reference(r, ops, 1, bf16)
    first = two.first
    assert not bool((first.abs().sum((0, 1, 2)) == 0).any()), "an all-zero output column"
    if r.data != "int":
        assert go.max_terms(r, ops) == 1.0
        x = torch.cat([go.load_view(v, h, w) for v in ops.ins], 3)
        full = x if r.data == "impulse_w" else ops.wt      # every mantissa bit of bf16 is in use somewhere
        bits = (full[full != 0].float().view(torch.int32) >> 16) & 0x7F
        assert len(set(bits.tolist())) == 128
    if "round" in r.claims:
        assert float((go.bf(first) != first).double().mean()) >= 0.01
    if "ties" in r.claims:
        assert int(go.is_tie(first).sum()) > 0
    if "disc" in r.claims:
        assert sum(int(((a != b) & ~torch.isnan(a)).sum()) for a, b in zip(one.out_tensors, two.out_tensors)) > 0
    else:   # rows that claim nothing of the kind must not depend on the rule either, unless they accumulate
        if not any(k in ("acc", "accgate") for _, _, k in ops.outs):
            assert all(torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
                       for a, b in zip(one.out_tensors, two.out_tensors))
    if "fold" in r.claims:
        v = ops.ins[0]
        raw = (v._cut(v.t, h, w) * v.scale + v.shift).clamp_min(0.0)
        assert int((go.bf(raw) != raw).sum()) > 0 and int(go.is_tie(raw).sum()) > 0
    if r.multi:
        for variant in r.variants:
            p = go.launch_plan(r, variant, 8)
            assert p["units"] > p["workers"], (variant, p["units"], p["workers"])


def test_largest_margin():
    """the figure the commit message states (margins computed by test_row_preconditions are reused)"""
    for r in go.ROWS:
        if r.id not in MARGINS:
            MARGINS[r.id] = go.exactness_margin(r, go.operands(r))
    mine = {r.id: MARGINS[r.id] for r in go.ROWS}
    worst = max(mine, key=mine.get)
    plain = {r.id: MARGINS[r.id] for r in go.ROWS if not r.stats}
    print("largest margin: %.4g (%s); without the scaled sums of squares: %.4g (%s); limit %.4g" % (
        MARGINS[worst], worst, max(plain.values()), max(plain, key=plain.get), go.EXACT_LIMIT))
    assert MARGINS[worst] < go.EXACT_LIMIT


# ------------------------------------------------------------------------------------------------ the launchers' choices
def _plan(rid, variant, cus=256):
    r = next(r for r in go.ROWS if r.id == rid)
    return go.launch_plan(r, variant, cus)


EXPECTED = [   # (row, variant) -> instantiation, written out by hand from the launchers
    ("k9-32-32-plain-multi", "dma4", "gemm_bf16_dma_kernel<9> waves=4 tw=32 NT=1 rw"),
    ("k9-32-32-plain-multi", "dma8", "gemm_bf16_dma_kernel<9> waves=8 tw=32 NT=1 resident"),
    ("k9-32-32-plain-multi", "reg", "gemm_bf16_kernel<9> tw=32 NT=1"),
    ("k9-32-32-stats-multi", "dma8", "gemm_bf16_dma_kernel<9> waves=4 tw=32 NT=1 STATS rw"),     # no 8-wave statistics form
    ("k9-32-32-stats-multi", "reg", "gemm_bf16_kernel<9> tw=32 NT=1 STATS"),
    ("k9-32-32-ties-tw8", "dma4", "gemm_bf16_dma_kernel<9> waves=4 tw=8 NT=1 rw"),
    ("k9-32-32-relu-ties-tw16", "reg", "gemm_bf16_kernel<9> tw=16 NT=1"),
    ("k9-cat192-64", "dma8", "gemm_bf16_dma_kernel<9> waves=8 tw=32 NT=2 streamed"),            # 6 chunks: not resident
    ("k9-cat192-64", "reg", "gemm_bf16_kernel<9> tw=32 NT=2"),
    ("k9-64-96-odd-tiles", "dma8", "gemm_bf16_dma_kernel<9> waves=8 tw=32 NT=1 streamed"),
    ("k9-64-96-odd-tiles", "reg", "gemm_bf16_kernel<9> tw=32 NT=1"),
    ("k9-64-64-multi", "dma8", "gemm_bf16_dma_kernel<9> waves=8 tw=32 NT=2 resident"),           # one group x two chunks <= 2 slots
    ("k9-128-32-resident", "dma8", "gemm_bf16_dma_kernel<9> waves=8 tw=32 NT=1 resident"),       # four chunks in four slots
    ("k9-partial-tw16", "dma4", "gemm_bf16_kernel<9> tw=16 NT=1"),                               # 16 / 8 / 40-channel views: refused
    ("k9-dgrad-kinds-multi", "reg", "gemm_bf16_kernel<9> tw=32 NT=2"),
    ("k9-dgrad-kinds-multi", "dma4", "gemm_bf16_dma_kernel<9> waves=4 tw=32 NT=1 rw"),
    ("k9-fold-exact", "reg", "gemm_bf16_kernel<9> tw=32 NT=2"),
    ("k1-deconv-fwd-64-32", "dma4", "gemm_bf16_dma_kernel<1> waves=4 tw=32 NT=2 plain"),
    ("k1-deconv-dgrad-accgate", "dma4", "gemm_bf16_dma_kernel<1> waves=4 tw=32 NT=2 rw"),
    ("k1-conv-64-32-one-tile-multi", "dma4", "gemm_bf16_dma_kernel<1> waves=4 tw=32 NT=1 plain"),  # the one-tile weight slot
    ("k1-deconv-dgrad-one-tile-tw16", "dma4", "gemm_bf16_dma_kernel<1> waves=4 tw=16 NT=1 rw"),
    ("k1-conv-128-96-relu", "reg", "gemm_bf16_kernel<1> tw=32 NT=1"),
    ("k1-fold-exact", "reg", "gemm_bf16_kernel<1> tw=16 NT=2"),
    ("pw-plain-q1-c1-w16", "pw", "gemm_pw_bf16_kernel QC=1 NCBP=1 EPI=0 threads=256 kchunk=1 pass=1"),
    ("pw-plain-q8-c8-w48", "pw", "gemm_pw_bf16_kernel QC=8 NCBP=8 EPI=0 threads=1024 kchunk=1 pass=1"),
    ("pw-rmw-q8-c8-w48", "pw", "gemm_pw_bf16_kernel QC=8 NCBP=4 EPI=1 threads=1024 kchunk=1 pass=2"),   # the ncbp 8 -> 4 rewrite
    ("pw-rmw-q4-c8-w16", "pw", "gemm_pw_bf16_kernel QC=4 NCBP=4 EPI=1 threads=512 kchunk=1 pass=2"),
    ("pw-kchunk2-plain", "pw", "gemm_pw_bf16_kernel QC=8 NCBP=2 EPI=0 threads=512 kchunk=2 pass=1"),
    ("pw-kchunk2-rmw", "pw", "gemm_pw_bf16_kernel QC=8 NCBP=2 EPI=1 threads=512 kchunk=2 pass=1"),
    ("pw-pass2-plain", "pw", "gemm_pw_bf16_kernel QC=2 NCBP=8 EPI=0 threads=512 kchunk=1 pass=2"),
    ("pw-pass4-rmw", "pw", "gemm_pw_bf16_kernel QC=2 NCBP=4 EPI=1 threads=512 kchunk=1 pass=4"),
    ("pw-relu-only", "pw", "gemm_pw_bf16_kernel QC=2 NCBP=2 EPI=1 threads=256 kchunk=1 pass=1"),    # a ReLU is no plain store
    ("pw-refuse-k96", "pw", "gemm_bf16_dma_kernel<1> waves=4 tw=32 NT=1 plain"),
    ("pw-refuse-w20", "pw", "gemm_bf16_dma_kernel<1> waves=4 tw=32 NT=2 plain"),
    ("pw-refuse-fold", "pw", "gemm_bf16_kernel<1> tw=32 NT=2"),
    ("pw-refuse-lds", "pw", "gemm_bf16_dma_kernel<1> waves=4 tw=16 NT=2 plain"),
    ("small-c3-stats", "small", "small_cin_fwd_kernel C=3 stats"),
    ("fld-c4", "fld", "first_layer_dgrad_bf16 C=4"),
]


@pytest.mark.parametrize("rid,variant,key", EXPECTED, ids=["%s-%s" % e[:2] for e in EXPECTED])
def test_launch_plan_gives_the_instantiation(rid, variant, key):
    p = _plan(rid, variant)
    assert p["key"] == key
    assert key.startswith(p["label"])
    if rid in go.PW_REFUSED:
        assert p["label"] == go.PW_REFUSED[rid]


def test_launch_plan_formulas():
    """the unit and workgroup counts of the launchers at 8 and at 256 CUs, and the pointwise kernel's limits"""
    assert go.tile_geom(5, 7)[0] == 3 and go.tile_geom(20, 16)[0] == 4 and go.tile_geom(37, 21) == (5, 1, 5)
    p = _plan("k9-32-32-plain-multi", "dma8", 8)
    assert (p["units"], p["workers"]) == (2 * 3 * 3, 8)               # 16 x 32 patches, one workgroup per CU
    p = _plan("k9-32-32-plain-multi", "dma4", 8)
    assert (p["units"], p["workers"]) == (2 * 5 * 3, 16)              # 8 x 32 patches, two per CU
    p = _plan("k9-dgrad-kinds-multi", "reg", 8)
    assert (p["units"], p["workers"]) == (30 * 2, 16)                 # four column tiles, two per unit
    p = _plan("k9-dgrad-kinds-multi", "dma4", 8)
    assert (p["units"], p["workers"]) == (30 * 4, 16)                 # the 4-wave form takes one tile per unit
    p = _plan("k1-deconv-fwd-multi", "dma4", 8)
    assert (p["units"], p["workers"]) == (30 * 2, 24)                 # plain pointwise stores: three per CU
    p = _plan("k1-deconv-dgrad-multi", "dma4", 8)
    assert (p["units"], p["workers"]) == (30, 16)
    p = _plan("k9-32-32-plain-multi", "reg", 13)
    assert p["workers"] == 24                                          # (2 x 13) & ~7
    p = _plan("pw-multi-1024", "pw", 8)
    assert (p["threads"], p["lds"], p["units"], p["workers"]) == (1024, 256 * 256 * 2 + 1024, 38, 8)
    p = _plan("pw-multi-plain", "pw", 8)
    assert (p["threads"], p["units"], p["workers"], p["tiles_x"]) == (256, 60, 32, 3)
    assert [go.pwb_block_count(u) for u in (1, 2, 3, 4, 5, 6, 8, 12, 16, 24)] == [1, 2, 0, 4, 0, 0, 8, 0, 8, 8]
    big = row("x", "pw", (1, 3, 16), "fwd", [256], [288], taps=1, variants=["pw"])
    assert go.pw_plan(big) is None                                     # N / 32 = 9
    edge = row("x", "pw", (1, 3, 16), "fwd", [256], [256], taps=1, variants=["pw"])
    assert go.pw_plan(edge)["lds"] <= 148 * 1024 < go.pw_plan(edge)["lds"] * 2
    assert go.pw_plan(next(r for r in go.ROWS if r.id == "pw-refuse-lds")) is None


def test_the_rows_cover_the_dispatch_space():
    keys = {go.launch_plan(r, v, 256)["key"] for r, v, _ in go.cells()}
    for q in (1, 2, 4, 8):
        for c in (1, 2, 4, 8):
            assert any(k.startswith("%s QC=%d NCBP=%d EPI=0 " % (go.PWB, q, c)) for k in keys), (q, c)
            if c < 8:
                assert any(k.startswith("%s QC=%d NCBP=%d EPI=1 " % (go.PWB, q, c)) for k in keys), (q, c)
    assert {int(k.split("threads=")[1].split()[0]) for k in keys if k.startswith(go.PWB)} == {256, 512, 1024}
    assert any("kchunk=2" in k for k in keys) and any("pass=2" in k for k in keys)
    widths = {r.shape[2] // 16 for r in go.PW_ROWS if go.pw_plan(r) is not None}
    assert {1, 2, 3} <= widths                                         # tiles_x 3 is no power of two
    for tw in (8, 16, 32):
        for stats in ("", " STATS"):
            assert "%s waves=4 tw=%d NT=1%s rw" % (go.DMA9, tw, stats) in keys
            assert "%s tw=%d NT=1%s" % (go.REG9, tw, stats) in keys
    for k in ("%s waves=8 tw=32 NT=1 resident", "%s waves=8 tw=32 NT=1 streamed", "%s waves=8 tw=32 NT=2 resident",
              "%s waves=8 tw=32 NT=2 streamed"):
        assert k % go.DMA9 in keys
    for nt in (1, 2):
        assert any(k.startswith("%s tw=" % go.REG9) and "NT=%d" % nt in k for k in keys)
        for rw in ("plain", "rw"):
            assert any(k.startswith(go.DMA1) and ("NT=%d %s" % (nt, rw)) in k for k in keys), (nt, rw)
        assert any(k.startswith(go.REG1) and "NT=%d" % nt in k for k in keys)
    for c in (1, 3, 4):
        for st in ("plain", "stats"):
            assert "%s C=%d %s" % (go.SMALL, c, st) in keys
    for c in (1, 2, 3, 4):
        assert "%s C=%d" % (go.FLD, c) in keys
    multi = {go.launch_plan(r, v, 8)["label"] for r, v, _ in go.cells() if r.multi}
    assert multi == {go.REG9, go.REG1, go.DMA9, go.DMA1, go.PWB, go.SMALL}


# ------------------------------------------------------------------------------------------------ the fp32 rows
def _fp32_rows():
    from tests.test_gpu_gemm_fp32_exact import FP32_ROWS
    return FP32_ROWS


@pytest.mark.parametrize("r", _fp32_rows(), ids=[r.id for r in _fp32_rows()])
def test_fp32_row_preconditions(r):
    """tests/test_gpu_gemm_fp32_exact.py: the same margin; rows that run the Winograd kernel also through its transforms
    (helpers.wino_magnitude on |x| and |w|, against the same 2^22); impulse rows add a single product per element"""
    from tests.helpers import wino_magnitude
    from tests.test_gpu_gemm_fp32_exact import fp32_operands
    ops = fp32_operands(r)
    n, h, w = r.shape
    assert go.exactness_margin(r, ops) < go.EXACT_LIMIT
    e = go.reference(r, ops, 1, bf16=False)
    assert not bool((e.first.abs().sum((0, 1, 2)) == 0).any())
    assert all(go.fp32_exact(t) for t in e.out_tensors)
    if r.data != "int":
        assert go.max_terms(r, ops) == 1.0
    if any(v.startswith("wino") for v in r.variants):
        x = torch.cat([go.load_view(v, h, w, bf16=False) for v in ops.ins], 3).abs().permute(0, 3, 1, 2)
        wk = ops.wt.abs().view(3, 3, r.k, r.ncols).permute(3, 2, 0, 1)      # [o, i, r, s] of the equivalent convolution
        m = wino_magnitude(x, wk, None if ops.bias is None else ops.bias.abs())
        old = sum(float(t[~torch.isnan(t)].abs().max()) for t in ops.out_tensors if bool((~torch.isnan(t)).any()))
        assert float(m.max()) + old < go.EXACT_LIMIT
        MARGINS["wino/" + r.id] = float(m.max()) + old
    if r.multi:
        assert go.fast_geometry(r)["patches"] > 16      # more patches than the 16 workgroups of 8 CUs
