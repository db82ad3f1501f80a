"""The plant list of tests/test_gpu_nonfinite.py on the CPU (tests/nonfinite_oracle.py): for every plant the reference's
non-finite set R is not empty and lies inside the footprint F, and for every activation plant at least half of the
launch's output lies outside F -- so that neither rule of DESIGN.md 5f.1 can pass on the GPU without having looked at
anything.  Also: the footprints against a brute-force statement of what a window reads, the pool winner rule against
torch.max_pool2d, and the ReLU restatement against torch.relu.
"""
import math

import pytest
import torch

from tests import nonfinite_oracle as nf
from tests.wgrad_oracle import F64

CELLS = [(r, v) for r in nf.ROWS for v in r.variants]
_OPS = {}


def _operands(r):
    if r.id not in _OPS:
        _OPS[r.id] = nf.operands(r)
    return _OPS[r.id]


def _nonfinite_sets(r, ops, p):
    res, stats = nf.reference(r, nf.planted(r, ops, p), nf.is_bf16(r) and r.family != "fld")
    base, _ = nf.reference(r, ops, nf.is_bf16(r) and r.family != "fld")
    # an output tensor starts as NaN where the launch writes nothing: R is what the plant ADDS
    return [~torch.isfinite(a) & torch.isfinite(b) for a, b in zip(res, base)], stats


@pytest.mark.parametrize("r", nf.ROWS, ids=[r.id for r in nf.ROWS])
def test_reference_sets_and_footprints_of_every_plant(r):
    ops = _operands(r)
    plants = nf.plants(r, ops)
    assert len({p.id for p in plants}) == len(plants), "plant ids must be unique"
    wheres = {p.where for p in plants}
    assert "x" in wheres and {"interior", "corner", "last"} <= {p.tag for p in plants}
    for p in plants:
        R, _ = _nonfinite_sets(r, ops, p)
        n_r = sum(int(m.sum()) for m in R)
        if p.where in ("x_off", "gate_off"):
            assert n_r == 0, (r.id, p.id, "a plant nothing reads reached the reference's output")
            continue
        assert n_r > 0, (r.id, p.id, "R is empty")
        for variant in r.variants:
            F, rows, outside = nf.footprint(r, ops, p, variant)
            for m_r, m_f in zip(R, F):
                assert not bool((m_r & ~m_f).any()), (r.id, p.id, variant, "R leaves F")
            assert bool(rows.any())
            if p.where == "x":
                assert outside >= 0.5, (r.id, p.id, variant, outside)


def test_every_value_and_position_is_planted_somewhere():
    seen_f32, seen_bf16, tags = set(), set(), set()
    for r in nf.ROWS:
        for p in nf.plants(r, _operands(r)):
            tags.add(p.where if p.where != "x" else p.tag)
            if p.where == "x" and nf.is_bf16(r) and r.family != "small":
                seen_bf16.add(p.value)
            else:
                seen_f32.add(p.value)
    assert seen_f32 == set(nf.VALUES) and seen_bf16 == set(nf.BF16_VALUES)
    assert {"interior", "corner", "last", "unit2", "slice-first", "slice-last", "x_off", "gate_off", "weight", "bias", "scale",
            "shift"} <= tags, tags
    for name in nf.NANS:
        assert math.isnan(nf.as_float(name))


def _reads(shape, taps, pos, wino):
    """brute force: the output pixels whose window (direct: 3x3 / 1x1 around the pixel; Winograd: the 4x4 input tile of
    the pixel's 2x2 output tile) holds `pos`"""
    n, h, w = shape
    b, py, px = pos
    m = torch.zeros(n, h, w, dtype=torch.bool)
    for y in range(h):
        for x in range(w):
            if wino:
                ys, xs = range(2 * (y // 2) - 1, 2 * (y // 2) + 3), range(2 * (x // 2) - 1, 2 * (x // 2) + 3)
            else:
                rr = 1 if taps == 9 else 0
                ys, xs = range(y - rr, y + rr + 1), range(x - rr, x + rr + 1)
            m[b, y, x] = py in ys and px in xs
    return m


@pytest.mark.parametrize("shape", [nf.G57, nf.G2016, (1, 6, 9)])
def test_footprints_against_brute_force(shape):
    n, h, w = shape
    for pos in [(0, 0, 0), (n - 1, h - 1, w - 1), (n - 1, h // 2, w // 2), (0, h - 1, 0), (0, 1, w - 2), (0, h - 2, 1)]:
        for taps in (9, 1):
            assert torch.equal(nf.footprint_direct(shape, taps, pos), _reads(shape, taps, pos, False)), (shape, pos, taps)
        fw = nf.footprint_wino(shape, pos)
        assert torch.equal(fw, _reads(shape, 9, pos, True)), (shape, pos)
        assert not bool((nf.footprint_direct(shape, 9, pos) & ~fw).any()), "the direct footprint lies inside the tile footprint"
        assert int(fw.sum()) <= 16


def test_patches_of():
    pix = torch.zeros(nf.G2016, dtype=torch.bool)    # 16 x 16 patches: two rows of patches per image, the second ragged
    pix[1, 15, 3] = pix[1, 16, 3] = True
    assert nf.patches_of(nf.G2016, pix).tolist() == [False, False, True, True]
    pix = torch.zeros(nf.G4072, dtype=torch.bool)    # 8 x 32 patches: 5 x 3 per image
    pix[1, 10, 70] = True
    assert nf.patches_of(nf.G4072, pix).nonzero().flatten().tolist() == [20]


def test_pool_winner_rule_and_relu_against_torch():
    g = torch.Generator().manual_seed(5)
    act = torch.randint(-3, 4, (2, 6, 8, 5), generator=g).to(F64)       # ties everywhere: the first maximum must win
    nan = float("nan")
    act[0, 0, 0, 0] = nan                       # first of the window
    act[0, 1, 3, 1] = nan                       # last of the window
    act[0, 2, 4, 2] = act[0, 3, 5, 2] = nan     # two in one window: the last keeps it
    act[1, 4, 6, 3] = float("inf")
    act[1, 5, 7, 4] = float("-inf")
    pooled, idx = nf.pool_reference(act)
    want, widx = torch.nn.functional.max_pool2d(act.permute(0, 3, 1, 2), 2, return_indices=True)
    want, widx = want.permute(0, 2, 3, 1), widx.permute(0, 2, 3, 1)
    assert torch.equal(torch.isnan(pooled), torch.isnan(want)) and int(torch.isnan(pooled).sum()) == 3
    assert torch.equal(pooled[~torch.isnan(want)], want[~torch.isnan(want)])
    w = act.shape[2]
    oy = 2 * torch.arange(3).view(1, -1, 1, 1) + idx // 2
    ox = 2 * torch.arange(4).view(1, 1, -1, 1) + idx % 2
    assert torch.equal(oy * w + ox, widx), "winner indices (NaN windows included) are torch's"
    assert int(idx[0, 0, 0, 0]) == 0 and int(idx[0, 0, 1, 1]) == 3 and int(idx[0, 1, 2, 2]) == 3
    v = torch.tensor([nan, -nan, float("inf"), float("-inf"), -0.0, 0.0, -1.5, 2.5], dtype=F64)
    got, ref = nf.relu_keep_nan(v), torch.relu(v)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[2:], ref[2:])
    assert not bool(torch.signbit(got[4])), "-0 becomes +0"
