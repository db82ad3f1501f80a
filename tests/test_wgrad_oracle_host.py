"""tests/wgrad_oracle.py against autograd, a float32 restatement of the Winograd weight gradient against the oracle,
and the exactness precondition of every GPU case row (tests/test_gpu_wgrad_exact.py).  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_oracle as wo
from tests.test_gpu_wgrad_exact import TIER_A, TIER_B
from tests.wgrad_oracle import case

F64 = torch.float64

HOST_CASES = [
    case("plain9", "-", (2, 9, 11), [5], 6, ()),
    case("plain1", "-", (2, 9, 11), [5], 6, (), taps=1),
    case("sliced", "-", (2, 7, 10), [(12, 4, 5)], (9, 2, 6), ()),
    case("concatenated", "-", (1, 8, 9), [3, 8, 2], 7, ()),
    case("folded", "-", (2, 7, 10), [8, 4], 5, (), fold=(True, False)),
    case("gated", "-", (2, 7, 10), [6], (9, 2, 6), (), gate=True),
    case("four-phase", "-", (2, 5, 6), [7], 3, (), taps=1, deconv=True),
    case("four-phase-sliced-padded", "-", (2, 5, 6), [(9, 1, 7)], (8, 2, 3), (), taps=1, deconv=True, dy_pad=1, gate=True),
]


def _autograd(c, ops):
    """(dW in torch layout, flattened; db) by F.conv2d / F.conv_transpose2d backward in float64, from the raw tensors"""
    n, h, w = c.shape
    parts = []
    for v in ops.xs:
        t = v.t[..., v.c_off:v.c_off + v.width]
        if v.scale is not None:
            t = t * v.scale + v.shift
        parts.append(F.relu(t) if v.relu else t)
    x = torch.cat(parts, 3).permute(0, 3, 1, 2).contiguous()
    _, c_off, co = c.dy
    d0 = ops.dys[0]
    hh, ww = (2 * h, 2 * w) if c.deconv else (h, w)
    dy = d0.t[:, :hh, :ww, c_off:c_off + co]
    if d0.gate is not None:
        dy = dy * (d0.gate[:, :hh, :ww, c_off:c_off + co] > 0)
    dy = dy.permute(0, 3, 1, 2).contiguous()
    wt = torch.zeros(c.dw_shape, dtype=F64, requires_grad=True)
    bias = torch.zeros(co, dtype=F64, requires_grad=True)
    y = F.conv_transpose2d(x, wt, bias, stride=2) if c.deconv else F.conv2d(x, wt, bias, padding=c.taps // 9)
    y.backward(dy)
    return wt.grad.reshape(-1), bias.grad


def _randomise(ops, seed):
    """the same views over full-mantissa random data (NaN poison kept where it was)"""
    g = torch.Generator().manual_seed(seed)
    new = {}

    def rnd(t):
        if id(t) not in new:
            new[id(t)] = torch.where(torch.isnan(t), t, torch.randn(t.shape, generator=g, dtype=F64))
        return new[id(t)]
    for v in ops.xs + ops.dys:
        v.t = rnd(v.t)
        if v.gate is not None:
            v.gate = rnd(v.gate)
        if v.scale is not None:
            v.scale, v.shift = rnd(v.scale), rnd(v.shift)
    return ops


@pytest.mark.parametrize("c", HOST_CASES, ids=[c.id for c in HOST_CASES])
def test_oracle_equals_autograd_on_integers(c):
    ops = wo.integer_operands(c)
    dw, db = wo.reference(c, ops)
    adw, adb = _autograd(c, ops)
    assert torch.equal(dw, adw) and torch.equal(db, adb)
    assert float(dw.abs().max()) > 0 and float(db.abs().max()) > 0


@pytest.mark.parametrize("c", HOST_CASES, ids=[c.id for c in HOST_CASES])
def test_oracle_matches_autograd_on_random_data(c):
    ops = _randomise(wo.integer_operands(c), 7)
    dw, db = wo.reference(c, ops)
    adw, adb = _autograd(c, ops)
    assert float((dw - adw).abs().max()) <= 1e-12 * float(adw.abs().max())
    assert float((db - adb).abs().max()) <= 1e-12 * float(adb.abs().max())


def test_winograd_planes_of_the_oracle_give_the_direct_sum():
    """G^T [ sum (B^T d B) . (A dY A^T) ] G with the unsigned last row and the finish's signs = the nine shifted sums"""
    c = case("wino-id", "-", (2, 7, 9), [5], 4, ())   # odd H and W: ragged 2x2 tiles
    ops = wo.integer_operands(c)
    x, dy = wo.concat(ops.xs, 7, 9), wo.concat(ops.dys, 7, 9)
    assert torch.equal(wo.wino_finish(wo.wino_planes(x, dy)), wo.shifted_sums(x, dy, 9))


# ---------------------------------------------------------------------------------------- float32 Winograd restatement
def _wino_f32(x, dy, n_split, seed):
    """csrc/wgrad_wino.hip in numpy float32: B^T d B by a column and a row pass of single adds, A dY A^T with the unsigned
    last row, one product per (tile, plane, channel, column) added to one of n_split slabs in a SHUFFLED tile order, the
    slabs summed, then the finish's two fused chains with the sign in G's last row.  Returns ([9, K, C] float32, db,
    the largest transform-domain |sum| seen)."""
    f = np.float32
    x, dy = x.astype(f), dy.astype(f)
    n, h, w, k = x.shape
    nc = dy.shape[3]
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = np.zeros((n, 2 * th + 2, 2 * tw + 2, k), f)
    xp[:, 1:h + 1, 1:w + 1] = x
    yp = np.zeros((n, 2 * th, 2 * tw, nc), f)
    yp[:, :h, :w] = dy
    d = [[xp[:, a:a + 2 * th:2, b:b + 2 * tw:2].reshape(-1, k) for b in range(4)] for a in range(4)]
    t = [[None] * 4 for _ in range(4)]
    for b in range(4):   # column pass
        t[0][b], t[1][b], t[2][b], t[3][b] = d[0][b] - d[2][b], d[1][b] + d[2][b], d[2][b] - d[1][b], d[1][b] - d[3][b]
    v = []
    for i in range(4):   # row pass
        v += [t[i][0] - t[i][2], t[i][1] + t[i][2], t[i][2] - t[i][1], t[i][1] - t[i][3]]
    e = [[yp[:, p::2, q::2].reshape(-1, nc) for q in range(2)] for p in range(2)]
    rows = [(e[0][0], e[0][1]), (e[0][0] + e[1][0], e[0][1] + e[1][1]), (e[0][0] - e[1][0], e[0][1] - e[1][1]), (e[1][0], e[1][1])]
    m = []
    for left, right in rows:
        m += [left, left + right, left - right, right]
    v_all, m_all = np.stack(v, 1), np.stack(m, 1)   # [tiles, 16, K], [tiles, 16, C]
    assert v_all.dtype == f and m_all.dtype == f
    tiles = v_all.shape[0]
    slabs = np.zeros((n_split, 16, k, nc), f)
    dbs = np.zeros((n_split, nc), f)
    for j, ti in enumerate(np.random.default_rng(seed).permutation(tiles)):
        slabs[j % n_split] += v_all[ti][:, :, None] * m_all[ti][:, None, :]
        dbs[j % n_split] += m_all[ti][5]   # plane (1, 1): the plain sum of the 2x2 tile
    u = np.zeros((16, k, nc), f)
    db = np.zeros(nc, f)
    for s in range(n_split):
        u += slabs[s]
        db += dbs[s]
    seen = float(np.abs(slabs).max())
    out = np.zeros((9, k, nc), f)
    for r in range(3):
        for cc in range(3):
            gr = [f(r == 0), f(0.5), f(-0.5 if r == 1 else 0.5), f(-1.0 if r == 2 else 0.0)]
            gc = [f(cc == 0), f(0.5), f(-0.5 if cc == 1 else 0.5), f(-1.0 if cc == 2 else 0.0)]
            acc = np.zeros((k, nc), f)
            for aa in range(4):
                rowsum = np.zeros((k, nc), f)
                for bb in range(4):
                    rowsum = gc[bb] * u[4 * aa + bb] + rowsum   # (products by 0, +-0.5, +-1 are exact: one rounding, as fmaf)
                acc = gr[aa] * rowsum + acc
            out[3 * r + cc] = acc
    assert out.dtype == f
    return out, db, max(seen, float(np.abs(u).max()))


@pytest.mark.parametrize("shape,fold,n_split", [((5, 40, 96), False, 7), ((2, 25, 97), False, 3), ((1, 17, 33), False, 1),
                                                ((2, 25, 97), True, 5)])
def test_float32_winograd_restatement_is_bit_equal_on_integers(shape, fold, n_split):
    c = case("f32-wino-%dx%dx%d-%d" % (shape + (fold,)), "wgrad_wino_kernel", shape, [8], 8, (), fold=fold)
    ops = wo.integer_operands(c)
    n, h, w = shape
    x, dy = wo.concat(ops.xs, h, w), wo.concat(ops.dys, h, w)
    want_dw, want_db = wo.reference(c, ops)
    got, db, seen = _wino_f32(x.numpy(), dy.numpy(), n_split, seed=shape[1])
    got_dw = wo.scatter_dw(torch.from_numpy(got).double(), c.dw_strides, c.n_inner)
    assert torch.equal(got_dw, want_dw)
    assert torch.equal(torch.from_numpy(db).double(), want_db)
    margin = wo.exactness_margin(c, ops)
    assert seen <= margin < wo.EXACT_LIMIT, (seen, margin)


# ---------------------------------------------------------------------------------------- the GPU tables
def test_case_ids_are_unique_and_splits_fit():
    ids = [c.id for c in TIER_A + TIER_B]
    assert len(ids) == len(set(ids))
    for c in TIER_A + TIER_B:
        assert c.splits and all(1 <= s <= c.max_split for s in c.splits), (c.id, c.splits, c.max_split)
        n, h, w = c.shape
        assert n * h * w <= 20000, c.id


@pytest.mark.parametrize("c", TIER_A, ids=[c.id for c in TIER_A])
def test_gpu_case_rows_satisfy_the_exactness_margin(c):
    """the precondition of the equality the GPU test demands: no accumulator sees 2^22 or more in absolute terms"""
    ops = wo.integer_operands(c)
    margin = wo.exactness_margin(c, ops)
    assert 0 < margin < wo.EXACT_LIMIT, (c.id, margin)
    for v in ops.xs + ops.dys:   # operands are integers (x after the fold: multiples of 1/2), bf16 values
        lv = v.logical(*c.shape[1:])
        assert torch.equal(lv * 2, (lv * 2).round()) and float(lv.abs().max()) <= 10
        assert torch.equal(lv.bfloat16().double(), lv)


@pytest.mark.parametrize("c", [c for c in TIER_B if c.shape == (2, 25, 97)][:6] + [c for c in TIER_B if c.label == "wgrad_pw_kernel"],
                         ids=lambda c: c.id)
def test_impulse_reference_is_a_copy_of_the_window(c):
    n, h, w = c.shape
    for chunk in range(wo.impulse_chunks(c)):
        ops, pairs = wo.impulse_operands(c, chunk)
        dw, db = wo.reference(c, ops)
        x = torch.nn.functional.pad(wo.concat(ops.xs, h, w), (0, 0, 1, 1, 1, 1))
        want = torch.zeros((c.dy[2], c.k) + c.dw_shape[2:], dtype=F64)
        for j, ((i, y, xx), col) in enumerate(pairs):
            if c.gate and j == 0:
                continue   # gated off: the column stays zero
            win = x[i, y:y + 3, xx:xx + 3] if c.taps == 9 else x[i, y + 1:y + 2, xx + 1:xx + 2]
            want[col] = win.permute(2, 0, 1)
        assert torch.equal(dw, want.reshape(-1))
        assert torch.equal(dw.float().double(), dw)   # fp32 values: a direct-sum kernel can return them unchanged
