"""Top-k focal loss on the GPU (csrc/topk_loss.hip, ops.topk_focal_heads, losses.TopKFocalLoss_BCE_2d) against the
numpy oracle (tests/topk_oracle.py): kth bit for bit, every selected gradient inside its a-priori interval, every other
gradient exactly +0.0, the loss inside its bound; ties in index order; the focal kernel's bits on the selected elements;
the heads form against the written-out loop; the wiring into train_step, validate_step and GraphedTrainStep."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_oracle as lo, topk_oracle as TO

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _abi_topk(dev, preds, target, k, denom, gamma, want_grad=True):
    """unetpp_topk_focal_heads through the C ABI on [R, P] numpy inputs, with a NaN guard behind every grad
    -> (loss [1 + heads], [grad [R, P]] or None, kth [heads, R]) as numpy"""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    from unet_nested4tiny_objects_keypoints_amd.ops import _ptr, _stream, check
    lib = _lib.lib()
    rows, pixels = target.shape
    n = rows * pixels
    td = torch.from_numpy(target).to(dev)
    pd = [torch.from_numpy(p).to(dev) for p in preds]
    ws = torch.empty(int(lib.unetpp_topk_focal_workspace_bytes(len(preds), rows, pixels)) // 4, dtype=torch.float32, device=dev)
    loss = torch.empty(1 + len(preds), dtype=torch.float32, device=dev)
    kth = torch.empty(len(preds), rows, dtype=torch.float32, device=dev)
    bufs = [torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev) for _ in preds] if want_grad else None
    hd = _lib.FocalHeads()
    hd.n_heads = len(preds)
    for i, p in enumerate(pd):
        hd.pred[i] = p.data_ptr()
        hd.grad[i] = bufs[i].data_ptr() if want_grad else None
    check(lib.unetpp_topk_focal_heads(C.byref(hd), _ptr(td), rows, pixels, int(k), int(denom), float(gamma), _ptr(ws),
                                      _ptr(kth), _ptr(loss), _stream()), "unetpp_topk_focal_heads")
    torch.cuda.synchronize()
    grads = None
    if want_grad:
        for b in bufs:
            assert bool(torch.isnan(b[n:]).all()), "the guard behind grad was written"
        grads = [b[:n].cpu().numpy().reshape(rows, pixels) for b in bufs]
    return loss.cpu().numpy(), grads, kth.cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------------------------------------------- T1
@pytest.mark.parametrize("size_average", [False, True])
@pytest.mark.parametrize("gamma", [3, 2])
@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (1, 2, 1, 7), (2, 2, 5, 13), (1, 3, 17, 241), (3, 1, 64, 64)])
def test_shapes_and_k(dev, shape, gamma, size_average):
    """P = 1, 7, 65, 4097, 4096 (row bases unaligned for the odd ones); k in {1, 2, P-1, P, P+5}, fraction in {0.01, 0.5}"""
    import math
    rows, pixels = shape[0] * shape[1], shape[2] * shape[3]
    (pred,), target = TO.random_inputs(rows, pixels, seed=pixels)
    ks = sorted({k for k in (1, 2, pixels - 1, pixels, pixels + 5, max(1, math.ceil(0.01 * pixels)),
                             max(1, math.ceil(0.5 * pixels))) if k >= 1})
    failures, worst = [], 0.0
    for k in ks:
        k_eff = min(k, pixels)
        denom = rows * k_eff if size_average else rows
        want = TO.expected(pred, target, k, gamma, denom)
        loss, grads, kth = _abi_topk(dev, [pred], target, k, denom, gamma)
        bad = TO.check(want, grads[0], kth[0], loss[1])
        if loss[0].view(U32) != loss[1].view(U32):
            bad.append("one head: loss[0] %r is not loss[1] %r" % (loss[0], loss[1]))
        loss_v, none, kth_v = _abi_topk(dev, [pred], target, k, denom, gamma, want_grad=False)     # validation: no grad buffer
        if none is not None or not np.array_equal(loss_v.view(U32), loss.view(U32)) or not np.array_equal(kth_v.view(U32), kth.view(U32)):
            bad.append("want_grad = False gives another loss or kth")
        worst = max(worst, lo.loss_ratio(loss[1], want.loss))
        failures += ["k = %d: %s" % (k, m) for m in bad]
    print("topk shapes:", shape, "gamma", gamma, "size_average", size_average, "k", ks, "worst loss ratio %.3g" % worst)
    assert not failures, failures


# --------------------------------------------------------------------------------------------------------------- T2
def test_all_equal_row_takes_the_first_indices(dev):
    pred, target = TO.tie_inputs(2, 300, [(0, 300)], seed=1)
    want = TO.expected(pred, target, 5, 3, 2)
    loss, grads, kth = _abi_topk(dev, [pred], target, 5, 2, 3)
    assert TO.check(want, grads[0], kth[0], loss[1]) == []
    for r in range(2):
        assert np.flatnonzero(grads[0][r]).tolist() == [0, 1, 2, 3, 4]
    assert np.all(kth == F32(0.25))


@pytest.mark.parametrize("k,first,last", [(43, 3, 0), (49, 5, 4)])
def test_k_cuts_a_tie_run_in_the_middle(dev, k, first, last):
    """tie runs at 62..66 and 290..299 (the row's end), 40 larger elements: k = 43 takes 62..64, k = 49 also 290..293"""
    preds, target, _ = TO.cut_inputs(heads=1)
    want = TO.expected(preds[0], target, k, 3, 3)
    loss, grads, kth = _abi_topk(dev, preds, target, k, 3, 3)
    assert TO.check(want, grads[0], kth[0], loss[1]) == []
    ties = (np.abs(preds[0] - target) == F32(0.25)) & (grads[0] != 0)
    for r in range(3):
        assert np.flatnonzero(ties[r]).tolist() == list(range(62, 62 + first)) + list(range(290, 290 + last))
    # the same runs above a flat background: every element below the ties is equal as well
    pred, target = TO.tie_inputs(3, 300, [(62, 67), (290, 300)], seed=3, background=0.125)
    for kk, sel in ((3, [62, 63, 64]), (9, [62, 63, 64, 65, 66, 290, 291, 292, 293]), (17, list(range(62, 67)) + list(range(290, 300)) + [0, 1])):
        want = TO.expected(pred, target, kk, 3, 3)
        loss, grads, kth = _abi_topk(dev, [pred], target, kk, 3, 3)
        assert TO.check(want, grads[0], kth[0], loss[1]) == []
        for r in range(3):
            assert sorted(np.flatnonzero(grads[0][r]).tolist()) == sorted(sel)


def test_exact_row_gives_zero(dev):
    """pred == target, k = 3: loss exactly 0, kth = 0, every gradient +0.0 bit for bit -- the three selected exact hits
    too (the focal kernel itself writes -0.0 at an exact hit; this kernel writes no negative zero)"""
    (_, ), target = TO.random_inputs(2, 65, seed=9)
    for gamma in (3, 2, 0.5):
        loss, grads, kth = _abi_topk(dev, [target.copy()], target, 3, 2, gamma)
        assert loss.view(U32).tolist() == [0, 0] and kth.view(U32).ravel().tolist() == [0, 0]
        assert np.all(grads[0].view(U32) == 0), gamma


def test_all_equal_row_longer_than_16_bit_counts(dev):
    pred, target = TO.tie_inputs(1, 70001, [(0, 70001)], seed=4)
    k = 66000
    want = TO.expected(pred, target, k, 3, 1)
    loss, grads, kth = _abi_topk(dev, [pred], target, k, 1, 3)
    assert TO.check(want, grads[0], kth[0], loss[1]) == []
    assert np.array_equal(grads[0][0] != 0, np.arange(70001) < k)


# --------------------------------------------------------------------------------------------------------------- T3
@pytest.mark.parametrize("gamma", [3, 2, 0.5])
def test_selected_gradients_are_the_focal_kernels_bits(dev, gamma):
    from unet_nested4tiny_objects_keypoints_amd import ops
    preds, target = TO.random_inputs(4, 4097, seed=12, heads=2)
    sel = [TO.selection(p, target, 41)[0] for p in preds]
    td = torch.from_numpy(target).to(dev)
    pd = [torch.from_numpy(p).to(dev) for p in preds]
    for denom in (4, 4 * 41):
        _, grads, _ = _abi_topk(dev, preds[:1], target, 41, denom, gamma)
        focal = ops.focal_bce(pd[0], td, denom, gamma)[1].cpu().numpy()
        assert np.array_equal(grads[0].view(U32), np.where(sel[0], focal, F32(0.0)).view(U32))
        _, grads, _ = _abi_topk(dev, preds, target, 41, denom, gamma)
        focal = [g.cpu().numpy() for g in ops.focal_bce_heads(pd, td, denom, gamma)[1]]
        for h in range(2):
            assert np.array_equal(grads[h].view(U32), np.where(sel[h], focal[h], F32(0.0)).view(U32))


@pytest.mark.parametrize("size_average", [False, True])
@pytest.mark.parametrize("kw", [dict(k=65), dict(k=1000), dict(fraction=1.0)])
def test_all_pixels_is_the_focal_loss_bit_for_bit(dev, kw, size_average):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, TopKFocalLoss_BCE_2d
    (pred,), target = TO.random_inputs(6, 65, seed=13)
    t = torch.from_numpy(target).to(dev).view(2, 3, 5, 13)
    p1 = torch.from_numpy(pred).to(dev).view(2, 3, 5, 13).requires_grad_(True)
    p2 = p1.detach().clone().requires_grad_(True)
    crit = TopKFocalLoss_BCE_2d(gamma=3, size_average=size_average, **kw)
    a = crit(p1, t)
    b = FocalLoss_BCE_2d(gamma=3, size_average=size_average)(p2, t)
    a.backward()
    b.backward()
    assert _same_bits(a, b) and _same_bits(p1.grad, p2.grad)
    assert np.array_equal(crit.last_threshold.cpu().numpy().view(U32), np.abs(pred - target).min(1).view(U32))


# --------------------------------------------------------------------------------------------------------------- T4
def test_digits(dev):
    """target = 0 and pred = float32 from uint32, so the key is the pattern: row 0 differs in the low 7 bits only (a
    permutation), row 1 in the lowest mantissa bit only (two values, alternating), row 2 in the top byte only
    (0x34 .. 0x3E, six of each).  Every key has a non-zero gradient, so the non-zero gradients are the selection."""
    rng = np.random.default_rng(21)
    pixels = 66
    pat = np.zeros((3, pixels), U32)
    pat[0] = 0x3E800000 + rng.permutation(pixels)
    pat[1] = 0x3E800000 + (np.arange(pixels) % 2)
    pat[2] = ((0x34 + rng.permutation(pixels) % 11).astype(U32) << 24) | 0x2AAAAA
    pred, target = TO.bit_pattern_inputs(pat)
    for k in (1, 10, 15, 33, 40, 65):
        want = TO.expected(pred, target, k, 3, 3)
        loss, grads, kth = _abi_topk(dev, [pred], target, k, 3, 3)
        assert TO.check(want, grads[0], kth[0], loss[1]) == [], k
        assert np.array_equal(grads[0] != 0, want.selected), k
        assert np.array_equal(kth[0].view(U32), np.sort(pat, axis=1)[:, ::-1][:, k - 1]), k


@pytest.mark.parametrize("in_bin", [2047, 2048, 2049])
def test_threshold_bin_at_the_candidate_list_size(dev, in_bin):
    """the kernel lists the keys of the first digit's bin in LDS when there are at most 2048 of them and reads the row a
    third time otherwise: rows whose threshold bin (keys 0x3E8xxxxx) holds 2047, 2048 and 2049 elements, the other
    elements in bins below and above it; k reaches into that bin"""
    rng = np.random.default_rng(in_bin)
    pixels = 3001
    pat = np.zeros((2, pixels), U32)
    for r in range(2):
        keys = np.concatenate([0x3E800000 + rng.integers(0, 1 << 20, in_bin), 0x3F000000 + rng.integers(0, 1 << 22, 100),
                               0x3D000000 + rng.integers(0, 1 << 23, pixels - in_bin - 100)]).astype(U32)
        pat[r] = rng.permutation(keys)
    pat[1, 5:40] = 0x3E812345       # and a tie run at the threshold of row 1 for k = 120
    pat[1, np.flatnonzero((pat[1] > 0x3E812345) & (pat[1] < 0x3F000000))[18:]] = 0x3E800001
    pred, target = TO.bit_pattern_inputs(pat)
    for k in (120, 1000, 100 + in_bin, 101 + in_bin):
        want = TO.expected(pred, target, k, 3, 2)
        loss, grads, kth = _abi_topk(dev, [pred], target, k, 2, 3)
        assert TO.check(want, grads[0], kth[0], loss[1]) == [], k
        assert np.array_equal(grads[0] != 0, want.selected), k


# --------------------------------------------------------------------------------------------------------------- T5
def _loop(crit_kw, preds, target):
    """the trainer's loop body with single-head calls and float32 tensor arithmetic -> (avg, [grad], [kth])"""
    from unet_nested4tiny_objects_keypoints_amd import TopKFocalLoss_BCE_2d
    crit = TopKFocalLoss_BCE_2d(**crit_kw)
    leaves = [p.detach().clone().requires_grad_(True) for p in preds]
    avg, kth = 0, []
    for p in leaves:
        avg = avg + crit(p, target)
        kth.append(crit.last_threshold)
    avg = 1.0 * avg / len(leaves)
    avg.backward()
    return avg.detach(), [p.grad for p in leaves], torch.stack(kth)


@pytest.mark.parametrize("heads,shape,kw", [(1, (2, 3, 5, 13), dict(k=7)), (2, (2, 3, 5, 13), dict(k=7, size_average=True)),
                                            (5, (1, 3, 17, 241), dict(fraction=0.01)), (8, (2, 2, 16, 16), dict(fraction=0.5, gamma=2)),
                                            (8, (7, 100, 3, 11), dict(k=4))])
def test_heads_form_is_the_written_out_loop_bit_for_bit(dev, heads, shape, kw):
    """(the last case: 8 heads x 700 rows of P = 33 -- 5600 workgroups)"""
    from unet_nested4tiny_objects_keypoints_amd import TopKFocalLoss_BCE_2d, ops
    rows, pixels = shape[0] * shape[1], shape[2] * shape[3]
    preds_np, target_np = TO.random_inputs(rows, pixels, seed=heads, heads=heads)
    target = torch.from_numpy(target_np).to(dev).view(shape)
    preds = [torch.from_numpy(p).to(dev).view(shape) for p in preds_np]
    avg, grads, kth = _loop(kw, preds, target)
    crit = TopKFocalLoss_BCE_2d(**kw)
    k_eff = crit.k_for(pixels)
    loss, got, got_kth = ops.topk_focal_heads(preds, target, k_eff, crit._denom(rows, k_eff), float(crit.gamma))
    assert _same_bits(loss[0], avg) and _same_bits(got_kth, kth)
    for a, b in zip(got, grads):
        assert _same_bits(a, b)
    fused = crit.mean_over_heads(tuple(p.requires_grad_(True) for p in preds), target)
    if heads == 1:
        assert fused is None      # (the contract of FocalLoss_BCE_2d.mean_over_heads: the caller runs the loop)
    else:
        assert _same_bits(fused[0], avg) and fused[0].dim() == 0 and _same_bits(crit.last_threshold, kth)
        for a, b in zip(fused[1], grads):
            assert _same_bits(a, b)
        assert crit.mean_over_heads(tuple(p.detach().cpu() for p in preds), target.cpu()) is None
    # and the first head against the oracle
    want = TO.expected(preds_np[0], target_np, k_eff, crit.gamma, crit._denom(rows, k_eff), heads=heads)
    assert TO.check(want, got[0].cpu().numpy(), got_kth[0].cpu().numpy(), loss[1].item()) == []


def test_loss_in_the_finish_kernels_second_trip(dev):
    """1027 rows of 8 pixels, two heads, k = 3: the heads equal the target except in rows 1023, 1024 and 1026, so the
    loss sits in the last partial of the finish's first trip over the rows and in two of its second trip"""
    rows, pixels, k, hot = 1027, 8, 3, [1023, 1024, 1026]
    rand, target = TO.random_inputs(rows, pixels, seed=57, heads=2)
    preds = [target.copy() for _ in rand]
    for p, r in zip(preds, rand):
        p[hot] = r[hot]
    loss, grads, kth = _abi_topk(dev, preds, target, k, rows, 3)
    for h in range(2):
        want = TO.expected(preds[h], target, k, 3, rows, heads=2)
        assert TO.check(want, grads[h], kth[h], loss[1 + h]) == []          # (kth bit for bit)
        assert np.flatnonzero(kth[h]).tolist() == hot
        second = float(want.iv.l_want.reshape(rows, pixels)[1024:][want.selected[1024:]].sum()) / rows
        assert second > 0.1 * want.loss[0] > 0 and want.loss[2] - want.loss[1] < 1e-3 * second   # a lost trip shows
    avg = (F32(0) + loss[1]) + loss[2]
    assert loss[0].view(U32) == ((F32(1.0) * avg) * F32(0.5)).view(U32)


def test_one_long_row(dev):
    pixels = 2 ** 20 + 3
    (pred,), target = TO.random_inputs(1, pixels, seed=31)
    k = 10486      # fraction 0.01
    want = TO.expected(pred, target, k, 3, 1)
    loss, grads, kth = _abi_topk(dev, [pred], target, k, 1, 3)
    assert TO.check(want, grads[0], kth[0], loss[1]) == []


# --------------------------------------------------------------------------------------------------------------- T6
def test_nan_ranks_first(dev):
    (pred,), target = TO.random_inputs(4, 65, seed=41)
    clean = pred.copy()
    clean[2, 17] = target[2, 17]
    pred[2, 17] = np.nan
    want = TO.expected(clean, target, 1, 3, 4)
    loss, grads, kth = _abi_topk(dev, [pred], target, 1, 4, 3)
    assert np.isnan(kth[0, 2]) and np.isnan(loss[1]) and np.isnan(loss[0])
    others = np.arange(4) != 2
    assert TO.check(want, grads[0], kth[0], loss[1], rows=others) == []
    assert np.all(grads[0][2, np.arange(65) != 17].view(U32) == 0)


# --------------------------------------------------------------------------------------------------------------- T7
def test_criterion_backward_scales_the_kernel_gradient(dev):
    from unet_nested4tiny_objects_keypoints_amd import TopKFocalLoss_BCE_2d, ops
    (pred,), target = TO.random_inputs(6, 65, seed=51)
    t = torch.from_numpy(target).to(dev).view(2, 3, 5, 13)
    p = torch.from_numpy(pred).to(dev).view(2, 3, 5, 13).requires_grad_(True)
    crit = TopKFocalLoss_BCE_2d(fraction=0.1)
    loss = crit(p, t)
    (2.0 * loss).backward()
    _, grads, kth = ops.topk_focal_heads([p.detach()], t, 7, 6, 3.0)
    assert _same_bits(p.grad, grads[0] * 2.0) and _same_bits(crit.last_threshold, kth[0])
    assert crit.last_threshold.shape == (6,)
    want = TO.expected(pred, target, 7, 3, 6)
    assert TO.check(want, grads[0].cpu().numpy(), kth[0].cpu().numpy(), loss.item()) == []


def _small_net(dev):
    from tests.helpers import load_golden
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    _, ctor = load_golden("fs8_bilinear_32x32_b2")
    torch.manual_seed(61)
    m = UNet_Nested(**ctor).to(dev).train()
    m.drop_out.p = 0.0
    g = torch.Generator().manual_seed(62)
    return m, torch.randn(2, 1, 32, 32, generator=g).to(dev), torch.rand(2, 4, 32, 32, generator=g).to(dev)


def test_train_step_equals_the_written_out_loop(dev):
    from unet_nested4tiny_objects_keypoints_amd import TopKFocalLoss_BCE_2d, train_step
    model, x, target = _small_net(dev)
    twin = copy.deepcopy(model)
    crit = TopKFocalLoss_BCE_2d(fraction=0.05)
    opt, opt2 = torch.optim.SGD(model.parameters(), lr=0.05), torch.optim.SGD(twin.parameters(), lr=0.05)
    outs, loss = train_step(model, opt, crit, x, target)
    assert crit.last_threshold.shape == (len(outs), 8)
    opt2.zero_grad()
    outs2 = twin(x)
    assert isinstance(outs2, tuple) and len(outs2) >= 2
    avg = 0
    for o in outs2:
        avg = avg + crit(o, target)
    avg = 1.0 * avg / len(outs2)
    avg.backward()
    assert _same_bits(loss, avg.detach())
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        assert _same_bits(p.grad, q.grad), n
    # the same call twice gives identical bits
    a, b = copy.deepcopy(twin), copy.deepcopy(twin)
    results = []
    for m in (a, b):
        o = torch.optim.SGD(m.parameters(), lr=0.05)
        _, l = train_step(m, o, TopKFocalLoss_BCE_2d(fraction=0.05), x, target)
        results.append((l, [p.grad.clone() for p in m.parameters()]))
    assert _same_bits(results[0][0], results[1][0])
    for p, q in zip(results[0][1], results[1][1]):
        assert _same_bits(p, q)


def test_validate_step_returns_the_criterions_values(dev):
    from unet_nested4tiny_objects_keypoints_amd import Heatmap, TopKFocalLoss_BCE_2d, validate_step
    model, x, _ = _small_net(dev)
    model.eval()
    hm = Heatmap([[0], [1, 2, 3], [4], [5, 6]], 32, 32)
    labels = (torch.rand(2, 8, 2, generator=torch.Generator().manual_seed(63)) * 20 + 6).to(dev)
    crit = TopKFocalLoss_BCE_2d(fraction=0.05)
    res = validate_step(model, crit, hm, x, labels)
    with torch.no_grad():
        outs = model(x)
        target = hm.create_heatmap(labels)
        want = torch.stack([crit(o, target) for o in (outs if isinstance(outs, tuple) else (outs,))])
    assert _same_bits(res.heatmap_losses, want)
    for o, v in zip(outs if isinstance(outs, tuple) else (outs,), want):
        exp = TO.expected(o.cpu().numpy().reshape(8, -1), target.cpu().numpy().reshape(8, -1), crit.k_for(1024), 3, 8)
        assert lo.loss_ratio(v.item(), exp.loss) <= 1.0


def test_graphed_train_step_replays_the_eager_step(dev):
    from unet_nested4tiny_objects_keypoints_amd import GraphedTrainStep, TopKFocalLoss_BCE_2d, train_step
    a, x0, t0 = _small_net(dev)
    b = copy.deepcopy(a)
    crit_a, crit_b = TopKFocalLoss_BCE_2d(fraction=0.05), TopKFocalLoss_BCE_2d(fraction=0.05)
    oa = torch.optim.SGD(a.parameters(), lr=2e-3, momentum=0.9)
    ob = torch.optim.SGD(b.parameters(), lr=2e-3, momentum=0.9)
    g = torch.Generator().manual_seed(64)
    xs = [x0] + [torch.randn(2, 1, 32, 32, generator=g).to(dev) for _ in range(2)]
    ts = [t0] + [torch.rand(2, 4, 32, 32, generator=g).to(dev) for _ in range(2)]
    step = GraphedTrainStep(a, oa, crit_a, xs[0], ts[0], capture_optimizer=True)
    for x, t in zip(xs, ts):
        outs_g, loss_g = step(x, t)
        outs_e, loss_e = train_step(b, ob, crit_b, x, t)
        assert float(loss_g) == float(loss_e)
        assert _same_bits(crit_a.last_threshold, crit_b.last_threshold)
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert _same_bits(p, q) and _same_bits(p.grad, q.grad), k
