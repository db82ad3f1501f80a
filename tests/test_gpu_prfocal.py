"""Penalty-reduced focal loss on the GPU (csrc/pr_focal.hip, ops.pr_focal_heads, losses.PenaltyReducedFocalLoss) against
the float64 oracle (tests/prfocal_oracle.py): every gradient inside its a-priori interval, exactly +0.0 behind a closed
gate, n_pos exact, every loss inside its bound; tails, an unaligned view, a size at which the finish and the count pass
take further trips; the heads form against the written-out loop; the wiring into train_step and GraphedTrainStep."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import prfocal_oracle as PO

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ops(dev, preds, target, want_grad=True, **params):
    """ops.pr_focal_heads on numpy inputs -> (loss [1 + heads], [grad] or None, n_pos) as numpy / int"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    kw = dict(PO.DEFAULTS, **params)
    loss, grads, n_pos = ops.pr_focal_heads([torch.from_numpy(np.array(p, dtype=F32)).to(dev) for p in preds],
                                            torch.from_numpy(np.array(target, dtype=F32)).to(dev), kw["alpha"], kw["beta"],
                                            kw["eps"], kw["positive"], want_grad=want_grad)
    assert n_pos.dtype == torch.int64 and n_pos.dim() == 0 and n_pos.is_cuda
    return loss.cpu().numpy(), None if grads is None else [g.cpu().numpy() for g in grads], int(n_pos)


def _abi(dev, preds, target, fill=None, **params):
    """unetpp_pr_focal_heads through the C ABI, a NaN guard behind every grad and the workspace pre-filled with the byte
    `fill` -> as _ops"""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    from unet_nested4tiny_objects_keypoints_amd.ops import _ptr, _stream, check
    lib = _lib.lib()
    kw = dict(PO.DEFAULTS, **params)
    n = target.size
    td = torch.from_numpy(target).to(dev)
    pd = [torch.from_numpy(p).to(dev) for p in preds]
    nbytes = int(lib.unetpp_pr_focal_workspace_bytes(len(preds), n))
    assert nbytes > 0
    ws = torch.zeros((nbytes + 7) // 8 * 8, dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.fill_(fill)
    loss = torch.empty(1 + len(preds), dtype=torch.float32, device=dev)
    n_pos = torch.full((), -7, dtype=torch.int64, device=dev)
    bufs = [torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev) for _ in preds]
    hd = _lib.FocalHeads()
    hd.n_heads = len(preds)
    for i, p in enumerate(pd):
        hd.pred[i] = p.data_ptr()
        hd.grad[i] = bufs[i].data_ptr()
    check(lib.unetpp_pr_focal_heads(C.byref(hd), _ptr(td), n, kw["alpha"], kw["beta"], kw["eps"], kw["positive"], _ptr(ws),
                                    _ptr(n_pos), _ptr(loss), _stream()), "unetpp_pr_focal_heads")
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(torch.isnan(b[n:]).all()), "the guard behind grad was written"
    return loss.cpu().numpy(), [b[:n].cpu().numpy() for b in bufs], int(n_pos)


def _same(a, b):
    """two results of _ops / _abi, bit for bit"""
    if not np.array_equal(a[0].view(U32), b[0].view(U32)) or a[2] != b[2]:
        return False
    if (a[1] is None) != (b[1] is None):
        return False
    return a[1] is None or all(np.array_equal(x.view(U32), y.view(U32)) for x, y in zip(a[1], b[1]))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# --------------------------------------------------------------------------------------------------------------- P1
@pytest.mark.parametrize("positive", PO.POSITIVES)
@pytest.mark.parametrize("heads", [1, 3])
def test_elements_tails_and_parameters(dev, heads, positive):
    """every tail size x every (alpha, beta): the planted p (0, lo, just below lo, hi, just above hi, 1) against the
    planted t (positive, just below it, 0) at the front and inside the scalar tail"""
    failures, worst = [], 0.0
    for n in PO.TAIL_SIZES:
        preds, target = PO.inputs(n, heads=heads, seed=heads, positive=positive)
        for alpha, beta in PO.PARAMS:
            params = dict(alpha=alpha, beta=beta, eps=1e-4, positive=positive)
            got = _ops(dev, preds, target, **params)
            bad = PO.check_all(preds, target, got, **params)
            if heads == 1 and got[0][0].view(U32) != got[0][1].view(U32):
                bad.append("one head: loss[0] %r is not loss[1] %r" % (got[0][0], got[0][1]))
            exp = PO.expected(preds[0], target, heads=heads, **params)
            worst = max(worst, float(PO.grad_ratio(got[1][0], exp).max()), PO.loss_ratio(got[0][1], exp.loss))
            failures += ["n = %d, %r: %s" % (n, params, m) for m in bad]
    print("prfocal elements: heads", heads, "positive", positive, "worst err / room %.3g" % worst)
    assert not failures, failures[:10]


@pytest.mark.parametrize("n", PO.TAIL_SIZES)
def test_nothing_is_written_behind_the_gradient(dev, n):
    preds, target = PO.inputs(n, heads=2, seed=7)
    got = _abi(dev, preds, target)
    assert PO.check_all(preds, target, got, **PO.DEFAULTS) == []
    assert _same(got, _ops(dev, preds, target))


def test_view_that_starts_four_bytes_into_its_storage(dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n = 2051
    preds, target = PO.inputs(n, heads=2, seed=8)
    store = [torch.zeros(n + 1, device=dev) for _ in range(3)]
    views = [s[1:] for s in store]
    for v, a in zip(views, preds + [target]):
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    loss, grads, n_pos = ops.pr_focal_heads(views[:2], views[2], 2.0, 4.0, 1e-4, 1.0)
    got = (loss.cpu().numpy(), [g.cpu().numpy() for g in grads], int(n_pos))
    assert PO.check_all(preds, target, got, **PO.DEFAULTS) == []
    assert _same(got, _ops(dev, preds, target))


# --------------------------------------------------------------------------------------------------------------- P2
@pytest.mark.parametrize("region", sorted(PO.BIG_REGIONS))
def test_large_n_one_region_at_a_time(dev, region):
    """BIG_N elements: 1026 workgroups, so the finish kernel's strided loop takes a second trip, and 513 count chunks on
    256 count workgroups, so those take a second and a third; the loss and the positives come from ONE region"""
    pred, target = PO.region_inputs(region)
    got = _ops(dev, [pred], target)
    exp = PO.expected(pred, target)
    assert exp.n_pos == (1 if region == "last3" else 75)
    assert PO.check(exp, got[1][0], got[2], got[0][1]) == []
    lo, hi = PO.BIG_REGIONS[region]
    inside = float(exp.l_want[lo:hi].sum())
    assert inside > 0.999 * float(exp.l_want.sum())             # a lost block would lose the loss


def test_two_heads_loss_in_the_finish_kernels_second_trip(dev):
    """two heads of 1024 * 2048 + 5 elements -- 1025 workgroups, the last over the 5-element tail: p = 0 against t = 0
    everywhere (as PO.region_inputs) except 300 elements of block 1023 and the tail, a quarter of them positives, so each
    head's loss sits in the last partial of the finish's first trip and in the one partial of its second"""
    n = 1024 * PO.BLOCK + 5
    rng = np.random.default_rng(7400)
    idx = np.concatenate([1023 * PO.BLOCK + np.sort(rng.choice(PO.BLOCK, 300, replace=False)), np.arange(n - 5, n)])
    t = np.zeros(n, F32)
    t[idx] = rng.random(idx.size).astype(F32)
    t[idx[::4]] = 1.0
    preds = [np.zeros(n, F32) for _ in range(2)]
    for p in preds:
        p[idx] = (rng.random(idx.size).astype(F32) * F32(0.998) + F32(0.001)).astype(F32)
    got = _ops(dev, preds, t)
    assert got[2] == int((t >= 1.0).sum()) == 77                 # n_pos exactly; the tail holds two of them
    assert PO.check_all(preds, t, got, **PO.DEFAULTS) == []
    for p in preds:
        exp = PO.expected(p, t, heads=2)
        tail, block = float(exp.l_want[n - 5:].sum()), float(exp.l_want[1023 * PO.BLOCK:1024 * PO.BLOCK].sum())
        assert tail + block > 0.999 * float(exp.l_want.sum())
        assert min(tail, block) / exp.denom > 100 * (exp.loss[2] - exp.loss[1])   # a lost partial leaves the bound


def test_large_n_positives_in_every_count_trip(dev):
    """positives spread over all 513 count chunks, two heads"""
    rng = np.random.default_rng(77)
    t = rng.random(PO.BIG_N).astype(F32)
    t[rng.random(PO.BIG_N) < 0.001] = 1.0
    preds = [(rng.random(PO.BIG_N).astype(F32) * F32(0.998) + F32(0.001)).astype(F32) for _ in range(2)]
    got = _ops(dev, preds, t)
    assert got[2] == int((t >= 1.0).sum()) > 1500
    assert PO.check_all(preds, t, got, **PO.DEFAULTS) == []


# --------------------------------------------------------------------------------------------------------------- P3
@pytest.mark.parametrize("n", [5, 2049])
def test_degenerate_targets(dev, n):
    preds, target = PO.inputs(n, heads=2, seed=9, positives=0.0, plant=False)
    got = _ops(dev, preds, target)
    assert got[2] == 0 and np.isfinite(got[0]).all()              # no positive: the sum is divided by 1
    assert PO.check_all(preds, target, got, **PO.DEFAULTS) == []
    ones = np.ones(n, F32)
    got = _ops(dev, preds, ones)
    assert got[2] == n
    assert PO.check_all(preds, ones, got, **PO.DEFAULTS) == []
    low = dict(PO.DEFAULTS, positive=0.85)
    t = np.full(n, F32(0.85))
    got = _ops(dev, preds, t, **low)
    assert got[2] == n and PO.check_all(preds, t, got, **low) == []
    t = np.full(n, PO.just_below(0.85))
    got = _ops(dev, preds, t, **low)
    assert got[2] == 0 and PO.check_all(preds, t, got, **low) == []


def test_nan_in_pred_is_not_hidden(dev):
    preds, target = PO.inputs(2049, heads=2, seed=10)
    preds[1][1000] = np.nan
    got = _ops(dev, preds, target)
    assert np.isnan(got[0][0]) and np.isnan(got[0][2]) and np.isfinite(got[0][1])
    assert PO.check_all(preds, target, got, **PO.DEFAULTS) == []
    g = got[1][1][1000]
    assert np.isnan(g) or g == 0


@pytest.mark.parametrize("n", [7, 4099])
def test_want_grad_false_repeat_and_workspace(dev, n):
    """want_grad = False gives the same loss bits; two runs give the same bits in every output; a workspace pre-filled
    with NaN bytes changes nothing"""
    preds, target = PO.inputs(n, heads=3, seed=11)
    first = _ops(dev, preds, target)
    again = _ops(dev, preds, target)
    assert _same(first, again)
    without = _ops(dev, preds, target, want_grad=False)
    assert without[1] is None and np.array_equal(without[0].view(U32), first[0].view(U32)) and without[2] == first[2]
    assert _same(first, _abi(dev, preds, target, fill=0xFF))
    assert _same(first, _abi(dev, preds, target, fill=0x00))


# --------------------------------------------------------------------------------------------------------------- P4
def _loop(crit, preds, target):
    """the trainer's loop body with single-head calls and float32 tensor arithmetic -> (avg, [grad])"""
    leaves = [p.detach().clone().requires_grad_(True) for p in preds]
    avg = 0
    for p in leaves:
        avg = avg + crit(p, target)
    avg = 1.0 * avg / len(leaves)
    avg.backward()
    return avg.detach(), [p.grad for p in leaves]


@pytest.mark.parametrize("heads", [2, 3, 8])
@pytest.mark.parametrize("kw", [dict(), dict(alpha=2.5, beta=3.5, positive=0.85)])
def test_heads_form_is_the_written_out_loop_bit_for_bit(dev, heads, kw):
    from unet_nested4tiny_objects_keypoints_amd import PenaltyReducedFocalLoss
    shape = (2, 4, 64, 64)
    n = int(np.prod(shape))
    preds_np, target_np = PO.inputs(n, heads=heads, seed=20 + heads, positive=kw.get("positive", 1.0), positives=0.01)
    target = torch.from_numpy(target_np).to(dev).view(shape)
    preds = [torch.from_numpy(p).to(dev).view(shape) for p in preds_np]
    crit = PenaltyReducedFocalLoss(**kw)
    avg, grads = _loop(crit, preds, target)
    count = crit.last_num_positives.clone()
    fused = crit.mean_over_heads(tuple(p.requires_grad_(True) for p in preds), target)
    assert fused is not None and fused[0].dim() == 0 and not fused[0].requires_grad
    assert _same_bits(fused[0], avg)
    for a, b in zip(fused[1], grads):
        assert _same_bits(a, b)
    assert torch.equal(crit.last_num_positives, count) and int(count) == int((target_np >= F32(kw.get("positive", 1.0))).sum())
    params = dict(PO.DEFAULTS, **kw)
    exp = PO.expected(preds_np[0], target_np, heads=heads, **params)
    assert PO.check(exp, fused[1][0].cpu().numpy(), int(count), None) == []
    assert crit.mean_over_heads(tuple(p.detach().cpu() for p in preds), target.cpu()) is None
    assert crit.mean_over_heads((preds[0],), target) is None


def test_nine_heads_return_none(dev):
    from unet_nested4tiny_objects_keypoints_amd import PenaltyReducedFocalLoss
    t = torch.rand(2, 4, 64, 64, device=dev)
    assert PenaltyReducedFocalLoss().mean_over_heads(tuple(torch.rand_like(t) for _ in range(9)), t) is None


def test_criterion_backward_scales_the_kernel_gradient(dev):
    from unet_nested4tiny_objects_keypoints_amd import PenaltyReducedFocalLoss, ops
    (pred,), target = PO.inputs(2 * 3 * 5 * 13, seed=30)
    t = torch.from_numpy(target).to(dev).view(2, 3, 5, 13)
    p = torch.from_numpy(pred).to(dev).view(2, 3, 5, 13).requires_grad_(True)
    crit = PenaltyReducedFocalLoss()
    loss = crit(p, t)
    (2.0 * loss).backward()
    losses, grads, n_pos = ops.pr_focal_heads([p.detach()], t, 2.0, 4.0, 1e-4, 1.0)
    assert _same_bits(p.grad, grads[0] * 2.0) and _same_bits(loss.detach(), losses[0])
    assert torch.equal(crit.last_num_positives, n_pos)
    with torch.no_grad():
        assert _same_bits(crit(p, t), losses[0])


# --------------------------------------------------------------------------------------------------------------- P5
def _net(dev):
    from tests.helpers import load_golden
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    _, ctor = load_golden("c1_fs4_64x64_b4_seed0")
    torch.manual_seed(71)
    m = UNet_Nested(**ctor).to(dev).train()
    m.drop_out.p = 0.0
    return m, ctor


def _batch(ctor, g, dev, batch=2):
    x = torch.randn(batch, ctor["in_channels"], 64, 64, generator=g)
    t = torch.rand(batch, ctor["n_classes"], 64, 64, generator=g)
    t[torch.rand(t.shape, generator=g) < 0.002] = 1.0
    return x.to(dev), t.to(dev)


def test_train_step_equals_the_written_out_loop(dev, monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import PenaltyReducedFocalLoss, step, train_step
    model, ctor = _net(dev)
    twin = copy.deepcopy(model)
    x, target = _batch(ctor, torch.Generator().manual_seed(72), dev)
    crit, crit2 = PenaltyReducedFocalLoss(), PenaltyReducedFocalLoss()
    opt, opt2 = torch.optim.SGD(model.parameters(), lr=0.05), torch.optim.SGD(twin.parameters(), lr=0.05)
    assert step._FUSED_HEAD_LOSS
    outs, loss = train_step(model, opt, crit, x, target)
    assert isinstance(outs, tuple) and len(outs) >= 2
    monkeypatch.setattr(step, "_FUSED_HEAD_LOSS", False)
    outs2, loss2 = train_step(twin, opt2, crit2, x, target)
    assert _same_bits(loss.detach(), loss2.detach())
    assert int(crit.last_num_positives) == int(crit2.last_num_positives) == int((target >= 1.0).sum()) > 0
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        assert _same_bits(p.grad, q.grad) and _same_bits(p, q), n


def test_train_step_at_a_pruned_head_runs(dev):
    from unet_nested4tiny_objects_keypoints_amd import PenaltyReducedFocalLoss, train_step
    model, ctor = _net(dev)
    x, target = _batch(ctor, torch.Generator().manual_seed(73), dev)
    crit = PenaltyReducedFocalLoss()
    _, loss = train_step(model, torch.optim.SGD(model.parameters(), lr=0.05), crit, x, target, head=1)
    assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
    assert int(crit.last_num_positives) == int((target >= 1.0).sum())


def test_graphed_train_step_replays_the_eager_step(dev):
    from unet_nested4tiny_objects_keypoints_amd import GraphedTrainStep, PenaltyReducedFocalLoss, train_step
    a, ctor = _net(dev)
    b = copy.deepcopy(a)
    crit_a, crit_b = PenaltyReducedFocalLoss(), PenaltyReducedFocalLoss()
    oa = torch.optim.SGD(a.parameters(), lr=2e-3, momentum=0.9)
    ob = torch.optim.SGD(b.parameters(), lr=2e-3, momentum=0.9)
    g = torch.Generator().manual_seed(74)
    batches = [_batch(ctor, g, dev) for _ in range(3)]
    step = GraphedTrainStep(a, oa, crit_a, batches[0][0], batches[0][1], capture_optimizer=True)
    counts = set()
    for x, t in batches:
        _, loss_g = step(x, t)
        _, loss_e = train_step(b, ob, crit_b, x, t)
        assert float(loss_g) == float(loss_e)
        assert int(crit_a.last_num_positives) == int(crit_b.last_num_positives) == int((t >= 1.0).sum())
        counts.add(int(crit_a.last_num_positives))
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert _same_bits(p, q) and _same_bits(p.grad, q.grad), k
    assert len(counts) > 1          # the targets change, and the count with them
