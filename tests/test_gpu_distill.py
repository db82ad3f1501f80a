"""Self-distillation across the heads on the GPU (csrc/distill.hip, ops.distill_heads, losses.HeadDistillLoss) against the
float64 oracle (tests/distill_oracle.py) and, bit for bit, against the composition of the existing entry points
(ops.focal_bce_heads, ops.focal_bce and float32 tensor arithmetic); tails, guard words, an unaligned view, a size at which
the finish takes a second trip, non-finite values, set_weight, and the wiring into train_step and GraphedTrainStep."""
import copy
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import distill_oracle as DO
from tests import loss_oracle as LO

pytestmark = pytest.mark.gpu
F32, F64, U32 = np.float32, np.float64, np.uint32
GUARD = 64
# (teacher, gate, ignore, distill_ignored): distill_ignored only matters with ignore on
CONFIGS = [dict(teacher=t, gate=g, ignore=i, distill_ignored=k)
           for t, g, (i, k) in itertools.product(DO.TEACHERS, DO.GATES, ((False, True), (True, True), (True, False)))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(heads, n, seed, ignore):
    preds, t = DO.inputs(heads, n, seed, ignore)
    for a in preds + [t]:
        a.flags.writeable = False     # (cached: shared among the tests)
    return tuple(preds), t


def _weight(dev, w):
    return torch.full((1,), float(w), dtype=torch.float32, device=dev)


def _run(dev, preds, target, rows, gamma, w, want_grad=True, **cfg):
    """ops.distill_heads on numpy inputs -> (loss [1 + heads], [grad] or None, S [heads], D [heads]) as numpy"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    loss, grads, sup, dis = ops.distill_heads([torch.from_numpy(np.array(p, dtype=F32)).to(dev) for p in preds],
                                              torch.from_numpy(np.array(target, dtype=F32)).to(dev), rows, gamma,
                                              _weight(dev, w), want_grad=want_grad, **cfg)
    assert loss.shape == (1 + len(preds),) and sup.shape == dis.shape == (len(preds),)
    return (loss.cpu().numpy(), None if grads is None else [g.cpu().numpy() for g in grads], sup.cpu().numpy(),
            dis.cpu().numpy())


def _same(a, b):
    """two results of _run / _abi, bit for bit"""
    if not all(np.array_equal(a[k].view(U32), b[k].view(U32)) for k in (0, 2, 3)):
        return False
    if (a[1] is None) != (b[1] is None):
        return False
    return a[1] is None or all(np.array_equal(x.view(U32), y.view(U32)) for x, y in zip(a[1], b[1]))


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1: elements, tails
@pytest.mark.parametrize("gamma", [3.0, 2.0, 0.5])
@pytest.mark.parametrize("heads", [1, 2, 3, 8])
def test_elements_and_tails(dev, heads, gamma):
    """every tail size (the vector path, the scalar tail, three blocks) x both teachers x both gates x ignore off / on x
    distill_ignored both ways: every gradient inside its interval, the sign rules and the exact zeros, S_j, D_j, L_j and
    the mean inside their bounds"""
    failures, worst, rows, w = [], 0.0, 3, 0.75
    for n in LO.TAIL_SIZES:
        for cfg in CONFIGS:
            preds, t = _inputs(heads, n, heads, cfg["ignore"])
            got = _run(dev, preds, t, rows, gamma, w, **cfg)
            bad, r = DO.check(DO.expected(preds, t, rows, gamma, w, **cfg), *got)
            if heads == 1 and got[0][0].view(U32) != got[0][1].view(U32):
                bad.append("one head: loss[0] %r is not loss[1] %r" % (got[0][0], got[0][1]))
            worst = max(worst, r)
            failures += ["n = %d, %r: %s" % (n, cfg, m) for m in bad]
    print("distill elements: heads", heads, "gamma", gamma, "worst err / room %.3g" % worst)
    assert not failures, failures[:10]


# ----------------------------------------------------------------------- 2: the composition of existing entry points
def _composition(preds, target, rows, gamma, w, teacher, gate, ignore, distill_ignored):
    """ops.focal_bce_heads for the supervised part, ops.focal_bce(p_j, p_T) for the distillation part, float32 tensor
    arithmetic for the rest: one multiply by the mask (where there is one), one by float32(1 / heads), one by w, one add
    -> (focal_bce_heads' losses, [D_j or None where a mask changes the order of the sum], [grad], all_admitted)"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    heads = len(preds)
    inv_heads, w32 = float(F32(1.0) / F32(heads)), float(F32(w))
    plain, G = ops.focal_bce_heads(preds, target, rows, gamma, ignore=ignore)
    D, grads = [], []
    for j in range(heads - 1):
        p, q = preds[j], preds[DO.teacher_of(j, heads, teacher)]
        ld, gd = ops.focal_bce(p, q, rows, gamma)
        admit = torch.ones_like(target, dtype=torch.bool)
        if gate == "teacher_better":
            admit = (q - target).abs() < (p - target).abs()
        if ignore:
            admit = torch.where(target < 0, torch.full_like(admit, bool(distill_ignored)), admit)
        everything = bool(admit.all())
        if not everything:
            gd = gd * admit.to(torch.float32)
        D.append(ld if everything else None)
        grads.append(G[j] + w32 * (gd * inv_heads))
    grads.append(G[heads - 1])
    D.append(torch.zeros((), dtype=torch.float32, device=target.device))
    return plain, D, grads


@pytest.mark.parametrize("heads", [2, 3, 8])
@pytest.mark.parametrize("gamma", [3.0, 0.5])
def test_bit_for_bit_against_the_composition(dev, heads, gamma):
    """S_j and the supervised gradients are focal_bce_heads'; without gate and ignore rule D_j is focal_bce(p_j, p_T)'s loss
    and the stored gradient G_s + w32 * (focal_bce_grad * float32(1 / heads)); with them the same with the D gradient
    masked, and D_j inside the oracle's bound (the masked sum has another order)"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, rows, w = 4099, 4, 0.75
    for cfg in CONFIGS:
        preds_np, t_np = _inputs(heads, n, 20 + heads, cfg["ignore"])
        preds = [torch.from_numpy(np.array(p)).to(dev) for p in preds_np]
        t = torch.from_numpy(np.array(t_np)).to(dev)
        loss, grads, sup, dis = ops.distill_heads(preds, t, rows, gamma, _weight(dev, w), **cfg)
        plain, D, want = _composition(preds, t, rows, gamma, w, **cfg)
        assert _same_bits(sup, plain[1:]), cfg
        for j in range(heads):
            assert _same_bits(grads[j], want[j]), (cfg, j)
            if D[j] is not None:
                assert _same_bits(dis[j], D[j]), (cfg, j)
        if cfg["gate"] == "none" and not cfg["ignore"]:
            assert all(d is not None for d in D)
        L = sup + float(F32(w)) * dis                       # one product, one sum
        assert _same_bits(loss[1:], L), cfg
        avg = torch.zeros((), dtype=torch.float32, device=dev)
        for j in range(heads):
            avg = avg + L[j]
        assert _same_bits(loss[0], (1.0 * avg) * float(F32(1.0) / F32(heads))), cfg
        got = (loss.cpu().numpy(), [g.cpu().numpy() for g in grads], sup.cpu().numpy(), dis.cpu().numpy())
        bad, _ = DO.check(DO.expected(preds_np, t_np, rows, gamma, w, **cfg), *got)
        assert bad == [], (cfg, bad[:3])


# ---------------------------------------------------------------------------------------------------- 3: weight = 0
@pytest.mark.parametrize("heads", [2, 3])
def test_weight_zero_is_focal_bce_heads_bit_for_bit(dev, heads):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, rows = 4099, 4
    for cfg in CONFIGS:
        preds_np, t_np = _inputs(heads, n, 30 + heads, cfg["ignore"])
        preds = [torch.from_numpy(np.array(p)).to(dev) for p in preds_np]
        t = torch.from_numpy(np.array(t_np)).to(dev)
        loss, grads, sup, dis = ops.distill_heads(preds, t, rows, 3.0, _weight(dev, 0.0), **cfg)
        plain, G = ops.focal_bce_heads(preds, t, rows, 3.0, ignore=cfg["ignore"])
        assert _same_bits(loss, plain) and _same_bits(sup, plain[1:]), cfg
        for a, b in zip(grads, G):
            assert _same_bits(a, b), cfg
        assert bool((dis[:-1] > 0).all()) and float(dis[-1]) == 0.0      # D_j is reported, but it does not enter


# --------------------------------------------------------------------------------------------------- 4: set_weight
def test_set_weight_changes_the_result_without_a_new_tensor(dev):
    from unet_nested4tiny_objects_keypoints_amd import HeadDistillLoss
    shape, rows = (2, 2, 32, 33), 4
    n = int(np.prod(shape))
    preds_np, t_np = _inputs(3, n, 40, False)
    preds = tuple(torch.from_numpy(np.array(p)).to(dev).view(shape).requires_grad_(True) for p in preds_np)
    t = torch.from_numpy(np.array(t_np)).to(dev).view(shape)
    crit = HeadDistillLoss(weight=0.5, gate="teacher_better")
    results = []
    for w in (0.5, 0.125):
        crit.set_weight(w)
        avg, grads = crit.mean_over_heads(preds, t)
        assert avg.dim() == 0 and not avg.requires_grad
        held = crit.weight_tensor(dev)
        results.append((avg.clone(), [g.clone() for g in grads], held.data_ptr()))
        sup, dis = crit.last_supervised.cpu().numpy(), crit.last_distill.cpu().numpy()
        loss = np.concatenate([[avg.cpu().numpy()], sup + F32(w) * dis]).astype(F32)
        exp = DO.expected(preds_np, t_np, rows, 3.0, w, gate="teacher_better")
        bad, _ = DO.check(exp, loss, [g.cpu().numpy() for g in grads], sup, dis)
        assert bad == [], (w, bad[:3])
    assert results[0][2] == results[1][2] and len(crit._weight_dev) == 1 and float(held) == 0.125
    assert float(results[1][0]) < float(results[0][0])
    assert not _same_bits(results[0][1][0], results[1][1][0]) and _same_bits(results[0][1][2], results[1][1][2])
    leaves = [p.detach().clone().requires_grad_(True) for p in preds]
    (2.0 * crit.heads_loss(tuple(leaves), t)).backward()
    for leaf, g in zip(leaves, results[1][1]):
        assert _same_bits(leaf.grad, g * 2.0)
    with torch.no_grad():      # one map has no teacher: forward is FocalLoss_BCE_2d with the same bits
        from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
        assert _same_bits(crit(preds[0], t), FocalLoss_BCE_2d(gamma=3)(preds[0], t))


# ------------------------------------------------------------------------------- 5: guards, alignment, want_grad
def _abi(dev, preds, target, rows, gamma, w, with_grad=True, fill=None, teacher="last", gate="none", ignore=False,
         distill_ignored=True):
    """unetpp_distill_heads through the C ABI, a NaN guard behind every grad and the workspace pre-filled with the byte
    `fill` -> as _run; with_grad=False passes no gradient pointer and checks that the planted buffers stay untouched"""
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import _ptr, _stream, check
    lib = _lib.lib()
    heads, n = len(preds), target.size
    td = torch.from_numpy(np.array(target)).to(dev)
    pd = [torch.from_numpy(np.array(p)).to(dev) for p in preds]
    blocks = int(lib.unetpp_focal_bce_blocks(n))
    ws = torch.zeros(2 * heads * blocks + GUARD, dtype=torch.float32, device=dev)
    if fill is not None:
        ws.view(torch.uint8).fill_(fill)
    ws[2 * heads * blocks:] = float("nan")
    loss = torch.full((1 + 3 * heads + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    bufs = [torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=dev) for _ in preds]
    hd = _lib.FocalHeads()
    hd.n_heads = heads
    for i, p in enumerate(pd):
        hd.pred[i] = p.data_ptr()
        hd.grad[i] = bufs[i].data_ptr() if with_grad else None
    wd = _weight(dev, w)
    check(lib.unetpp_distill_heads(C.byref(hd), _ptr(td), n, rows, gamma, _ptr(wd), ops.DISTILL_TEACHERS[teacher],
                                   ops.DISTILL_GATES[gate], int(ignore), int(distill_ignored), _ptr(ws), _ptr(loss),
                                   _stream()), "unetpp_distill_heads")
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(torch.isnan(b[n if with_grad else 0:]).all()), "the guard behind grad was written"
    assert bool(torch.isnan(ws[2 * heads * blocks:]).all()) and bool(torch.isnan(loss[1 + 3 * heads:]).all())
    out = loss[:1 + 3 * heads].cpu().numpy()
    return (out[:1 + heads], [b[:n].cpu().numpy() for b in bufs] if with_grad else None, out[1 + heads:1 + 2 * heads],
            out[1 + 2 * heads:])


@pytest.mark.parametrize("n", LO.TAIL_SIZES)
def test_nothing_is_written_behind_a_gradient(dev, n):
    cfg = dict(teacher="next", gate="teacher_better", ignore=True, distill_ignored=True)
    preds, t = _inputs(3, n, 50, True)
    got = _abi(dev, preds, t, 3, 3.0, 0.5, **cfg)
    assert DO.check(DO.expected(preds, t, 3, 3.0, 0.5, **cfg), *got)[0] == []
    assert _same(got, _run(dev, preds, t, 3, 3.0, 0.5, **cfg))


@pytest.mark.parametrize("n", [7, 4099])
def test_want_grad_false_repeat_and_workspace(dev, n):
    """without gradient pointers no gradient is written and the losses keep their bits; two runs give the same bits; a
    workspace pre-filled with NaN bytes changes nothing"""
    cfg = dict(teacher="last", gate="teacher_better", ignore=True, distill_ignored=False)
    preds, t = _inputs(3, n, 51, True)
    first = _run(dev, preds, t, 3, 2.0, 0.5, **cfg)
    assert _same(first, _run(dev, preds, t, 3, 2.0, 0.5, **cfg))
    without = _run(dev, preds, t, 3, 2.0, 0.5, want_grad=False, **cfg)
    assert without[1] is None and all(np.array_equal(without[k].view(U32), first[k].view(U32)) for k in (0, 2, 3))
    planted = _abi(dev, preds, t, 3, 2.0, 0.5, with_grad=False, fill=0xFF, **cfg)
    assert planted[1] is None and all(np.array_equal(planted[k].view(U32), first[k].view(U32)) for k in (0, 2, 3))
    assert _same(first, _abi(dev, preds, t, 3, 2.0, 0.5, fill=0xFF, **cfg))
    assert _same(first, _abi(dev, preds, t, 3, 2.0, 0.5, fill=0x00, **cfg))


def test_view_that_starts_four_bytes_into_its_storage(dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n = 2051
    preds, t = _inputs(2, n, 52, False)
    store = [torch.zeros(n + 1, device=dev) for _ in range(3)]
    views = [s[1:] for s in store]
    for v, a in zip(views, list(preds) + [t]):
        v.copy_(torch.from_numpy(np.array(a)))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    loss, grads, sup, dis = ops.distill_heads(views[:2], views[2], 3, 3.0, _weight(dev, 0.5))
    got = (loss.cpu().numpy(), [g.cpu().numpy() for g in grads], sup.cpu().numpy(), dis.cpu().numpy())
    assert DO.check(DO.expected(preds, t, 3, 3.0, 0.5), *got)[0] == []
    assert _same(got, _run(dev, preds, t, 3, 3.0, 0.5))


# ------------------------------------------------------------------------------------------------------ 6: large n
def test_large_n_distillation_terms_in_block_1024(dev):
    """BIG_N elements: 1026 workgroups, so the finish takes its second strided trip for S and for D.  Two heads; the
    teacher equals the target, the student differs from both inside block 1024 only, so D_0 (and S_0) come from there."""
    student, target = LO.region_inputs("block1024")
    preds = (student, target)
    got = _run(dev, preds, target, 7, 3.0, 0.5)
    exp = DO.expected(preds, target, 7, 3.0, 0.5)
    bad, _ = DO.check(exp, *got)
    assert bad == [], bad[:3]
    assert exp.heads[0].D[0] > 0 and got[3][0] > 0 and got[2][1] == 0 and got[3][1] == 0
    lo, hi = LO.BIG_REGIONS["block1024"]
    assert np.flatnonzero(got[1][0]).min() >= lo and np.flatnonzero(got[1][0]).max() < hi


# --------------------------------------------------------------------------------------------------- 7: non-finite
def test_nan_is_not_hidden(dev):
    """A NaN in a student's map reaches its L_j and the mean.  A NaN in the teacher's map reaches D_j of its students with
    gate="none"; it does not reach the teacher's own S_J when it lies under an ignored target.  With gate="teacher_better"
    a NaN on either side of the comparison keeps the element out of D_j: the student's gradient there is its supervised
    gradient, and D_j stays finite."""
    n, i = 2049, 1000
    preds, t = _inputs(2, n, 60, False)
    student = [np.array(p) for p in preds]
    student[0][i] = np.nan
    loss, grads, sup, dis = _run(dev, student, t, 3, 3.0, 0.5)
    assert np.isnan(loss[0]) and np.isnan(loss[1]) and np.isnan(sup[0]) and np.isfinite(loss[2]) and np.isfinite(sup[1])
    assert np.isfinite(np.delete(grads[0], i)).all() and np.isfinite(grads[1]).all()

    teacher = [np.array(p) for p in preds]
    teacher[1][i] = np.nan
    ti = np.array(t)
    ti[i] = -1.0
    loss, grads, sup, dis = _run(dev, teacher, ti, 3, 3.0, 0.5, ignore=True, distill_ignored=True)
    assert np.isnan(dis[0]) and np.isnan(loss[1]) and np.isnan(loss[0])
    assert np.isfinite(sup).all() and np.isfinite(loss[2]) and dis[1].view(U32) == 0
    assert grads[1][i].view(U32) == 0 and np.isfinite(grads[1]).all()
    loss, grads, sup, dis = _run(dev, teacher, ti, 3, 3.0, 0.5, ignore=True, distill_ignored=False)
    assert np.isfinite(loss).all() and np.isfinite(dis).all() and grads[0][i].view(U32) == 0

    loss, grads, sup, dis = _run(dev, teacher, t, 3, 3.0, 0.5, gate="teacher_better")
    from unet_nested4tiny_objects_keypoints_amd import ops
    plain, G = ops.focal_bce_heads([torch.from_numpy(p).to(dev) for p in teacher], torch.from_numpy(np.array(t)).to(dev), 3, 3.0)
    assert np.isfinite(dis).all() and np.isfinite(sup[0]) and np.isnan(sup[1]) and np.isfinite(loss[1])
    assert grads[0][i].view(U32) == G[0].cpu().numpy()[i].view(U32) and np.isfinite(grads[0]).all()
    loss, grads, sup, dis = _run(dev, student, t, 3, 3.0, 0.5, gate="teacher_better")
    assert np.isfinite(dis).all() and np.isnan(sup[0])       # (the student's side of the comparison)


# --------------------------------------------------------------------------------------------- 8: through the step
def _net(dev):
    from tests.helpers import load_golden, sub
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    z, ctor = load_golden("fs8_bilinear_32x32_b2")
    m = UNet_Nested(**ctor)
    m.load_state_dict(sub(z, "state0"), strict=True)
    return m.to(dev).train(), ctor


def _batch(ctor, g, dev):
    x = torch.randn(2, ctor["in_channels"], 32, 32, generator=g)
    t = torch.rand(2, ctor["n_classes"], 32, 32, generator=g)
    t[torch.rand(t.shape, generator=g) < 0.1] = -1.0
    return x.to(dev), t.to(dev)


_STEP_CFG = dict(teacher="last", gate="teacher_better", ignore_negative=True, distill_ignored=True)


@pytest.mark.parametrize("head", [None, 2])
def test_train_step_is_the_forward_and_the_composition_gradients(dev, head):
    from unet_nested4tiny_objects_keypoints_amd import HeadDistillLoss, train_step
    model, ctor = _net(dev)
    twin, again = copy.deepcopy(model), copy.deepcopy(model)
    x, target = _batch(ctor, torch.Generator().manual_seed(81), dev)
    crit = HeadDistillLoss(weight=0.75, **_STEP_CFG)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    torch.manual_seed(82)
    outs, loss = train_step(model, opt, crit, x, target, head=head)
    assert isinstance(outs, tuple) and len(outs) == (head or len(outs)) >= 2
    assert crit.last_distill.shape == (len(outs),) and float(crit.last_distill[0]) > 0
    torch.manual_seed(82)
    outs2 = twin(x) if head is None else twin.forward_pruned(x, head)
    for a, b in zip(outs, outs2):
        assert _same_bits(a, b)
    rows = target.shape[0] * target.shape[1]
    _, _, grads = _composition([o.detach() for o in outs2], target, rows, 3.0, 0.75, "last", "teacher_better", True, True)
    torch.autograd.backward(list(outs2), grads)
    seen = 0
    for (k, p), q in zip(model.named_parameters(), twin.parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            assert _same_bits(p.grad, q.grad), k
            seen += 1
    assert seen > 10
    torch.manual_seed(82)              # a repeat of the same call gives the same bits
    _, loss2 = train_step(again, torch.optim.SGD(again.parameters(), lr=0.0), HeadDistillLoss(weight=0.75, **_STEP_CFG), x,
                          target, head=head)
    assert _same_bits(loss.detach(), loss2.detach())
    for (k, p), q in zip(model.named_parameters(), again.parameters()):
        if p.grad is not None:
            assert _same_bits(p.grad, q.grad), k


def test_graphed_train_step_follows_set_weight_without_a_new_capture(dev):
    from unet_nested4tiny_objects_keypoints_amd import GraphedTrainStep, HeadDistillLoss, train_step
    a, ctor = _net(dev)
    a.drop_out.p = 0.0
    b = copy.deepcopy(a)
    crit_a, crit_b = HeadDistillLoss(weight=0.75, **_STEP_CFG), HeadDistillLoss(weight=0.75, **_STEP_CFG)
    oa = torch.optim.SGD(a.parameters(), lr=2e-3, momentum=0.9)
    ob = torch.optim.SGD(b.parameters(), lr=2e-3, momentum=0.9)
    g = torch.Generator().manual_seed(83)
    batches = [_batch(ctor, g, dev) for _ in range(4)]
    step = GraphedTrainStep(a, oa, crit_a, batches[0][0], batches[0][1], capture_optimizer=True)
    graph = step._graph
    for k, (x, t) in enumerate(batches):
        if k == 2:                      # the schedule moves: a fill_ of the device word, the same captured graph
            crit_a.set_weight(0.0)
            crit_b = HeadDistillLoss(weight=0.0, **_STEP_CFG)
        _, loss_g = step(x, t)
        _, loss_e = train_step(b, ob, crit_b, x, t)
        assert _same_bits(loss_g.detach(), loss_e.detach()), k
        assert _same_bits(crit_a.last_supervised, crit_b.last_supervised) and _same_bits(crit_a.last_distill, crit_b.last_distill)
        for (name, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert _same_bits(p, q) and _same_bits(p.grad, q.grad), (k, name)
    assert step._graph is graph and len(crit_a._weight_dev) == 1
    assert float(crit_a.last_distill[0]) > 0        # still reported at weight 0
