"""Distillation from an external map on the GPU (csrc/distill.hip: unetpp_teacher_heads, ops.teacher_heads,
losses.TeacherDistillLoss, SceneCrops(teacher=...)) against the float64 oracle (tests/teacher_oracle.py) and, bit for bit,
against the existing entry points: ops.focal_bce_heads for the supervised part, ops.focal_bce for the distillation part,
float32 tensor arithmetic for the masks and the two combinations, and ops.distill_heads with the deepest head's own map
as the teacher; tails, guard words, an unaligned view, a size at which the finish takes a second trip, non-finite
values, set_teacher, the wiring into train_step and GraphedTrainStep, the windows SceneCrops cuts out of a teacher's
scene maps, and a frame without labels that trains on the teacher alone."""
import copy
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import loss_oracle as LO
from tests import teacher_oracle as TO

pytestmark = pytest.mark.gpu
F32, F64, U32 = np.float32, np.float64, np.uint32
GUARD = 64
# (gate, ignore, distill_ignored): distill_ignored only matters with ignore on
CONFIGS = [dict(gate=g, ignore=i, distill_ignored=k)
           for g, (i, k) in itertools.product(TO.GATES, ((False, True), (True, True), (True, False)))]
BIG_TAILS = tuple(n for n in LO.TAIL_SIZES if n >= TO.MIN_SHARE_N)
# (heads, n, seed) of every case below that relies on the mask classes: tests/test_teacher_host.py asserts on the CPU that
# each class holds 5 % of the elements per head for every one of CONFIGS; the tests here assert it again before they run
MASKED_CASES = ([(h, n, h) for h in (1, 2, 3, 8) for n in BIG_TAILS] + [(h, 4099, 20 + h) for h in (2, 3, 8)]
                + [(3, n, 50) for n in BIG_TAILS] + [(3, 4099, 51)])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(heads, n, seed, ignore, void=True):
    preds, t, q = TO.inputs(heads, n, seed, ignore, void)
    for a in preds + [t, q]:
        a.flags.writeable = False     # (cached: shared among the tests)
    return tuple(preds), t, q


@functools.lru_cache(maxsize=None)
def _expected(heads, n, seed, rows, gamma, w, gate, ignore, distill_ignored, void=True):
    """the oracle's expectation, computed once and shared; the mask classes asserted where the case relies on them"""
    preds, t, q = _inputs(heads, n, seed, ignore, void)
    exp = TO.expected(preds, t, q, rows, gamma, w, gate, ignore, distill_ignored)
    if void and n >= TO.MIN_SHARE_N:
        assert (heads, n, seed) in MASKED_CASES
        thin = TO.thin_classes(exp, gate, ignore, distill_ignored, void)
        assert thin == [], "a mask class below 5 %%: %r" % (thin,)
    return exp


def _weight(dev, w):
    return torch.full((1,), float(w), dtype=torch.float32, device=dev)


def _to(dev, a):
    return torch.from_numpy(np.array(a, dtype=F32)).to(dev)


def _np(loss, grads, sup, dis):
    return (loss.cpu().numpy(), None if grads is None else [g.cpu().numpy() for g in grads], sup.cpu().numpy(),
            dis.cpu().numpy())


def _run(dev, preds, target, teacher, rows, gamma, w, want_grad=True, **cfg):
    """ops.teacher_heads on numpy inputs -> (loss [1 + heads], [grad] or None, S [heads], D [heads]) as numpy"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    loss, grads, sup, dis = ops.teacher_heads([_to(dev, p) for p in preds], _to(dev, target), _to(dev, teacher), rows, gamma,
                                              _weight(dev, w), want_grad=want_grad, **cfg)
    assert loss.shape == (1 + len(preds),) and sup.shape == dis.shape == (len(preds),)
    return _np(loss, grads, sup, dis)


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
    """every tail size (the vector path, the scalar tail, three blocks) x both gates x ignore off / on x distill_ignored
    both ways, a third of the teacher void: every gradient inside its interval, the sign rules and the exact zeros,
    S_h, D_h, L_h and the mean inside their bounds, L_h and the mean the float32 combinations of what is reported"""
    failures, worst, rows, w = [], 0.0, 3, 0.75
    for n in LO.TAIL_SIZES:
        for cfg in CONFIGS:
            preds, t, q = _inputs(heads, n, heads, cfg["ignore"])
            got = _run(dev, preds, t, q, rows, gamma, w, **cfg)
            bad, r = TO.check(_expected(heads, n, heads, rows, gamma, w, **cfg), *got)
            if heads == 1 and got[0][0].view(U32) != got[0][1].view(U32):
                bad.append("one head: loss[0] %r is not loss[1] %r" % (got[0][0], got[0][1]))
            worst = max(worst, r)
            failures += ["n = %d, %r: %s" % (n, cfg, m) for m in bad]
    print("teacher elements: heads", heads, "gamma", gamma, "worst err / room %.3g" % worst)
    assert not failures, failures[:10]


# ----------------------------------------------------------------------- 2: the composition of existing entry points
def _composition(preds, target, teacher, rows, gamma, w, gate="none", ignore=False, distill_ignored=True):
    """The kernel's rule restated in float32 over the existing entry points: ops.focal_bce_heads for the supervised part,
    the three masks as float32 tensor comparisons, ops.focal_bce(p_h, q') for the distillation part with q' = q on an
    admitted element and p_h itself elsewhere (an exact hit: its term and its gradient are zeros, and a zero added to a
    sum leaves its bits), one product by float32(1 / heads), one by w, one sum, and the supervised gradient's own bits on
    an element that is kept out  -> (focal_bce_heads' losses, [D_h], [grad], [admitted])"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    heads = len(preds)
    inv_heads, w32 = float(F32(1.0) / F32(heads)), float(F32(w))
    plain, G = ops.focal_bce_heads(preds, target, rows, gamma, ignore=ignore)
    void = teacher < 0
    D, grads, admits = [], [], []
    for j, p in enumerate(preds):
        admit = torch.ones_like(target, dtype=torch.bool)
        if gate == "teacher_better":
            admit = (teacher - target).abs() < (p - target).abs()
        if ignore:
            admit = torch.where(target < 0, torch.full_like(admit, bool(distill_ignored)), admit)
        admit = admit & ~void
        ld, gd = ops.focal_bce(p, torch.where(admit, teacher, p), rows, gamma)
        D.append(ld)
        grads.append(torch.where(admit, G[j] + w32 * (gd * inv_heads), G[j]))
        admits.append(admit)
    return plain, D, grads, admits


@pytest.mark.parametrize("heads", [2, 3, 8])
@pytest.mark.parametrize("gamma", [3.0, 0.5])
@pytest.mark.parametrize("void", [False, True])
def test_bit_for_bit_against_the_composition(dev, heads, gamma, void):
    """S_h and the supervised gradients are focal_bce_heads' (or _ignore's); without gate, ignore and a void element D_h
    is focal_bce(p_h, q)'s loss and the stored gradient G_s + w32 * (focal_bce_grad * float32(1 / heads)); with masks the
    float32 restatement over the same entry points (_composition) has the same bits, its masks being the oracle's"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, rows, w, seed = 4099, 4, 0.75, 20 + heads
    for cfg in CONFIGS:
        preds_np, t_np, q_np = _inputs(heads, n, seed, cfg["ignore"], void)
        exp = _expected(heads, n, seed, rows, gamma, w, void=void, **cfg)
        preds, t, q = [_to(dev, p) for p in preds_np], _to(dev, t_np), _to(dev, q_np)
        loss, grads, sup, dis = ops.teacher_heads(preds, t, q, rows, gamma, _weight(dev, w), **cfg)
        plain, D, want, admits = _composition(preds, t, q, rows, gamma, w, **cfg)
        assert _same_bits(sup, plain[1:]), cfg
        plain_everything = cfg["gate"] == "none" and not cfg["ignore"] and not void
        for j in range(heads):
            assert np.array_equal(admits[j].cpu().numpy(), exp.heads[j].admitted), (cfg, j)
            if plain_everything:
                assert bool(admits[j].all())
                ld, gd = ops.focal_bce(preds[j], q, rows, gamma)
                assert _same_bits(dis[j], ld), (cfg, j)
                G = ops.focal_bce_heads(preds, t, rows, gamma)[1]
                assert _same_bits(grads[j], G[j] + float(F32(w)) * (gd * float(F32(1.0) / F32(heads)))), (cfg, j)
            assert _same_bits(grads[j], want[j]), (cfg, j)
            assert _same_bits(dis[j], D[j]), (cfg, j)
        L = sup + float(F32(w)) * dis                       # one product, one sum
        assert _same_bits(loss[1:], L), cfg
        avg = torch.zeros((), dtype=torch.float32, device=dev)
        for j in range(heads):
            avg = avg + L[j]
        assert _same_bits(loss[0], (1.0 * avg) * float(F32(1.0) / F32(heads))), cfg
        bad, _ = TO.check(exp, *_np(loss, grads, sup, dis))
        assert bad == [], (cfg, bad[:3])


# ------------------------------------------------------------------------------------------------ 3: degenerate cases
@pytest.mark.parametrize("heads", [2, 3])
def test_weight_zero_is_focal_bce_heads_bit_for_bit(dev, heads):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, rows = 4099, 4
    for cfg in CONFIGS:
        preds_np, t_np, q_np = _inputs(heads, n, 30 + heads, cfg["ignore"], False)
        preds, t, q = [_to(dev, p) for p in preds_np], _to(dev, t_np), _to(dev, q_np)
        loss, grads, sup, dis = ops.teacher_heads(preds, t, q, rows, 3.0, _weight(dev, 0.0), **cfg)
        plain, G = ops.focal_bce_heads(preds, t, rows, 3.0, ignore=cfg["ignore"])
        assert _same_bits(loss, plain) and _same_bits(sup, plain[1:]), cfg
        for a, b in zip(grads, G):
            assert _same_bits(a, b), cfg
        assert bool((dis > 0).all())                        # D_h is reported, the deepest head's too, but it does not enter


@pytest.mark.parametrize("heads", [1, 3])
def test_a_teacher_that_is_negative_everywhere_is_focal_bce_heads_for_any_weight(dev, heads):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, rows = 4099, 4
    for cfg in CONFIGS:
        preds_np, t_np, _ = _inputs(heads, n, 35 + heads, cfg["ignore"], False)
        preds, t = [_to(dev, p) for p in preds_np], _to(dev, t_np)
        q = -torch.rand(n, device=dev) - 1e-3
        q[::2] = -1.0
        plain, G = ops.focal_bce_heads(preds, t, rows, 3.0, ignore=cfg["ignore"])
        for w in (0.0, 0.75, 1e6):
            loss, grads, sup, dis = ops.teacher_heads(preds, t, q, rows, 3.0, _weight(dev, w), **cfg)
            assert _same_bits(loss, plain) and _same_bits(sup, plain[1:]), (cfg, w)
            assert bool((_bits(dis) == 0).all()), (cfg, w)             # +0.0
            for a, b in zip(grads, G):
                assert _same_bits(a, b), (cfg, w)


# -------------------------------------------------------------------------------------- 4: against the existing kernel
@pytest.mark.parametrize("heads", [2, 3, 8])
@pytest.mark.parametrize("gamma", [3.0, 0.5])
def test_the_deepest_heads_own_map_as_teacher_is_distill_heads_last(dev, heads, gamma):
    """heads 0 .. J-2: L_h, S_h, D_h and the gradients are unetpp_distill_heads(teacher = last)'s bits.  The deepest head
    is left out on purpose: against itself its distillation gradient is a zero whose sum with the supervised gradient
    may differ from that gradient in the sign of a zero."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, rows, w = 4099, 4, 0.75
    for cfg in CONFIGS:
        preds_np, t_np, _ = _inputs(heads, n, 40 + heads, cfg["ignore"], False)
        preds, t = [_to(dev, p) for p in preds_np], _to(dev, t_np)
        got = ops.teacher_heads(preds, t, preds[-1].clone(), rows, gamma, _weight(dev, w), **cfg)
        ref = ops.distill_heads(preds, t, rows, gamma, _weight(dev, w), teacher="last", **cfg)
        s = slice(0, heads - 1)
        assert _same_bits(got[0][1:][s], ref[0][1:][s]), cfg
        assert _same_bits(got[2][s], ref[2][s]) and _same_bits(got[3][s], ref[3][s]), cfg
        assert _same_bits(got[2], ref[2]), cfg                            # (S of the deepest head as well)
        for j in range(heads - 1):
            assert _same_bits(got[1][j], ref[1][j]), (cfg, j)
        assert float(ref[3][s].min()) > 0


# ------------------------------------------------------------------------------- 5: guards, alignment, want_grad
def _abi(dev, preds, target, teacher, rows, gamma, w, with_grad=True, fill=None, gate="none", ignore=False,
         distill_ignored=True):
    """unetpp_teacher_heads through the C ABI, a NaN guard behind every grad and the workspace of exactly 2 * heads *
    blocks floats, guarded and pre-filled with the byte `fill` -> as _run; with_grad=False passes no gradient pointer and
    checks that the planted buffers stay untouched"""
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import _ptr, _stream, check
    lib = _lib.lib()
    heads, n = len(preds), target.size
    td, qd = _to(dev, target), _to(dev, teacher)
    pd = [_to(dev, p) for p in preds]
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
    check(lib.unetpp_teacher_heads(C.byref(hd), _ptr(td), _ptr(qd), n, rows, gamma, _ptr(wd), ops.DISTILL_GATES[gate],
                                   int(ignore), int(distill_ignored), _ptr(ws), _ptr(loss), _stream()),
          "unetpp_teacher_heads")
    torch.cuda.synchronize()
    for b in bufs:
        assert bool(torch.isnan(b[n if with_grad else 0:]).all()), "the guard behind grad was written"
    assert bool(torch.isnan(ws[2 * heads * blocks:]).all()) and bool(torch.isnan(loss[1 + 3 * heads:]).all())
    if fill == 0xFF:      # every float of the workspace was written: none keeps the planted NaN pattern
        assert not bool(torch.isnan(ws[:2 * heads * blocks]).any())
    out = loss[:1 + 3 * heads].cpu().numpy()
    return (out[:1 + heads], [b[:n].cpu().numpy() for b in bufs] if with_grad else None, out[1 + heads:1 + 2 * heads],
            out[1 + 2 * heads:])


@pytest.mark.parametrize("n", LO.TAIL_SIZES)
def test_nothing_is_written_behind_a_gradient(dev, n):
    cfg = dict(gate="teacher_better", ignore=True, distill_ignored=True)
    preds, t, q = _inputs(3, n, 50, True)
    got = _abi(dev, preds, t, q, 3, 3.0, 0.5, **cfg)
    assert TO.check(_expected(3, n, 50, 3, 3.0, 0.5, **cfg), *got)[0] == []
    assert _same(got, _run(dev, preds, t, q, 3, 3.0, 0.5, **cfg))


@pytest.mark.parametrize("n", [7, 4099])
def test_want_grad_false_repeat_and_workspace(dev, n):
    """without gradient pointers no gradient is written and the losses keep their bits; two runs give the same bits; the
    workspace is exactly 2 * heads * blocks floats, all of them written, and what it held before changes nothing"""
    cfg = dict(gate="teacher_better", ignore=True, distill_ignored=False)
    preds, t, q = _inputs(3, n, 51, True)
    first = _run(dev, preds, t, q, 3, 2.0, 0.5, **cfg)
    assert TO.check(_expected(3, n, 51, 3, 2.0, 0.5, **cfg), *first)[0] == []
    assert _same(first, _run(dev, preds, t, q, 3, 2.0, 0.5, **cfg))
    without = _run(dev, preds, t, q, 3, 2.0, 0.5, want_grad=False, **cfg)
    assert without[1] is None and all(np.array_equal(without[k].view(U32), first[k].view(U32)) for k in (0, 2, 3))
    planted = _abi(dev, preds, t, q, 3, 2.0, 0.5, with_grad=False, fill=0xFF, **cfg)
    assert planted[1] is None and all(np.array_equal(planted[k].view(U32), first[k].view(U32)) for k in (0, 2, 3))
    assert _same(first, _abi(dev, preds, t, q, 3, 2.0, 0.5, fill=0xFF, **cfg))
    assert _same(first, _abi(dev, preds, t, q, 3, 2.0, 0.5, fill=0x00, **cfg))


def test_view_that_starts_four_bytes_into_its_storage(dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    n = 2051
    preds, t, q = _inputs(2, n, 52, False)
    store = [torch.zeros(n + 1, device=dev) for _ in range(4)]
    views = [s[1:] for s in store]
    for v, a in zip(views, list(preds) + [t, q]):
        v.copy_(torch.from_numpy(np.array(a)))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    got = _np(*ops.teacher_heads(views[:2], views[2], views[3], 3, 3.0, _weight(dev, 0.5)))
    assert _same(got, _run(dev, preds, t, q, 3, 3.0, 0.5))
    assert TO.check(TO.expected(preds, t, q, 3, 3.0, 0.5), *got)[0] == []


# ------------------------------------------------------------------------------------------------------ 6: large n
def test_large_n_teacher_terms_in_block_1024(dev):
    """BIG_N elements: 1026 workgroups, so the finish takes its second strided trip for S and for D.  The teacher is void
    everywhere but inside block 1024, where it equals the target; head 0 differs from the target there only, head 1 is
    the target: D_0 (and S_0) come from block 1024, D_1 and S_1 are zero."""
    student, target = LO.region_inputs("block1024")
    lo, hi = LO.BIG_REGIONS["block1024"]
    teacher = np.full(LO.BIG_N, -1.0, dtype=F32)
    teacher[lo:hi] = target[lo:hi]
    preds = (student, target)
    got = _run(dev, preds, target, teacher, 7, 3.0, 0.5)
    exp = TO.expected(preds, target, teacher, 7, 3.0, 0.5)
    assert int(exp.heads[0].admitted.sum()) == hi - lo and not exp.heads[0].admitted[:lo].any()
    bad, _ = TO.check(exp, *got)
    assert bad == [], bad[:3]
    assert exp.heads[0].D[0] > 0 and got[3][0] > 0 and got[2][1] == 0 and got[3][1] == 0
    assert got[3][0].view(U32) == got[2][0].view(U32)                   # the same terms in the same places
    assert np.flatnonzero(got[1][0]).min() >= lo and np.flatnonzero(got[1][0]).max() < hi


# --------------------------------------------------------------------------------------------------- 7: non-finite
def test_nan_is_not_hidden(dev):
    """A NaN teacher element is not negative: without the gate it is admitted and reaches D_h of every head and the mean,
    and leaves every S_h intact; with gate="teacher_better" the comparison is false, the element is kept out, the stored
    gradient there is the supervised one and everything is finite.  A NaN in a student's map reaches its L_h and the
    mean, and on the student's side of the gate keeps the element out of D_h."""
    from unet_nested4tiny_objects_keypoints_amd import ops
    n, i = 2049, 1000
    preds, t, q = _inputs(2, n, 60, False, False)
    bad_q = np.array(q)
    bad_q[i] = np.nan
    loss, grads, sup, dis = _run(dev, preds, t, bad_q, 3, 3.0, 0.5)
    assert np.isnan(dis).all() and np.isnan(loss).all() and np.isfinite(sup).all()
    clean = _run(dev, preds, t, q, 3, 3.0, 0.5)
    assert np.array_equal(sup.view(U32), clean[2].view(U32))
    for g in grads:
        assert np.isnan(g[i]) and np.isfinite(np.delete(g, i)).all()

    loss, grads, sup, dis = _run(dev, preds, t, bad_q, 3, 3.0, 0.5, gate="teacher_better")
    plain, G = ops.focal_bce_heads([_to(dev, p) for p in preds], _to(dev, t), 3, 3.0)
    assert np.isfinite(loss).all() and np.isfinite(dis).all() and np.isfinite(sup).all()
    for g, gs in zip(grads, G):
        assert np.isfinite(g).all() and g[i].view(U32) == gs.cpu().numpy()[i].view(U32)

    student = [np.array(p) for p in preds]
    student[0][i] = np.nan
    loss, grads, sup, dis = _run(dev, student, t, q, 3, 3.0, 0.5)
    assert np.isnan(loss[0]) and np.isnan(loss[1]) and np.isnan(sup[0]) and np.isfinite(loss[2]) and np.isfinite(sup[1])
    assert np.isfinite(dis[1]) and np.isfinite(np.delete(grads[0], i)).all() and np.isfinite(grads[1]).all()
    loss, grads, sup, dis = _run(dev, student, t, q, 3, 3.0, 0.5, gate="teacher_better")
    assert np.isfinite(dis).all() and np.isnan(sup[0])       # (the student's side of the comparison)


# --------------------------------------------------------------------------------------------------- 8: set_teacher
def test_set_teacher_keeps_its_buffer_and_the_result_follows_its_contents(dev):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, TeacherDistillLoss, ops
    shape, rows = (2, 2, 32, 33), 4
    n = int(np.prod(shape))
    preds_np, t_np, q_np = _inputs(3, n, 70, False)
    _, _, other_np = _inputs(3, n, 71, False)
    preds = tuple(_to(dev, p).view(shape).requires_grad_(True) for p in preds_np)
    t, qa, qb = _to(dev, t_np).view(shape), _to(dev, q_np).view(shape), _to(dev, other_np).view(shape)
    crit = TeacherDistillLoss(weight=0.5, gate="teacher_better")
    with pytest.raises(RuntimeError, match="no teacher"):
        crit.mean_over_heads(preds, t)
    held = crit.set_teacher(qa)
    ptr = held.data_ptr()
    assert ptr != qa.data_ptr()
    results = []
    for q in (qa, qb):
        assert crit.set_teacher(q) is held and held.data_ptr() == ptr and len(crit._teacher) == 1
        avg, grads = crit.mean_over_heads(preds, t)
        assert avg.dim() == 0 and not avg.requires_grad
        want = ops.teacher_heads([p.detach() for p in preds], t, q, rows, 3.0, crit.weight_tensor(dev), gate="teacher_better")
        assert _same_bits(avg, want[0][0]) and _same_bits(crit.last_supervised, want[2]) and _same_bits(crit.last_distill, want[3])
        for a, b in zip(grads, want[1]):
            assert _same_bits(a, b)
        results.append((avg.clone(), [g.clone() for g in grads]))
    assert not _same_bits(results[0][0], results[1][0]) and not _same_bits(results[0][1][2], results[1][1][2])
    exp = TO.expected(preds_np, t_np, other_np, rows, 3.0, 0.5, gate="teacher_better")
    sup, dis = crit.last_supervised.cpu().numpy(), crit.last_distill.cpu().numpy()
    loss = np.concatenate([[results[1][0].cpu().numpy()], sup + F32(0.5) * dis]).astype(F32)
    assert TO.check(exp, loss, [g.cpu().numpy() for g in results[1][1]], sup, dis)[0] == []
    crit.set_weight(0.125)
    assert crit.weight_tensor(dev).data_ptr() == crit.weight_tensor("cuda").data_ptr() and len(crit._weight_dev) == 1
    assert float(crit.mean_over_heads(preds, t)[0]) < float(results[1][0])
    leaves = [p.detach().clone().requires_grad_(True) for p in preds]
    avg, grads = crit.mean_over_heads(preds, t)
    (2.0 * crit.heads_loss(tuple(leaves), t)).backward()
    for leaf, g in zip(leaves, grads):
        assert _same_bits(leaf.grad, g * 2.0)
    with torch.no_grad():      # one map: forward is FocalLoss_BCE_2d with the same bits
        assert _same_bits(crit(preds[0], t), FocalLoss_BCE_2d(gamma=3)(preds[0], t))
    assert crit.set_teacher(torch.rand(1, 2, 32, 33, device=dev)) is not held and len(crit._teacher) == 2


# --------------------------------------------------------------------------------------------- 9, 10: through the step
_STEP_CFG = dict(gate="teacher_better", ignore_negative=True, distill_ignored=True)


def _teacher_map(target, g):
    """a teacher for a batch: random in [0, 1], a third of it void"""
    q = torch.rand(target.shape, generator=g)
    q[torch.rand(target.shape, generator=g) < 1.0 / 3.0] = -1.0
    return q.to(target.device)


@pytest.mark.parametrize("head", [None, 2])
def test_train_step_is_the_forward_and_the_composition_gradients(dev, head):
    from tests.test_gpu_distill import _batch, _net
    from unet_nested4tiny_objects_keypoints_amd import TeacherDistillLoss, train_step
    model, ctor = _net(dev)
    twin, again = copy.deepcopy(model), copy.deepcopy(model)
    g = torch.Generator().manual_seed(81)
    x, target = _batch(ctor, g, dev)
    teacher = _teacher_map(target, g)
    crit = TeacherDistillLoss(weight=0.75, **_STEP_CFG)
    crit.set_teacher(teacher)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    torch.manual_seed(82)
    outs, loss = train_step(model, opt, crit, x, target, head=head)
    assert isinstance(outs, tuple) and len(outs) == (head or len(outs)) >= 2
    assert crit.last_distill.shape == (len(outs),) and float(crit.last_distill.min()) > 0
    torch.manual_seed(82)
    outs2 = twin(x) if head is None else twin.forward_pruned(x, head)
    for a, b in zip(outs, outs2):
        assert _same_bits(a, b)
    rows = target.shape[0] * target.shape[1]
    plain, D, grads, admits = _composition([o.detach() for o in outs2], target, teacher, rows, 3.0, 0.75, "teacher_better",
                                           True, True)
    for a in admits:
        assert 0.05 < float(a.float().mean()) < 0.95         # (both sides of the masks are there)
    assert _same_bits(crit.last_supervised, plain[1:]) and _same_bits(crit.last_distill, torch.stack(D))
    L = plain[1:] + float(F32(0.75)) * torch.stack(D)
    avg = torch.zeros((), dtype=torch.float32, device=dev)
    for j in range(len(outs)):
        avg = avg + L[j]
    assert _same_bits(loss.detach(), (1.0 * avg) * float(F32(1.0) / F32(len(outs))))
    torch.autograd.backward(list(outs2), grads)
    seen = 0
    for (k, p), q in zip(model.named_parameters(), twin.parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            assert _same_bits(p.grad, q.grad), k
            seen += 1
    assert seen > 10
    torch.manual_seed(82)              # a repeat of the same call gives the same bits
    crit2 = TeacherDistillLoss(weight=0.75, **_STEP_CFG)
    crit2.set_teacher(teacher)
    _, loss2 = train_step(again, torch.optim.SGD(again.parameters(), lr=0.0), crit2, x, target, head=head)
    assert _same_bits(loss.detach(), loss2.detach())
    for (k, p), q in zip(model.named_parameters(), again.parameters()):
        if p.grad is not None:
            assert _same_bits(p.grad, q.grad), k


def test_graphed_train_step_follows_set_teacher_and_set_weight_without_a_new_capture(dev):
    from tests.test_gpu_distill import _batch, _net
    from unet_nested4tiny_objects_keypoints_amd import GraphedTrainStep, TeacherDistillLoss, train_step
    a, ctor = _net(dev)
    a.drop_out.p = 0.0
    b = copy.deepcopy(a)
    crit_a, crit_b = TeacherDistillLoss(weight=0.75, **_STEP_CFG), TeacherDistillLoss(weight=0.75, **_STEP_CFG)
    oa = torch.optim.SGD(a.parameters(), lr=2e-3, momentum=0.9)
    ob = torch.optim.SGD(b.parameters(), lr=2e-3, momentum=0.9)
    g = torch.Generator().manual_seed(83)
    batches = [_batch(ctor, g, dev) for _ in range(4)]
    teachers = [_teacher_map(t, g) for _, t in batches]
    held = crit_a.set_teacher(teachers[0])
    ptr = held.data_ptr()
    step = GraphedTrainStep(a, oa, crit_a, batches[0][0], batches[0][1], capture_optimizer=True, check_topology=True)
    assert step.topology["chain"] is True, step.topology
    graph = step._graph
    seen = []
    for k, ((x, t), q) in enumerate(zip(batches, teachers)):
        if k == 2:                      # the schedule moves: a fill_ of the device word, the same captured graph
            crit_a.set_weight(0.0)
            crit_b = TeacherDistillLoss(weight=0.0, **_STEP_CFG)
        assert crit_a.set_teacher(q) is held            # the teacher of this step: a copy_ into the captured buffer
        crit_b.set_teacher(q)
        _, loss_g = step(x, t)
        _, loss_e = train_step(b, ob, crit_b, x, t)
        assert _same_bits(loss_g.detach(), loss_e.detach()), k
        assert _same_bits(crit_a.last_supervised, crit_b.last_supervised) and _same_bits(crit_a.last_distill, crit_b.last_distill)
        for (name, p), (_, q2) in zip(a.named_parameters(), b.named_parameters()):
            assert _same_bits(p, q2) and _same_bits(p.grad, q2.grad), (k, name)
        seen.append(crit_a.last_distill.clone())
    assert step._graph is graph and held.data_ptr() == ptr and len(crit_a._teacher) == 1 and len(crit_a._weight_dev) == 1
    assert float(crit_a.last_distill.min()) > 0        # still reported at weight 0
    assert not _same_bits(seen[0], seen[1])


# -------------------------------------------------------------------------------------------- 11: SceneCrops(teacher=)
def _scene(H, W, classes=2, S=2, per=7, seed=9):
    """S frames of H x W (float32, one channel) with `per` labels each, some at the corners, and a teacher's maps of
    the same size with every element in (0, 1)"""
    rng = np.random.default_rng(seed)
    frames = rng.random((S, 1, H, W)).astype(F32)
    labels = np.zeros((S, per, 2), dtype=F32)
    cls = np.zeros((S, per), dtype=np.int32)
    for s in range(S):
        flat = rng.choice(H * W, per, replace=False)
        labels[s, :, 0], labels[s, :, 1] = flat % W, flat // W
        labels[s, 0] = (0, 0) if s == 0 else (W - 1, H - 1)
        cls[s] = rng.integers(0, classes, per)
    teacher = (rng.random((S, classes, H, W)) * 0.98 + 0.01).astype(F32)
    return frames, labels, cls, teacher


def _source_pixels(rows, size):
    """the source pixel (xs, ys) of every output pixel by the row's inverse map: int64 [N, Ho, Wo] each"""
    m = rows[:, :6].astype(F64)
    assert np.array_equal(m, np.round(m))
    yo, xo = np.meshgrid(np.arange(size[0]), np.arange(size[1]), indexing="ij")
    xs = m[:, 0, None, None] * xo + m[:, 1, None, None] * yo + m[:, 2, None, None]
    ys = m[:, 3, None, None] * xo + m[:, 4, None, None] * yo + m[:, 5, None, None]
    return xs.astype(np.int64), ys.astype(np.int64)


@pytest.mark.parametrize("H,W,augment", [(80, 96, None), (24, 96, None), (24, 96, dict(contrast=(0.5, 1.5), brightness=0.2))],
                         ids=["inside", "overhang", "overhang-photometric"])
def test_scene_crops_cut_the_teacher_with_the_batch(dev, H, W, augment):
    """Two frames, n_classes = 2, crop 32 x 32, n = 8, jitter (40, 40).  The draw keeps a window inside a frame that is
    at least as large as the window, whatever the jitter (unetpp_crops_draw clamps the origin), and centres it over a
    frame that is smaller: no batch holds both kinds.  So frames of 96 x 80 give the windows that lie inside and frames
    of 96 x 24 the ones that overhang (four rows above and four below), each asserted from crops.last; the photometric
    case draws a gain and a bias per window, which must not touch the teacher.  last_teacher is the loader oracle's warp
    of the teacher store bit for bit, every element -1 or the teacher element at the source pixel the row's inverse map
    names, and inputs, target, points and inside are those of a twin object without a teacher."""
    from tests import loader_oracle as LDO
    from unet_nested4tiny_objects_keypoints_amd import Augment, SceneCrops
    frames, labels, cls, teacher = _scene(H, W)
    size, n = (32, 32), 8
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    aug = None if augment is None else Augment(**augment)

    def make(**kw):
        return SceneCrops(t(frames), t(labels), t(cls), n_classes=2, crop=size, p_object=0.75, jitter=(40, 40),
                          augment=aug, mul=1.0, seed=13, **kw)

    crops, twin = make(teacher=t(teacher)), make()
    assert twin.last_teacher is None and crops.last_teacher is None
    for _ in range(2):                                   # (the second batch: the seed stream is untouched)
        got, want = crops.batch(n), twin.batch(n)
        assert twin.last_teacher is None
        for a, b in zip(got, want):
            kind = torch.uint8 if a.dtype == torch.uint8 else torch.int32
            assert a.shape == b.shape and torch.equal(a.view(kind), b.view(kind))
        for a, b in zip(crops.last, twin.last):
            assert torch.equal(a, b)
    cut = crops.last_teacher
    assert tuple(cut.shape) == (n, 2, 32, 32) and cut.dtype == torch.float32 and cut.device == crops.device
    rows, index, origin = (v.cpu().numpy() for v in crops.last)
    if augment is not None:
        assert (rows[:, 12] != 1.0).any() and (rows[:, 13] != 0.0).any()
    xs, ys = _source_pixels(rows, size)
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    whole = inside.reshape(n, -1).all(axis=1)
    if H >= 32:
        assert whole.any() and whole.all()               # at least one window lies inside (here: every one)
    else:
        assert (~whole).any()                            # at least one window overhangs (here: every one)
        assert (origin[:, 1] == -4).all() and int((~inside).sum()) == n * 8 * 32
    got = cut.cpu().numpy()
    unit = rows.copy()
    unit[:, 12], unit[:, 13] = 1.0, 0.0
    want, _ = LDO.warp_batch_ref(teacher, index, unit, size, 1.0, 0.0, -1.0)
    assert np.array_equal(want.astype(F32).astype(F64), want)
    assert np.array_equal(got.view(U32), want.astype(F32).view(U32))
    for i in range(n):
        for c in range(2):
            src = teacher[index[i], c][np.clip(ys[i], 0, H - 1), np.clip(xs[i], 0, W - 1)]
            assert np.array_equal(got[i, c].view(U32), np.where(inside[i], src, F32(-1.0)).view(U32)), (i, c)
    assert set(np.unique(index)) <= {0, 1}


def test_scene_crops_refuse_a_teacher_they_cannot_cut_exactly(dev):
    from unet_nested4tiny_objects_keypoints_amd import Augment, ObjectPaste, SceneCrops
    frames, labels, cls, teacher = _scene(80, 96)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    kw = dict(n_classes=2, crop=(32, 32), mul=1.0)
    SceneCrops(t(frames), t(labels), t(cls), teacher=t(teacher), **kw)
    for aug in (Augment(rotate=10.0), Augment(scale=(0.9, 1.1))):
        with pytest.raises(ValueError, match="resample"):
            SceneCrops(t(frames), t(labels), t(cls), augment=aug, teacher=t(teacher), **kw)
    with pytest.raises(ValueError, match="do not go together"):
        SceneCrops(t(frames), t(labels), t(cls), paste=ObjectPaste(patch_radius=1, core=0.5), teacher=t(teacher), **kw)
    nine = torch.rand(2, 9, 80, 96, device=dev)
    with pytest.raises(ValueError, match="classes"):
        SceneCrops(t(frames), t(labels), t(cls), n_classes=9, crop=(32, 32), mul=1.0, teacher=nine)
    with pytest.raises(ValueError):
        SceneCrops(t(frames), t(labels), t(cls), teacher=t(teacher)[:, :, :40], **kw)        # not the frames' size
    with pytest.raises(TypeError):
        SceneCrops(t(frames), t(labels), t(cls), teacher=t(teacher).double(), **kw)
    with pytest.raises(RuntimeError):
        SceneCrops(t(frames), t(labels), t(cls), teacher=torch.from_numpy(teacher), **kw)


# ------------------------------------------------------------------------------------------------ 12: unlabelled frame
@pytest.mark.parametrize("distill_ignored", [True, False])
def test_a_frame_under_one_ignore_rectangle_trains_on_the_teacher_alone(dev, distill_ignored):
    """Frames of 96 x 24 under one whole-frame ignore rectangle each, windows of 32 x 32 (eight rows of every window lie
    outside the frame: ignored by ignore_outside, and void in the teacher's cut): every target element is ignored, so
    every S_h is +0.0, and the gradients are w g_d of the composition where the teacher exists and +0.0 where it does
    not; with distill_ignored=False every gradient is +0.0."""
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions, SceneCrops, TeacherDistillLoss, ops
    H, W, n, w = 24, 96, 8, 0.75
    frames, labels, cls, teacher = _scene(H, W)
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    rect = torch.tensor([[[0.0, 0.0, W - 1.0, H - 1.0]]] * 2)
    crops = SceneCrops(t(frames), t(labels), t(cls), n_classes=2, crop=(32, 32), jitter=(40, 40), mul=1.0, seed=14,
                       ignore=IgnoreRegions(rect), ignore_outside=True, teacher=t(teacher))
    _, target, _, _ = crops.batch(n)
    q = crops.last_teacher
    assert bool((target < 0).all())
    void = q < 0
    assert abs(float(void.float().mean()) - 0.25) < 1e-6 and bool((q[~void] > 0).all())
    g = torch.Generator().manual_seed(15)
    outs = tuple((torch.rand(target.shape, generator=g) * 0.98 + 0.01).to(dev) for _ in range(3))
    crit = TeacherDistillLoss(weight=w, ignore_negative=True, distill_ignored=distill_ignored)
    crit.set_teacher(q)
    avg, grads = crit.mean_over_heads(outs, target)
    assert bool((_bits(crit.last_supervised) == 0).all())
    rows = target.shape[0] * target.shape[1]
    inv_heads, w32 = float(F32(1.0) / F32(3)), float(F32(w))
    for p, got in zip(outs, grads):
        if not distill_ignored:
            assert bool((_bits(got) == 0).all())
            continue
        _, gd = ops.focal_bce(p, torch.where(void, p, q), rows, 3.0)
        want = torch.where(void, torch.zeros_like(gd), w32 * (gd * inv_heads))
        assert _same_bits(got, want) and bool((got[~void] != 0).all()) and bool((_bits(got)[void] == 0).all())
    if distill_ignored:
        assert bool((crit.last_distill > 0).all()) and float(avg) > 0
    else:
        assert bool((_bits(crit.last_distill) == 0).all()) and int(_bits(avg)) == 0


# ----------------------------------------------------------------------------------------------------------- 13: ABI
def test_entry_point_refuses_bad_arguments_without_a_launch(dev):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    lib = _lib.lib()
    n, heads = 2051, 2
    blocks = int(lib.unetpp_focal_bce_blocks(n))
    bufs = {k: torch.full((n + 4,), float("nan"), device=dev) for k in ("p0", "p1", "t", "q", "g0", "g1")}
    ws = torch.full((2 * heads * blocks,), float("nan"), device=dev)
    loss = torch.full((1 + 3 * heads,), float("nan"), device=dev)
    wd = torch.full((4,), 0.5, device=dev)
    torch.cuda.synchronize()
    before = lib.unetpp_last_kernel_name()

    def call(**kw):
        a = dict(pred=(bufs["p0"].data_ptr(), bufs["p1"].data_ptr()), grad=(bufs["g0"].data_ptr(), bufs["g1"].data_ptr()),
                 n_heads=heads, heads=True, target=bufs["t"].data_ptr(), teacher=bufs["q"].data_ptr(), n=n, rows=3, gamma=3.0,
                 weight=wd.data_ptr(), gate=0, ignore=0, keep=1, partial=ws.data_ptr(), loss=loss.data_ptr())
        a.update(kw)
        hd = _lib.FocalHeads()
        hd.n_heads = a["n_heads"]
        for i in range(2):
            hd.pred[i], hd.grad[i] = a["pred"][i], a["grad"][i]
        return lib.unetpp_teacher_heads(C.byref(hd) if a["heads"] else None, a["target"], a["teacher"], a["n"], a["rows"],
                                        a["gamma"], a["weight"], a["gate"], a["ignore"], a["keep"], a["partial"], a["loss"],
                                        None)

    q, p1, g0 = bufs["q"].data_ptr(), bufs["p1"].data_ptr(), bufs["g0"].data_ptr()
    refused = [dict(teacher=None), dict(teacher=q + 4), dict(teacher=q + 8), dict(heads=False), dict(target=None),
               dict(weight=None), dict(partial=None), dict(loss=None), dict(n=0), dict(rows=0), dict(gamma=-1.0),
               dict(gamma=float("nan")), dict(gate=2), dict(ignore=2), dict(keep=2), dict(keep=-1),
               dict(target=bufs["t"].data_ptr() + 4), dict(weight=wd.data_ptr() + 2),
               dict(pred=(bufs["p0"].data_ptr(), p1 + 4)), dict(pred=(bufs["p0"].data_ptr(), None)),
               dict(grad=(g0 + 8, bufs["g1"].data_ptr())), dict(n_heads=0), dict(n_heads=_lib.MAX_HEADS + 1)]
    for kw in refused:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert lib.unetpp_last_kernel_name() == before
    for b in list(bufs.values()) + [ws, loss]:
        assert bool(torch.isnan(b).all())                   # nothing ran: every buffer keeps what was planted
    bufs["p0"].uniform_(), bufs["p1"].uniform_(), bufs["t"].uniform_(), bufs["q"].uniform_()
    assert call(grad=(None, None)) == 0                     # the same arguments, nothing refused
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all()) and bool(torch.isnan(bufs["g0"]).all())
