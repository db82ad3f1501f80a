"""Distillation from an external map without a GPU: the oracle's self-checks (tests/teacher_oracle.py), the float32
restatement and its planted mutations, the coverage of the mask classes on the input sets the GPU tests use, the class's
torch path against the oracle and against FocalLoss_BCE_2d, set_teacher's buffer, argument checks of the class, of
ops.teacher_heads and of the C entry point, and the header."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import loss_oracle as LO
from tests import teacher_oracle as TO

F32, F64, U32 = np.float32, np.float64, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (gate, ignore, distill_ignored): distill_ignored only matters with ignore on
VARIANTS = [dict(gate=g, ignore=i, distill_ignored=k)
            for g, (i, k) in itertools.product(TO.GATES, ((False, True), (True, True), (True, False)))]


def _id(v):
    return "%s-%s" % (v["gate"], ("keep" if v["distill_ignored"] else "drop") if v["ignore"] else "labelled")


def _crit(weight=0.5, **kw):
    from unet_nested4tiny_objects_keypoints_amd import TeacherDistillLoss
    return TeacherDistillLoss(weight=weight, **kw)


def _maps(arrays, dtype=torch.float32):
    """numpy [n] -> torch [1, 1, 1, n] (one row: rows = 1)"""
    return [torch.from_numpy(np.array(a)).to(dtype).view(1, 1, 1, -1) for a in arrays]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("v", VARIANTS, ids=_id)
@pytest.mark.parametrize("gamma", [3.0, 2.0, 0.5])
def test_oracle_gradient_is_the_central_difference_of_its_loss(v, gamma):
    """the float64 loss with the teacher and the masks held fixed, differentiated numerically, every head included"""
    heads, n, rows, w = 3, 40, 2, 0.75
    preds, t, q = TO.inputs(heads, n, seed=3, ignore=v["ignore"], void=True)
    exp = TO.expected(preds, t, q, rows, gamma, w, **v)
    w32 = float(F32(w))

    def loss(moved):
        total = 0.0
        for j, h in enumerate(exp.heads):
            p = moved[j]
            us = np.maximum(np.abs(p - t.astype(F64)) - 1e-20, 0.0)
            ud = np.maximum(np.abs(p - q.astype(F64)) - 1e-20, 0.0)
            total += float(LO._l_and_g(np.where(h.ignored, 0.0, us), gamma)[0][~h.ignored].sum()) / rows
            total += w32 * float(LO._l_and_g(np.where(h.admitted, ud, 0.0), gamma)[0][h.admitted].sum()) / rows
        return total / heads

    step, checked = 1e-6, 0
    for j, h in enumerate(exp.heads):
        for i in range(n):
            ds, dd = abs(float(preds[j][i]) - float(t[i])), abs(float(preds[j][i]) - float(q[i]))
            if (not h.ignored[i] and ds == 1.0) or (h.admitted[i] and dd == 1.0):
                continue    # the pole at |d| = 1
            if gamma < 1.0 and ((not h.ignored[i] and ds == 0.0) or (h.admitted[i] and dd == 0.0)):
                continue    # u^0.5 has no derivative at a hit
            vals = []
            for s in (+step, -step):
                moved = [p.astype(F64) for p in preds]
                moved[j][i] += s
                vals.append(loss(moved))
            diff, want = (vals[0] - vals[1]) / (2 * step), h.want[i]
            if h.zero_s[i] and h.zero_d[i]:
                assert want == 0.0
            assert abs(diff - want) <= 1e-5 * max(abs(want), 1e-3), (j, i, diff, want)
            checked += 1
    assert checked >= 60


def test_masks_on_planted_elements():
    """-0.0 and +0.0 are a teacher, a negative element is none; an exact tie of the gate is kept out; an ignored element
    passes the gate and is admitted iff distill_ignored and not void"""
    p = np.array([0.25, 0.25, 0.25, 0.25, 0.25, 0.25, 0.9], F32)
    t = np.array([0.5, 0.5, 0.5, -1.0, -1.0, 0.5, 0.5], F32)
    q = np.array([0.75, -0.0, 0.0, 0.9, -0.5, -1e-30, 0.6], F32)
    ign, void, adm = TO.masks(p, q, t, "teacher_better", True, True)
    assert ign.tolist() == [False, False, False, True, True, False, False]
    assert void.tolist() == [False, False, False, False, True, True, False]
    assert adm.tolist() == [False, False, False, True, False, False, True]
    ign, void, adm = TO.masks(p, q, t, "none", True, False)
    assert adm.tolist() == [True, True, True, False, False, False, True]
    ign, void, adm = TO.masks(p, np.full(7, np.nan, F32), t, "none", False, True)
    assert not void.any() and adm.all()                                  # a NaN is not negative: nothing is hidden
    ign, void, adm = TO.masks(p, np.full(7, np.nan, F32), t, "teacher_better", False, True)
    assert not adm.any()


# the (heads, n, seed) of every masked case of tests/test_gpu_teacher.py
def test_every_mask_class_holds_five_percent_on_the_gpu_tests_inputs():
    from tests.test_gpu_teacher import MASKED_CASES
    assert len(MASKED_CASES) >= 10
    for heads, n, seed in MASKED_CASES:
        assert n >= TO.MIN_SHARE_N
        for v in VARIANTS:
            preds, t, q = TO.inputs(heads, n, seed, ignore=v["ignore"], void=True)
            exp = TO.expected(preds, t, q, 3, 3.0, 0.75, **v)
            thin = TO.thin_classes(exp, void=True, **v)
            assert thin == [], (heads, n, seed, v, thin)
            assert abs(float((q < 0).mean()) - 1.0 / 3.0) < 0.05      # a third of the teacher is void


# --------------------------------------------------------------------------------------- restatement and mutations
_CASE = dict(heads=3, n=2051, rows=4, gamma=3.0, weight=0.75, seed=12)   # (a product by 0.5 is exact: fused or not, the same bits)
_MUTATION_CONFIG = {
    "void_rule_le": dict(),
    "void_ignored_under_distill_ignored": dict(ignore=True, distill_ignored=True),
    "gate_le": dict(gate="teacher_better"),
    "ignored_element_fails_gate": dict(gate="teacher_better", ignore=True, distill_ignored=True),
    "deepest_head_without_teacher": dict(),
    "weight_applied_to_supervised": dict(),
    "fused_combine": dict(),
    "divisor_n": dict(),
    "gate_inverted": dict(gate="teacher_better"),
    "weight_twice": dict(),
}


def _restated(cfg, mutation=None, gamma=None, void=True):
    c = dict(_CASE, gamma=gamma or _CASE["gamma"])
    preds, t, q = TO.inputs(c["heads"], c["n"], c["seed"], ignore=cfg.get("ignore", False), void=void)
    exp = TO.expected(preds, t, q, c["rows"], c["gamma"], c["weight"], **cfg)
    got = TO.restate_f32(preds, t, q, c["rows"], c["gamma"], c["weight"], mutation=mutation, **cfg)
    if mutation is None:     # the restatement's masks are the oracle's
        for h, admit in zip(exp.heads, got[4]):
            assert np.array_equal(h.admitted, admit)
    return TO.check(exp, *got[:4])


@pytest.mark.parametrize("gamma", [3.0, 2.0, 0.5])
def test_restatement_passes(gamma):
    for v, void in itertools.product(VARIANTS, (False, True)):
        bad, worst = _restated(v, gamma=gamma, void=void)
        assert bad == [], (v, void, bad[:3])
        assert worst <= 1.0


def test_mutation_table_is_complete():
    assert sorted(_MUTATION_CONFIG) == sorted(TO.MUTATIONS) and len(TO.MUTATIONS) >= 8


@pytest.mark.parametrize("mutation", TO.MUTATIONS)
def test_every_mutation_is_caught(mutation):
    cfg = _MUTATION_CONFIG[mutation]
    assert _restated(cfg)[0] == []
    bad, _ = _restated(cfg, mutation)
    assert bad, "the check accepts the mutation %s" % mutation


# ------------------------------------------------------------------------------------------------------- the class
@pytest.mark.parametrize("v", VARIANTS, ids=_id)
def test_cpu_rule_lies_inside_the_oracles_intervals(v):
    failures, worst = [], 0.0
    for n in LO.TAIL_SIZES:
        preds, t, q = TO.inputs(3, n, seed=6, ignore=v["ignore"], void=True)
        crit = _crit(0.5, gate=v["gate"], ignore_negative=v["ignore"], distill_ignored=v["distill_ignored"])
        target = _maps([t])[0]
        crit.set_teacher(_maps([q])[0])
        avg, grads = crit.mean_over_heads(tuple(_maps(preds)), target)
        assert avg.dim() == 0 and not avg.requires_grad and len(grads) == 3
        sup, dis = crit.last_supervised.numpy(), crit.last_distill.numpy()
        loss = np.concatenate([[avg.numpy()], sup + F32(0.5) * dis]).astype(F32)
        exp = TO.expected(preds, t, q, 1, 3.0, 0.5, **v)
        bad, r = TO.check(exp, loss, [g.numpy() for g in grads], sup, dis, exact=False)
        worst = max(worst, r)
        failures += ["n = %d: %s" % (n, m) for m in bad]
    print("teacher cpu path:", _id(v), "worst err / room %.3g" % worst)
    assert not failures, failures[:10]


def test_cpu_rule_passes_gradcheck():
    g = torch.Generator().manual_seed(5)
    shape = (1, 2, 2, 5)
    t = torch.rand(shape, generator=g, dtype=torch.float64)
    t[0, 0, 0, 1] = t[0, 1, 1, 3] = -1.0
    q = torch.rand(shape, generator=g, dtype=torch.float32)
    q[0, 0, 1, 2] = q[0, 1, 1, 3] = -1.0
    for gate in TO.GATES:
        crit = _crit(0.75, gate=gate, ignore_negative=True, gamma=3)
        crit.set_teacher(q)
        leaves = [(torch.rand(shape, generator=g, dtype=torch.float64) * 0.8 + 0.1).requires_grad_(True) for _ in range(3)]
        assert torch.autograd.gradcheck(lambda *xs: crit.heads_loss(tuple(xs), t), leaves, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_set_teacher_keeps_its_buffer_and_reallocates_on_a_new_shape():
    crit = _crit()
    a, b = torch.rand(1, 2, 4, 4), torch.rand(1, 2, 4, 4)
    held = crit.set_teacher(a)
    ptr = held.data_ptr()
    assert held.data_ptr() != a.data_ptr() and torch.equal(held, a) and not held.requires_grad
    assert crit.set_teacher(b) is held and held.data_ptr() == ptr and torch.equal(held, b)
    assert crit.teacher_tensor(torch.zeros(1, 2, 4, 4)) is held
    other = crit.set_teacher(torch.rand(2, 2, 4, 4))
    assert other is not held and other.data_ptr() != ptr and len(crit._teacher) == 2
    assert crit.teacher_tensor(torch.zeros(1, 2, 4, 4)) is held            # the first shape keeps its buffer
    leaf = torch.rand(1, 2, 4, 4, requires_grad=True)
    assert not crit.set_teacher(leaf * 2.0).requires_grad                  # used detached
    crit.clear_teacher()
    assert crit._teacher == {}
    with pytest.raises(RuntimeError, match="no teacher"):
        crit.teacher_tensor(torch.zeros(1, 2, 4, 4))
    for bad, err in ((torch.rand(1, 2, 4, 4, dtype=torch.float64), TypeError), (np.zeros((1, 2, 4, 4), F32), TypeError),
                     (torch.rand(4, 4), ValueError)):
        with pytest.raises(err):
            crit.set_teacher(bad)


def test_set_teacher_changes_the_result():
    preds, t, q = TO.inputs(2, 40, seed=11)
    maps, target = _maps(preds), _maps([t])[0]
    crit = _crit(0.5)
    crit.set_teacher(_maps([q])[0])
    first, _ = crit.mean_over_heads(tuple(maps), target)
    crit.set_teacher(target)                       # a teacher that is the target: D_h = S_h
    second, _ = crit.mean_over_heads(tuple(maps), target)
    assert float(first) != float(second)
    assert torch.equal(_bits(crit.last_distill), _bits(crit.last_supervised))


def test_mean_over_heads_raises_without_a_teacher():
    crit = _crit()
    t = torch.rand(1, 1, 4, 4)
    heads = (torch.rand(1, 1, 4, 4), torch.rand(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="no teacher"):
        crit.mean_over_heads(heads, t)
    with pytest.raises(RuntimeError, match="no teacher"):
        crit.heads_loss(heads, t)
    crit.set_teacher(torch.rand(1, 1, 4, 5))       # another shape is no teacher for this target
    with pytest.raises(RuntimeError, match="no teacher"):
        crit.mean_over_heads(heads, t)
    crit.set_teacher(torch.rand(1, 1, 4, 4))
    avg, grads = crit.mean_over_heads(heads, t)
    assert avg.dim() == 0 and len(grads) == 2
    crit.clear_teacher()
    with pytest.raises(RuntimeError, match="no teacher"):
        crit.mean_over_heads(heads, t)


@pytest.mark.parametrize("ignore", [False, True])
def test_forward_on_one_map_is_focal_loss_bce_2d(ignore):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    preds, t, _ = TO.inputs(1, 2049, seed=9, ignore=ignore)
    (pm,), tm = _maps(preds), _maps([t])[0]
    crit = _crit(0.5, ignore_negative=ignore)      # (no teacher set: forward does not need one)
    plain = FocalLoss_BCE_2d(gamma=3, ignore_negative=ignore)(pm, tm)
    assert torch.equal(_bits(crit(pm, tm)), _bits(plain))
    assert not isinstance(crit, FocalLoss_BCE_2d)


def test_weight_zero_and_a_void_teacher_are_the_plain_mean_over_heads():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    preds, t, q = TO.inputs(3, 2051, seed=8)
    maps, target = _maps(preds), _maps([t])[0]
    plain = FocalLoss_BCE_2d(gamma=3)
    avg = 0
    for p in maps:
        avg = avg + plain(p, target)
    avg = 1.0 * avg / 3
    crit = _crit(0.0)
    crit.set_teacher(_maps([q])[0])
    got, _ = crit.mean_over_heads(tuple(maps), target)
    assert torch.equal(_bits(got), _bits(avg)) and bool((crit.last_distill > 0).all())   # reported, but it does not enter
    crit.set_weight(0.75)
    crit.set_teacher(torch.full_like(target, -1.0))
    got, _ = crit.mean_over_heads(tuple(maps), target)
    assert torch.equal(_bits(got), _bits(avg)) and bool((_bits(crit.last_distill) == 0).all())


def test_heads_loss_backward_scales_the_stored_gradients():
    preds, t, q = TO.inputs(3, 40, seed=10, void=True)
    maps, target = _maps(preds), _maps([t])[0]
    crit = _crit(0.5)
    crit.set_teacher(_maps([q])[0])
    avg, grads = crit.mean_over_heads(tuple(maps), target)
    leaves = [m.clone().requires_grad_(True) for m in maps]
    loss = crit.heads_loss(tuple(leaves), target)
    assert loss.dim() == 0 and torch.equal(_bits(loss), _bits(avg))
    (2.0 * loss).backward()
    for leaf, g in zip(leaves, grads):
        assert torch.equal(_bits(leaf.grad), _bits(g * 2.0))


def test_set_weight_changes_the_tensor_in_place():
    crit = _crit(0.5)
    held = crit.weight_tensor("cpu")
    crit.set_weight(0.25)
    assert crit.weight_tensor("cpu") is held and float(held) == 0.25 and crit.weight == 0.25


# ------------------------------------------------------------------------------------------------------ arguments
def test_class_argument_validation():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    for kw in (dict(gate="student_better"), dict(weight=-0.1), dict(weight=float("nan")), dict(weight=float("inf")),
               dict(weight=1e39), dict(gamma=-1)):
        with pytest.raises(ValueError):
            _crit(**{"weight": 0.5, **kw})
    with pytest.raises(TypeError):
        _crit(weight=torch.tensor(0.5))
    with pytest.raises(TypeError):
        _crit(teacher="last")                      # the teacher is a map, not a choice among the heads
    crit = _crit()
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            crit.set_weight(w)
    assert crit.weight == 0.5
    t = torch.rand(1, 1, 4, 4)
    crit.set_teacher(torch.rand(1, 1, 4, 4))
    with pytest.raises(ValueError):
        crit.mean_over_heads(tuple(torch.rand(1, 1, 4, 4) for _ in range(_lib.MAX_HEADS + 1)), t)
    with pytest.raises(ValueError):
        crit.mean_over_heads((), t)
    with pytest.raises(ValueError):
        crit.mean_over_heads(torch.rand(1, 1, 4, 4), t)
    with pytest.raises(ValueError):
        crit.mean_over_heads((torch.rand(1, 1, 4, 5),), t)
    with pytest.raises(ValueError):
        crit.heads_loss((torch.rand(1, 1, 4, 5),), t)
    got = crit.mean_over_heads(tuple(torch.rand(1, 1, 4, 4) for _ in range(_lib.MAX_HEADS)), t)
    assert got is not None and len(got[1]) == _lib.MAX_HEADS
    one = crit.mean_over_heads((torch.rand(1, 1, 4, 4),), t)
    assert one is not None and len(one[1]) == 1


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


def test_ops_argument_validation_without_gpu(built_lib):
    from unet_nested4tiny_objects_keypoints_amd import ops
    t = torch.rand(1, 1, 4, 4)
    q = torch.rand(1, 1, 4, 4)
    w = torch.full((1,), 0.5)
    p = [torch.rand(1, 1, 4, 4) for _ in range(2)]
    with pytest.raises(ValueError, match="gate"):
        ops.teacher_heads(p, t, q, 1, 3.0, w, gate="always")
    with pytest.raises(ValueError, match="weight_dev"):
        ops.teacher_heads(p, t, q, 1, 3.0, torch.zeros(2))
    with pytest.raises(ValueError, match="weight_dev"):
        ops.teacher_heads(p, t, q, 1, 3.0, 0.5)
    with pytest.raises(TypeError, match="weight_dev"):
        ops.teacher_heads(p, t, q, 1, 3.0, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="weight_dev"):
        ops.teacher_heads(p, t, q, 1, 3.0, torch.zeros(1, device="meta"))
    with pytest.raises(TypeError, match="teacher"):
        ops.teacher_heads(p, t, None, 1, 3.0, w)
    with pytest.raises(TypeError, match="teacher"):
        ops.teacher_heads(p, t, q.double(), 1, 3.0, w)
    with pytest.raises(ValueError, match="teacher"):
        ops.teacher_heads(p, t, q.to("meta"), 1, 3.0, w)
    with pytest.raises(ValueError, match="teacher"):
        ops.teacher_heads(p, t, torch.rand(1, 1, 4, 5), 1, 3.0, w)
    with pytest.raises(ValueError, match="heads"):
        ops.teacher_heads([], t, q, 1, 3.0, w)
    with pytest.raises(ValueError, match="heads"):
        ops.teacher_heads(p * 5, t, q, 1, 3.0, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.teacher_heads(p, t, q, 1, 3.0, w)


def test_entry_point_refuses_bad_arguments_without_touching_the_device(built_lib):
    lib = built_lib.lib()
    hd = built_lib.FocalHeads()
    hd.n_heads = 2
    hd.pred[0], hd.pred[1] = 0x1000, 0x2000
    a = 0x3000   # (addresses are checked, never dereferenced: every call below is refused before a launch)

    def call(heads=hd, target=a, teacher=0x8000, n=8, rows=1, gamma=3.0, weight=0x4000, gate=0, ignore=0, keep=1,
             partial=0x5000, loss=0x6000):
        return lib.unetpp_teacher_heads(None if heads is None else C.byref(heads), target, teacher, n, rows, gamma, weight,
                                        gate, ignore, keep, partial, loss, None)

    assert call(teacher=None) == -1 and call(teacher=0x8004) == -1 and call(teacher=0x8008) == -1
    assert call(heads=None) == -1 and call(target=None) == -1 and call(weight=None) == -1
    assert call(partial=None) == -1 and call(loss=None) == -1
    assert call(n=0) == -1 and call(rows=0) == -1 and call(gamma=-1.0) == -1 and call(gamma=float("nan")) == -1
    assert call(gate=2) == -1 and call(ignore=2) == -1 and call(keep=-1) == -1 and call(keep=2) == -1
    assert call(target=a + 4) == -1 and call(weight=0x4002) == -1
    hd.pred[1] = 0x2004
    assert call() == -1
    hd.pred[1] = None
    assert call() == -1
    hd.pred[1] = 0x2000
    hd.grad[0] = 0x7008
    assert call() == -1
    hd.grad[0] = None
    for bad in (0, built_lib.MAX_HEADS + 1):
        hd.n_heads = bad
        assert call() == -1


def test_header_declares_the_entry_point_and_the_abi_is_still_13(built_lib):
    text = open(os.path.join(ROOT, "include", "unetpp_hip.h")).read()
    assert re.search(r"#define UNETPP_ABI_VERSION 14\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint unetpp_teacher_heads\s*\(", code)
    assert "added within v13: new entry points only" in text[:text.index("int unetpp_teacher_heads")].rsplit("/*", 1)[1]
    assert "unetpp_teacher_heads" in built_lib.SIGNATURES and "distill.hip" in built_lib.SOURCES
    assert len(built_lib.SIGNATURES["unetpp_teacher_heads"][1]) == 13
    assert built_lib.ABI_VERSION == 14 and built_lib.lib().unetpp_abi_version() == 14
