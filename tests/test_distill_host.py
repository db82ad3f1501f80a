"""Self-distillation across the heads without a GPU: the oracle (tests/distill_oracle.py) against central differences,
the class's torch path against the oracle and against FocalLoss_BCE_2d, the float32 restatement and its mutations, the
gate's coverage on the input sets, argument checks, the header and a from-scratch build with csrc/distill.hip in it."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import distill_oracle as DO
from tests import loss_oracle as LO

F32, F64, U32 = np.float32, np.float64, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [dict(teacher=t, gate=g, distill_ignored=di) for t, g, di in itertools.product(DO.TEACHERS, DO.GATES, (True, False))]


def _id(v):
    return "%s-%s-%s" % (v["teacher"], v["gate"], "keep" if v["distill_ignored"] else "drop")


def _crit(weight=0.5, **kw):
    from unet_nested4tiny_objects_keypoints_amd import HeadDistillLoss
    return HeadDistillLoss(weight=weight, **kw)


def _maps(arrays, dtype=torch.float32):
    """numpy [n] -> torch [1, 1, 1, n] (one row: rows = 1)"""
    return [torch.from_numpy(np.array(a)).to(dtype).view(1, 1, 1, -1) for a in arrays]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _plain_loop(preds, target, **kw):
    """the trainer's loop with FocalLoss_BCE_2d -> (avg, [grad])"""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    crit = FocalLoss_BCE_2d(**kw)
    leaves = [p.detach().clone().requires_grad_(True) for p in preds]
    avg = 0
    for p in leaves:
        avg = avg + crit(p, target)
    avg = 1.0 * avg / len(leaves)
    avg.backward()
    return avg.detach(), [p.grad for p in leaves]


# ------------------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("v", VARIANTS, ids=_id)
@pytest.mark.parametrize("gamma", [3.0, 2.0, 0.5])
def test_oracle_gradient_is_the_central_difference_of_its_loss(v, gamma):
    heads, n, rows, w = 3, 9, 2, 0.75
    preds, t = DO.inputs(heads, n, seed=3, ignore=True)
    exp = DO.expected(preds, t, rows, gamma, w, ignore=True, **v)
    ignored = [h.ignored for h in exp.heads]
    admitted = [h.admitted for h in exp.heads]
    teachers = [preds[DO.teacher_of(j, heads, v["teacher"])] for j in range(heads - 1)]
    step, checked = 1e-6, 0
    for j in range(heads):
        for i in range(n):
            q = teachers[j][i] if j < heads - 1 else preds[j][i]
            if abs(float(preds[j][i]) - float(t[i])) == 1.0 or abs(float(preds[j][i]) - float(q)) == 1.0:
                continue    # the pole at |d| = 1
            vals = []
            for s in (+step, -step):
                moved = [p.astype(F64) for p in preds]
                moved[j][i] += s
                vals.append(DO.loss_f64(moved, teachers, np.where(t < 0, 0.0, t), rows, gamma, w, ignored, admitted))
            diff = (vals[0] - vals[1]) / (2 * step)
            want = exp.heads[j].want[i]
            if exp.heads[j].zero_s[i] and exp.heads[j].zero_d[i]:
                assert want == 0.0
            hit_s = preds[j][i] == t[i] and not ignored[j][i]
            hit_d = j < heads - 1 and admitted[j][i] and preds[j][i] == q
            if gamma < 1.0 and (hit_s or hit_d):
                continue    # u^0.5 has no derivative at a hit
            assert abs(diff - want) <= 1e-5 * max(abs(want), 1e-3), (j, i, diff, want)
            checked += 1
    assert checked >= 15


def test_interval_is_a_point_where_both_terms_are_exact_zeros_and_narrow_elsewhere():
    preds, t = DO.inputs(3, 2051, seed=4, ignore=True)
    exp = DO.expected(preds, t, 4, 3.0, 0.5, ignore=True, distill_ignored=False)
    for h in exp.heads:
        both = h.zero_s & h.zero_d
        assert both.any() and (h.lo[both] == 0).all() and (h.hi[both] == 0).all() and (h.want[both] == 0).all()
        width = (h.hi - h.lo)[~both] / np.maximum(np.abs(h.want[~both]), 1e-30)
        assert np.median(width) < 1e-4


# ------------------------------------------------------------------------------------------------------- the class
def test_cpu_path_passes_gradcheck():
    g = torch.Generator().manual_seed(5)
    shape = (1, 2, 2, 5)
    t = torch.rand(shape, generator=g, dtype=torch.float64)
    t[0, 0, 0, 1] = t[0, 1, 1, 3] = -1.0
    for teacher, gate in itertools.product(DO.TEACHERS, DO.GATES):
        crit = _crit(0.75, teacher=teacher, gate=gate, ignore_negative=True, gamma=3)
        maps = [(torch.rand(shape, generator=g, dtype=torch.float64) * 0.8 + 0.1) for _ in range(3)]
        # a head that teaches enters the value as data: its numerical derivative would see that, its gradient must not
        free = (0, 1) if teacher == "last" else (0,)
        leaves = [m.clone().requires_grad_(True) for m in (maps[i] for i in free)]

        def f(*xs):
            full = list(maps)
            for i, x in zip(free, xs):
                full[i] = x
            return crit.heads_loss(tuple(full), t)

        assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("v", VARIANTS, ids=_id)
def test_cpu_path_lies_inside_the_oracles_intervals(v):
    failures, worst = [], 0.0
    for n in LO.TAIL_SIZES:
        preds, t = DO.inputs(3, n, seed=6, ignore=True)
        crit = _crit(0.5, ignore_negative=True, **v)
        avg, grads = crit.mean_over_heads(tuple(_maps(preds)), _maps([t])[0])
        assert avg.dim() == 0 and not avg.requires_grad and len(grads) == 3
        sup, dis = crit.last_supervised.numpy(), crit.last_distill.numpy()
        loss = np.concatenate([[avg.numpy()], sup + F32(0.5) * dis]).astype(F32)
        exp = DO.expected(preds, t, 1, 3.0, 0.5, ignore=True, **v)
        bad, r = DO.check(exp, loss, [g.numpy() for g in grads], sup, dis)
        worst = max(worst, r)
        failures += ["n = %d: %s" % (n, m) for m in bad]
    print("distill cpu path:", _id(v), "worst err / room %.3g" % worst)
    assert not failures, failures[:10]


@pytest.mark.parametrize("teacher", DO.TEACHERS)
def test_teacher_head_gradient_is_plain_focal_bit_for_bit(teacher):
    preds, t = DO.inputs(3, 2051, seed=7)
    maps, target = _maps(preds), _maps([t])[0]
    _, plain = _plain_loop(maps, target, gamma=3)
    _, grads = _crit(0.5, teacher=teacher, gate="teacher_better").mean_over_heads(tuple(maps), target)
    assert torch.equal(_bits(grads[2]), _bits(plain[2]))
    assert not torch.equal(_bits(grads[0]), _bits(plain[0]))     # (and a student's is something else)


@pytest.mark.parametrize("ignore", [False, True])
def test_weight_zero_is_the_plain_mean_over_heads_bit_for_bit(ignore):
    preds, t = DO.inputs(3, 2051, seed=8, ignore=ignore)
    maps, target = _maps(preds), _maps([t])[0]
    avg, _ = _plain_loop(maps, target, gamma=3, ignore_negative=ignore)
    crit = _crit(0.0, ignore_negative=ignore)
    got, grads = crit.mean_over_heads(tuple(maps), target)
    assert torch.equal(_bits(got), _bits(avg))
    assert float(crit.last_distill[0]) > 0 and float(crit.last_distill[2]) == 0      # reported, but it does not enter


def test_one_head_gives_forwards_value():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    (p,), t = DO.inputs(1, 2049, seed=9)
    (pm,), tm = _maps([p]), _maps([t])[0]
    crit = _crit(0.5)
    avg, grads = crit.mean_over_heads((pm,), tm)
    plain = FocalLoss_BCE_2d(gamma=3)(pm, tm)
    assert torch.equal(_bits(avg), _bits(crit(pm, tm))) and torch.equal(_bits(avg), _bits(plain))
    assert len(grads) == 1 and float(crit.last_distill[0]) == 0.0


def test_heads_loss_backward_scales_the_stored_gradients():
    preds, t = DO.inputs(3, 9, seed=10)
    maps, target = _maps(preds), _maps([t])[0]
    crit = _crit(0.5, teacher="next")
    avg, grads = crit.mean_over_heads(tuple(maps), target)
    leaves = [m.clone().requires_grad_(True) for m in maps]
    loss = crit.heads_loss(tuple(leaves), target)
    assert loss.dim() == 0 and torch.equal(_bits(loss), _bits(avg))
    (2.0 * loss).backward()
    for leaf, g in zip(leaves, grads):
        assert torch.equal(_bits(leaf.grad), _bits(g * 2.0))


def test_set_weight_changes_the_tensor_in_place():
    preds, t = DO.inputs(2, 9, seed=11)
    maps, target = _maps(preds), _maps([t])[0]
    crit = _crit(0.5)
    first, _ = crit.mean_over_heads(tuple(maps), target)
    held = crit.weight_tensor("cpu")
    crit.set_weight(0.25)
    assert crit.weight_tensor("cpu") is held and float(held) == 0.25 and crit.weight == 0.25
    second, _ = crit.mean_over_heads(tuple(maps), target)
    s, d = crit.last_supervised, crit.last_distill
    assert float(second) < float(first)
    assert abs(float(second) - float(((s + 0.25 * d).sum()) / 2)) <= 1e-6 * float(second)


# ------------------------------------------------------------------------------------------------- gate coverage
@pytest.mark.parametrize("heads", [2, 3, 8])
def test_gate_admits_between_a_quarter_and_three_quarters(heads):
    """a gate that admits everything or nothing would pass every other test unseen"""
    for n in (2047, 2048, 2049, 2051, 4099):
        for teacher in DO.TEACHERS:
            for ignore in (False, True):
                preds, t = DO.inputs(heads, n, seed=heads, ignore=ignore)
                share = DO.gated_share(preds, t, teacher, ignore)
                assert 0.25 <= share <= 0.75, (heads, n, teacher, ignore, share)
    preds, t = DO.inputs(3, 4099, seed=3, ignore=True)
    assert 0.05 <= float((t < 0).mean()) <= 0.15


# --------------------------------------------------------------------------------------- restatement and mutations
_CASE = dict(heads=3, n=2051, rows=4, gamma=3.0, weight=0.5)
_MUTATION_CONFIG = {
    "teacher_gets_gradient": dict(),
    "gate_inverted": dict(gate="teacher_better"),
    "gate_applied_to_ignored": dict(gate="teacher_better", ignore=True, distill_ignored=True),
    "weight_twice": dict(),
    "weight_read_as_one": dict(),
    "next_uses_last": dict(teacher="next"),
    "distill_dropped_on_ignored": dict(ignore=True, distill_ignored=True),
    "distill_kept_when_distill_ignored_false": dict(ignore=True, distill_ignored=False),
    "loss_misses_distill_sum": dict(),
}


def _restated(cfg, mutation=None, gamma=None):
    c = dict(_CASE, gamma=gamma or _CASE["gamma"])
    preds, t = DO.inputs(c["heads"], c["n"], seed=12, ignore=cfg.get("ignore", False))
    exp = DO.expected(preds, t, c["rows"], c["gamma"], c["weight"], **cfg)
    got = DO.restate_f32(preds, t, c["rows"], c["gamma"], c["weight"], mutation=mutation, **cfg)
    return DO.check(exp, *got)


@pytest.mark.parametrize("gamma", [3.0, 2.0, 0.5])
def test_restatement_passes(gamma):
    for v in VARIANTS:
        for ignore in (False, True):
            bad, worst = _restated(dict(v, ignore=ignore), gamma=gamma)
            assert bad == [], (v, ignore, bad[:3])
            assert worst <= 1.0


def test_mutation_table_is_complete():
    assert sorted(_MUTATION_CONFIG) == sorted(DO.MUTATIONS)


@pytest.mark.parametrize("mutation", DO.MUTATIONS)
def test_every_mutation_is_caught(mutation):
    cfg = _MUTATION_CONFIG[mutation]
    assert _restated(cfg)[0] == []
    bad, _ = _restated(cfg, mutation)
    assert bad, "the check accepts the mutation %s" % mutation


# ------------------------------------------------------------------------------------------------------ arguments
def test_class_argument_validation():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, _lib
    for kw in (dict(teacher="first"), dict(gate="student_better"), dict(weight=-0.1), dict(weight=float("nan")),
               dict(weight=float("inf")), dict(weight=1e39), dict(gamma=-1)):
        with pytest.raises(ValueError):
            _crit(**{"weight": 0.5, **kw})
    with pytest.raises(TypeError):
        _crit(weight=torch.tensor(0.5))
    crit = _crit()
    assert not isinstance(crit, FocalLoss_BCE_2d)
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            crit.set_weight(w)
    assert crit.weight == 0.5
    t = torch.rand(1, 1, 4, 4)
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


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


def test_ops_argument_validation_without_gpu(built_lib):
    from unet_nested4tiny_objects_keypoints_amd import ops
    t = torch.rand(1, 1, 4, 4)
    w = torch.full((1,), 0.5)
    p = [torch.rand(1, 1, 4, 4) for _ in range(2)]
    with pytest.raises(ValueError, match="heads"):
        ops.distill_heads([], t, 1, 3.0, w)
    with pytest.raises(ValueError, match="heads"):
        ops.distill_heads(p * 5, t, 1, 3.0, w)
    with pytest.raises(ValueError, match="teacher"):
        ops.distill_heads(p, t, 1, 3.0, w, teacher="first")
    with pytest.raises(ValueError, match="gate"):
        ops.distill_heads(p, t, 1, 3.0, w, gate="always")
    with pytest.raises(ValueError, match="weight_dev"):
        ops.distill_heads(p, t, 1, 3.0, torch.zeros(2))
    with pytest.raises(ValueError, match="weight_dev"):
        ops.distill_heads(p, t, 1, 3.0, 0.5)
    with pytest.raises(TypeError, match="weight_dev"):
        ops.distill_heads(p, t, 1, 3.0, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="weight_dev"):
        ops.distill_heads(p, t, 1, 3.0, torch.zeros(1, device="meta"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distill_heads(p, t, 1, 3.0, w)


def test_entry_point_refuses_bad_arguments_without_touching_the_device(built_lib):
    lib = built_lib.lib()
    hd = built_lib.FocalHeads()
    hd.n_heads = 2
    hd.pred[0], hd.pred[1] = 0x1000, 0x2000
    a = 0x3000   # (addresses are checked, never dereferenced: every call below is refused before a launch)

    def call(heads=hd, target=a, n=8, rows=1, gamma=3.0, weight=0x4000, teacher=0, gate=0, ignore=0, keep=1, partial=0x5000,
             loss=0x6000):
        return lib.unetpp_distill_heads(None if heads is None else C.byref(heads), target, n, rows, gamma, weight, teacher,
                                        gate, ignore, keep, partial, loss, None)

    assert call(heads=None) == -1 and call(target=None) == -1 and call(weight=None) == -1
    assert call(partial=None) == -1 and call(loss=None) == -1
    assert call(n=0) == -1 and call(rows=0) == -1 and call(gamma=-1.0) == -1 and call(gamma=float("nan")) == -1
    assert call(teacher=2) == -1 and call(gate=2) == -1 and call(ignore=2) == -1 and call(keep=-1) == -1
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
    assert re.search(r"\bint unetpp_distill_heads\s*\(", code)
    assert re.search(r"#define UNETPP_DISTILL_LAST 0\b", code) and re.search(r"#define UNETPP_DISTILL_NEXT 1\b", code)
    assert "added within v13: new entry points only" in text[:text.index("int unetpp_distill_heads")].rsplit("/*", 1)[1]
    assert "unetpp_distill_heads" in built_lib.SIGNATURES and "distill.hip" in built_lib.SOURCES
    assert built_lib.ABI_VERSION == 14 and built_lib.lib().unetpp_abi_version() == 14
    assert (built_lib.DISTILL_LAST, built_lib.DISTILL_NEXT) == (0, 1)


def test_library_builds_from_scratch_with_distill(tmp_path):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    out = _lib.build_library(force=True, out_path=str(tmp_path / "libunetpp_clean.so"), obj_dir=str(tmp_path / "obj"))
    assert os.path.exists(str(tmp_path / "obj" / "distill.o"))
    handle = C.CDLL(out)
    handle.unetpp_abi_version.restype = C.c_int
    assert handle.unetpp_abi_version() == 14
    assert hasattr(handle, "unetpp_distill_heads")
