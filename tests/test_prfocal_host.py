"""Penalty-reduced focal loss without a GPU: the oracle (tests/prfocal_oracle.py) against a central difference of its own
loss, the criterion's CPU path against autograd's gradcheck and against the oracle, the planted mutations of the float32
restatement, and the argument checks of the class and of the C entry point."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import prfocal_oracle as PO

F32, F64, U32 = np.float32, np.float64, np.uint32


def _cpu(pred, target, **kw):
    """the criterion's CPU path on float32 numpy inputs -> (loss, grad, last_num_positives)"""
    from unet_nested4tiny_objects_keypoints_amd import PenaltyReducedFocalLoss
    p = torch.from_numpy(pred.copy()).requires_grad_(True)
    crit = PenaltyReducedFocalLoss(**kw)
    loss = crit(p, torch.from_numpy(target.copy()))
    loss.backward()
    return loss.detach(), p.grad.numpy(), crit.last_num_positives


@pytest.mark.parametrize("alpha,beta", PO.PARAMS)
def test_oracle_gradient_is_the_central_difference_of_its_loss(alpha, beta):
    """float64 throughout; elements inside the open gate, away from its edges by more than the step"""
    rng = np.random.default_rng(11)
    n, h = 64, 1e-6
    p = rng.random(n) * 0.9 + 0.05
    t = rng.random(n)
    t[::5] = 1.0
    lo, hi = PO.bounds(1e-4)

    def loss(pp):
        l, _, pos, _ = PO.terms64(pp, t, alpha, beta, lo, hi, 1.0)
        return l.sum() / max(int(pos.sum()), 1)

    _, dq, pos, opened = PO.terms64(p, t, alpha, beta, lo, hi, 1.0)
    assert opened.all() and int(pos.sum()) == 13
    for i in range(n):
        e = np.zeros(n)
        e[i] = h
        numeric = (loss(p + e) - loss(p - e)) / (2 * h)
        analytic = dq[i] / 13
        assert abs(numeric - analytic) <= 1e-6 * max(abs(analytic), 1e-3), (i, numeric, analytic)


@pytest.mark.parametrize("alpha,beta", PO.PARAMS)
def test_cpu_path_passes_gradcheck_in_float64(alpha, beta):
    from unet_nested4tiny_objects_keypoints_amd import PenaltyReducedFocalLoss
    g = torch.Generator().manual_seed(3)
    p = (torch.rand(2, 2, 3, 5, generator=g, dtype=torch.float64) * 0.9 + 0.05).requires_grad_(True)
    t = torch.rand(2, 2, 3, 5, generator=g, dtype=torch.float64)
    t[0, 0, 1, 1] = t[1, 1, 2, 4] = 1.0
    crit = PenaltyReducedFocalLoss(alpha=alpha, beta=beta)
    assert torch.autograd.gradcheck(lambda x: crit(x, t), (p,), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("n", [1, 9, 2051])
@pytest.mark.parametrize("positive", PO.POSITIVES)
@pytest.mark.parametrize("alpha,beta", PO.PARAMS)
def test_cpu_path_is_inside_the_oracles_intervals(n, positive, alpha, beta):
    (pred,), target = PO.inputs(n, positive=positive)
    params = dict(alpha=alpha, beta=beta, eps=1e-4, positive=positive)
    loss, grad, n_pos = _cpu(pred, target, **params)
    exp = PO.expected(pred, target, **params)
    assert n_pos.dtype == torch.int64 and n_pos.dim() == 0
    # (the closed gate gives a zero of either sign under autograd: values here, bits on the GPU)
    assert np.all(grad[exp.closed] == 0)
    assert PO.check(exp._replace(closed=np.zeros_like(exp.closed)), grad, int(n_pos), float(loss)) == []


def test_cpu_path_zero_positives_divides_by_one_and_nan_is_not_hidden():
    (pred,), target = PO.inputs(300, positives=0.0, plant=False)
    assert not (target >= 1.0).any()
    loss, grad, n_pos = _cpu(pred, target)
    exp = PO.expected(pred, target)
    assert int(n_pos) == 0 and exp.denom == 1 and np.isfinite(float(loss))
    assert PO.check(exp, grad, int(n_pos), float(loss)) == []
    pred[17] = np.nan
    loss, grad, _ = _cpu(pred, target)
    assert np.isnan(float(loss))
    exp = PO.expected(pred, target)
    assert PO.check(exp, grad, 0, float(loss)) == []
    assert PO.check(exp, grad, 0, 1.0) != []          # a finite loss would be a hidden NaN


def _cases():
    """(preds, target, params): planted elements with two heads at both thresholds, a target without positives, and
    the single element p = lo against t = 0, whose loss is one term"""
    lo, _ = PO.bounds(1e-4)
    out = []
    for positive in PO.POSITIVES:
        preds, target = PO.inputs(2051, heads=2, seed=1, positive=positive)
        out.append((preds, target, dict(alpha=2.0, beta=4.0, eps=1e-4, positive=positive)))
    preds, target = PO.inputs(300, heads=2, seed=2, positives=0.0, plant=False)
    out.append((preds, target, dict(PO.DEFAULTS)))
    out.append(([np.array([lo], F32)], np.zeros(1, F32), dict(PO.DEFAULTS)))
    return out


def test_restatement_passes_for_every_parameter_set():
    for positive in PO.POSITIVES:
        for alpha, beta in PO.PARAMS:
            for n in (1, 7, 2051):
                preds, target = PO.inputs(n, heads=3, seed=4, positive=positive)
                params = dict(alpha=alpha, beta=beta, eps=1e-4, positive=positive)
                assert PO.check_all(preds, target, PO.restate_f32(preds, target, **params), **params) == [], (n, params)


def test_restatement_passes_and_every_mutation_is_caught():
    cases = _cases()
    for preds, target, params in cases:
        assert PO.check_all(preds, target, PO.restate_f32(preds, target, **params), **params) == []
    assert len(PO.MUTATIONS) == 7
    for m in PO.MUTATIONS:
        caught = [bool(PO.check_all(preds, target, PO.restate_f32(preds, target, mutation=m, **params), **params))
                  for preds, target, params in cases]
        assert any(caught), "mutation %s passes the checks" % m
        if m == "zero_positives_divide_by_zero":
            assert caught[2]
        if m == "plain_log_of_one_minus_q":
            assert caught[3], "the single term at q = lo must show the plain log"
        if m == "positive_is_strictly_greater":
            assert caught[0] and caught[1]


def test_intervals_are_narrow():
    """tight enough to mean something: the median relative half-width of the gradient intervals stays below 2^-17"""
    (pred,), target = PO.inputs(4099)
    for alpha, beta in PO.PARAMS:
        exp = PO.expected(pred, target, alpha=alpha, beta=beta)
        live = ~exp.closed & (exp.want != 0)
        width = (exp.hi - exp.lo)[live] / 2 / np.abs(exp.want[live])
        assert np.median(width) < 2.0 ** -17, (alpha, beta, np.median(width))


def test_loss_depth_and_sizes_are_written_out():
    assert PO.loss_depth(1) == 8 + 6 + 2 + 1 + 10 + 3
    assert PO.loss_depth(PO.BIG_N, heads=3) == 8 + 6 + 2 + 2 + 10 + 3 + 5
    assert PO.blocks_of(PO.BIG_N) > PO.FINISH_THREADS                       # the finish takes a second trip
    assert -(-PO.BIG_N // PO.COUNT_CHUNK) > 2 * PO.COUNT_BLOCKS            # count workgroup 0 takes a third
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "unet_nested4tiny_objects_keypoints_amd", "csrc", "pr_focal.hip")).read()
    for line in ("constexpr int kPrThreads = 256;", "constexpr int kPrPerThread = 8;", "constexpr int kPrCountLoads = 4;",
                 "constexpr int kPrCountBlocks = 256;"):
        assert line in src, line


def test_class_argument_validation():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, PenaltyReducedFocalLoss
    for kw in (dict(alpha=-1.0), dict(beta=-0.5), dict(alpha=float("nan")), dict(beta=float("nan")), dict(alpha=float("inf")),
               dict(eps=0.0), dict(eps=0.5), dict(eps=-1e-4), dict(eps=1e-60), dict(eps=float("nan")), dict(positive=0.0),
               dict(positive=1.5), dict(positive=-0.1), dict(positive=float("nan"))):
        with pytest.raises(ValueError):
            PenaltyReducedFocalLoss(**kw)
    assert not issubclass(PenaltyReducedFocalLoss, FocalLoss_BCE_2d)
    c = PenaltyReducedFocalLoss()
    assert (c.alpha, c.beta, c.eps, c.positive) == (2.0, 4.0, 1e-4, 1.0) and c.last_num_positives is None
    assert c.mean_over_heads((torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2)), torch.zeros(1, 1, 2, 2)) is None
    with pytest.raises(ValueError):
        c(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 3))


def test_abi_stays_13_and_the_new_names_are_declared():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    assert _lib.ABI_VERSION == 14
    header = open(os.path.join(_lib.INCLUDE, "unetpp_hip.h")).read()
    for name in ("unetpp_pr_focal_workspace_bytes", "unetpp_pr_focal_heads"):
        assert name in _lib.SIGNATURES and name + "(" in header
    assert "pr_focal.hip" in _lib.SOURCES


def test_entry_point_argument_validation_without_gpu():
    """unetpp_pr_focal_heads refuses bad arguments before it touches the device (status codes, no throw)"""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    import __graft_entry__ as entry
    entry.build()
    lib = _lib.lib()
    assert lib.unetpp_abi_version() == 14
    assert lib.unetpp_pr_focal_workspace_bytes(3, 1) == 256 * 8 + 3 * 4
    assert lib.unetpp_pr_focal_workspace_bytes(8, PO.BIG_N) == 256 * 8 + 8 * 1026 * 4
    for bad in ((0, 1), (9, 1), (-1, 1), (1, 0), (1, -5), (1, 2 ** 43)):
        assert lib.unetpp_pr_focal_workspace_bytes(*bad) == 0, bad
    hd = _lib.FocalHeads()
    hd.n_heads = 1
    hd.pred[0] = 0x1000
    ok = dict(heads=ctypes.byref(hd), target=0x2000, n=16, alpha=2.0, beta=4.0, eps=1e-4, positive=1.0, ws=0x3000,
              n_pos=0x4000, loss=0x5000)
    nan, inf = float("nan"), float("inf")

    def call(**over):
        a = dict(ok, **over)
        return lib.unetpp_pr_focal_heads(a["heads"], a["target"], a["n"], a["alpha"], a["beta"], a["eps"], a["positive"],
                                         a["ws"], a["n_pos"], a["loss"], None)

    for over in (dict(heads=None), dict(target=None), dict(ws=None), dict(n_pos=None), dict(loss=None), dict(n=0), dict(n=-3),
                 dict(alpha=-1.0), dict(alpha=nan), dict(beta=-1.0), dict(beta=nan), dict(eps=0.0), dict(eps=0.5), dict(eps=-1e-4),
                 dict(eps=nan), dict(positive=0.0), dict(positive=1.0000001), dict(positive=-1.0), dict(positive=nan),
                 dict(target=0x2004), dict(ws=0x3004), dict(n_pos=0x4004)):
        assert call(**over) == -1, over
    for n in (0, 9, -1):
        hd.n_heads = n
        assert call() == -1, n
    hd.n_heads = 2          # the second head has no pred
    assert call() == -1
    hd.n_heads = 1
    hd.pred[0] = 0x1008     # not 16-byte aligned
    assert call() == -1
    hd.pred[0] = 0x1000
    hd.grad[0] = 0x6004
    assert call() == -1
