"""Top-k focal loss without a GPU: the oracle (tests/topk_oracle.py) against the criterion's CPU path and torch.topk,
the tie rule, k >= P against FocalLoss_BCE_2d, the planted mutations of the float32 restatement, and the argument
checks of the class and of the C entry point."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_oracle, topk_oracle as TO

F32, U32 = np.float32, np.uint32


def _cpu(pred, target, shape=None, **kw):
    """the criterion's CPU path on [R, P] numpy inputs -> (loss, grad [R, P], last_threshold [R], selected [R, P])"""
    from unet_nested4tiny_objects_keypoints_amd import TopKFocalLoss_BCE_2d
    rows, pixels = pred.shape
    shape = shape or (1, rows, 1, pixels)
    p = torch.from_numpy(pred.copy()).reshape(shape).requires_grad_(True)
    crit = TopKFocalLoss_BCE_2d(**kw)
    loss = crit(p, torch.from_numpy(target.copy()).reshape(shape))
    loss.backward()
    return loss.detach(), p.grad.reshape(rows, pixels).numpy(), crit.last_threshold.numpy(), crit


@pytest.mark.parametrize("rows,pixels,k", [(3, 1, 1), (2, 7, 2), (4, 65, 64), (2, 4097, 41), (2, 65, 70)])
@pytest.mark.parametrize("size_average", [False, True])
def test_oracle_agrees_with_the_cpu_path(rows, pixels, k, size_average):
    (pred,), target = TO.random_inputs(rows, pixels, seed=1)
    k_eff = min(k, pixels)
    denom = rows * k_eff if size_average else rows
    want = TO.expected(pred, target, k, 3, denom)
    loss, grad, kth, _ = _cpu(pred, target, k=k, gamma=3, size_average=size_average)
    # selection exactly: the gradient is non-zero on a selected element unless it is an exact hit
    nonzero = grad != 0
    assert np.array_equal(nonzero | (want.selected & want.iv.hit.reshape(rows, pixels)), want.selected)
    assert np.array_equal(kth.view(U32), want.kth.view(U32))
    assert loss_oracle.loss_ratio(float(loss), want.loss) <= 1.0, (float(loss), want.loss)
    # the selected |d| are torch.topk's, whatever the tie-breaking
    d = np.abs(pred - target)
    top = torch.topk(torch.from_numpy(d), k_eff, dim=1).values.numpy()
    mine = np.sort(np.where(want.selected, d, -1.0), axis=1)[:, ::-1][:, :k_eff]
    assert np.array_equal(top, mine)


def test_stable_sort_takes_the_first_indices_of_a_tie_run():
    """27 planted ties: argsort(~key, stable) and torch.sort(stable, descending) agree index for index, and the ties
    that are taken are the first of the run"""
    pred, target = TO.tie_inputs(1, 200, [(20, 29), (100, 109), (191, 200)], seed=2)
    key = TO.keys(pred, target)
    assert int((key[0] == F32(0.25).view(U32)).sum()) == 27
    above = int((key[0] > F32(0.25).view(U32)).sum())
    for take in (1, 5, 9, 10, 14, 26, 27):
        k = above + take
        idx = TO.select(key[0], k)
        order = torch.sort(torch.from_numpy(np.abs(pred - target)[0]), descending=True, stable=True).indices.numpy()[:k]
        assert np.array_equal(idx, order)
        ties = sorted(i for i in idx if key[0, i] == F32(0.25).view(U32))
        all_ties = [i for r in ((20, 29), (100, 109), (191, 200)) for i in range(*r)]
        assert ties == all_ties[:take]
        _, grad, kth, _ = _cpu(pred, target, k=k)
        assert sorted(np.flatnonzero(grad[0]).tolist()) == sorted(idx.tolist()) and kth[0] == F32(0.25)


@pytest.mark.parametrize("size_average", [False, True])
@pytest.mark.parametrize("kw", [dict(k=35), dict(k=40), dict(fraction=1.0)])
def test_all_pixels_is_the_focal_loss(kw, size_average):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    (pred,), target = TO.random_inputs(6, 35, seed=3)
    loss, grad, kth, _ = _cpu(pred, target, shape=(2, 3, 5, 7), size_average=size_average, **kw)
    p = torch.from_numpy(pred.copy()).reshape(2, 3, 5, 7).requires_grad_(True)
    ref = FocalLoss_BCE_2d(gamma=3, size_average=size_average)(p, torch.from_numpy(target).reshape(2, 3, 5, 7))
    ref.backward()
    assert float(loss) == float(ref.detach())
    assert np.array_equal(grad, p.grad.reshape(6, 35).numpy())
    assert np.array_equal(kth, np.abs(pred - target).min(1))


def _complaints(preds, target, k, result, denom):
    loss, grads, kth = result
    bad = []
    for h, p in enumerate(preds):
        want = TO.expected(p, target, k, 3, denom, heads=len(preds))
        bad += TO.check(want, grads[h], kth[h], loss[1 + h])
    return bad


def test_restatement_passes_and_every_mutation_is_caught():
    """the tie case catches the tie, count, gradient and heads mutations; its threshold 0.25 has no low mantissa bits,
    so the skipped digit pass is caught on the random rows, whose keys differ in them"""
    preds, target, k = TO.cut_inputs()
    cases = [(preds, target, k)] + [TO.random_inputs(3, 257, seed=7, heads=2) + (100,)]
    for preds, target, k in cases:
        denom = target.shape[0]
        assert _complaints(preds, target, k, TO.restate_f32(preds, target, k, 3, denom), denom) == []
    assert len(TO.MUTATIONS) >= 6
    for m in TO.MUTATIONS:
        caught = [bool(_complaints(p, t, k, TO.restate_f32(p, t, k, 3, t.shape[0], mutation=m), t.shape[0]))
                  for p, t, k in cases]
        assert caught[1] if m == "lowest_digit_skipped" else caught[0], "mutation %s passes the checks" % m


def test_restatement_on_random_rows_and_low_bits():
    """random keys differ in their low mantissa bits: the restatement's three digit passes find the oracle's selection,
    two passes do not"""
    preds, target = TO.random_inputs(3, 257, seed=7, heads=2)
    for k in (1, 2, 100, 256, 257, 300):
        assert _complaints(preds, target, k, TO.restate_f32(preds, target, k, 3, 3), 3) == []
    assert _complaints(preds, target, 100, TO.restate_f32(preds, target, 100, 3, 3, mutation="lowest_digit_skipped"), 3)


def test_loss_depth_is_written_out():
    assert TO.loss_depth(65536, 656, 128) == 4 * 65 + 6 + 3 + 1 + 10
    assert TO.loss_depth(65, 5, 2100, heads=3) == 4 + 6 + 3 + 3 + 10 + 3
    assert TO.loss_depth(64, 64, 2) == loss_oracle.loss_depth(128)


def test_class_argument_validation():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, TopKFocalLoss_BCE_2d
    for kw in (dict(), dict(k=3, fraction=0.5), dict(k=0), dict(k=-1), dict(k=2.5), dict(k=True), dict(fraction=0.0),
               dict(fraction=1.5), dict(fraction=-0.1)):
        with pytest.raises(ValueError):
            TopKFocalLoss_BCE_2d(**kw)
    assert not issubclass(TopKFocalLoss_BCE_2d, FocalLoss_BCE_2d)
    c = TopKFocalLoss_BCE_2d(fraction=0.01)
    assert (c.k_for(65536), c.k_for(50), c.k_for(4097), c.k_for(1)) == (656, 1, 41, 1)
    assert TopKFocalLoss_BCE_2d(k=7).k_for(5) == 5 and TopKFocalLoss_BCE_2d(fraction=1.0).k_for(33) == 33
    assert c.mean_over_heads((torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2)), torch.zeros(1, 1, 2, 2)) is None


def test_entry_point_argument_validation_without_gpu():
    """unetpp_topk_focal_heads refuses bad arguments before it touches the device (status codes, no throw)"""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    import __graft_entry__ as entry
    entry.build()
    lib = _lib.lib()
    assert lib.unetpp_topk_focal_workspace_bytes(4, 128, 65536) == 4 * 4 * max(128, lib.unetpp_focal_bce_blocks(128 * 65536))
    assert lib.unetpp_topk_focal_workspace_bytes(8, 5600, 33) == 8 * 5600 * 4
    for bad in ((0, 1, 1), (9, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 2 ** 31), (1, 2 ** 31, 1), (1, 2 ** 40, 2 ** 30)):
        assert lib.unetpp_topk_focal_workspace_bytes(*bad) == 0, bad
    hd = _lib.FocalHeads()
    hd.n_heads = 1
    hd.pred[0] = 0x1000
    ok = dict(heads=ctypes.byref(hd), target=0x2000, rows=2, P=16, k=3, denom=2, ws=0x3000, kth=0x4000, loss=0x5000)

    def call(**over):
        a = dict(ok, **over)
        return lib.unetpp_topk_focal_heads(a["heads"], a["target"], a["rows"], a["P"], a["k"], a["denom"], 3.0, a["ws"],
                                           a["kth"], a["loss"], None)

    for over in (dict(heads=None), dict(target=None), dict(ws=None), dict(kth=None), dict(loss=None), dict(k=0), dict(k=-3),
                 dict(P=0), dict(P=2 ** 31), dict(rows=0), dict(rows=2 ** 31), dict(denom=0), dict(target=0x2004),
                 dict(rows=2 ** 40, P=2 ** 30)):
        assert call(**over) == -1, over
    for n in (0, 9, -1):
        hd.n_heads = n
        assert call() == -1, n
    hd.n_heads = 2          # the second head has no pred
    assert call() == -1
    hd.n_heads = 1
    hd.pred[0] = 0x1008     # not 16-byte aligned
    assert call() == -1
