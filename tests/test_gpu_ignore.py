"""Ignore regions on the GPU, against tests/ignore_oracle.py:
  (1) unetpp_target_ignore bit for bit against the mark oracle, guard bytes behind the target, a bit pattern in the
      elements it must not touch; rectangles inside, across window and tile edges, outside, single pixels, padding,
      class-specific and overlapping; R = 0, 1, 300; the four window kinds; `outside`; an all-fill sample; a small grid
      and a second class group; refusals;
  (2) the three *_ignore loss calls: non-ignored gradients are the plain call's bits, ignored ones +0.0, n_pos and kth
      exact, every loss inside the plain oracle's bound over the masked terms; without a negative target every output is
      the plain call's; a NaN target is not ignored;
  (3) the criteria, train_step, GraphedTrainStep, SceneCrops and evaluate end to end."""
import copy

import numpy as np
import pytest
import torch

from tests import crops_oracle as co
from tests import ignore_oracle as io
from tests import loss_oracle, prfocal_oracle, topk_oracle
from tests.loss_oracle import ulps

pytestmark = pytest.mark.gpu
F32, U32, I32 = np.float32, np.uint32, np.int32
GUARD = 64
PATTERN = np.array([0x3F2A5A5B], dtype=U32).view(F32)[0]        # what the untouched elements of a target hold (0.6654...)
GUARD_BITS = 0x7FC0BEEF                                          # a NaN behind the target


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# (1) -----------------------------------------------------------------------------------------------------------------
def _mark(dev, case, C_, size, outside, prefill=None):
    """unetpp_target_ignore through the C ABI on a target pre-filled with PATTERN (or `prefill` [N, C, Ho, Wo]) and a
    guard behind it -> the target as numpy"""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    from unet_nested4tiny_objects_keypoints_amd.ops import _ptr, _stream, check
    N, (Ho, Wo), (Hs, Ws) = len(case["index"]), size, case["src_size"]
    n = N * C_ * Ho * Wo
    buf = torch.empty(n + GUARD, dtype=torch.float32, device=dev)
    buf[:n] = float(PATTERN) if prefill is None else _t(prefill, dev).reshape(-1)
    buf[n:].view(torch.int32).fill_(GUARD_BITS)
    rects, cls = case["rects"], case["rect_class"]
    M, R = rects.shape[0], rects.shape[1]
    rd, cd = (_t(rects, dev), _t(cls, dev)) if R else (None, None)
    index, rows = _t(case["index"], dev), _t(case["rows"], dev)
    check(_lib.lib().unetpp_target_ignore(_ptr(rd), _ptr(cd), M, R, _ptr(index), N, _ptr(rows), C_, Ho, Wo, Hs, Ws,
                                          1 if outside else 0, _ptr(buf), _stream()), "unetpp_target_ignore")
    torch.cuda.synchronize()
    assert bool((buf[n:].view(torch.int32) == GUARD_BITS).all()), "the guard behind the target was written"
    return buf[:n].view(N, C_, Ho, Wo).cpu().numpy()


def _want(case, C_, size, outside, prefill=None):
    N = len(case["index"])
    base = np.full((N, C_) + tuple(size), PATTERN, dtype=F32) if prefill is None else prefill
    mask = io.mark_mask(case["rects"], case["rect_class"], case["index"], case["rows"], C_, size, case["src_size"], outside)
    return io.apply_mark(base, mask), mask


@pytest.mark.parametrize("R", [0, 1, 300])
@pytest.mark.parametrize("shape", io.MARK_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_mark_against_the_oracle(dev, shape, R):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    N, C_, Ho, Wo = shape
    first = io.MARK_SHAPES.index(shape) + [0, 1, 300].index(R)          # every sample slot sees every window kind
    for outside in (False, True):
        for kind0 in ([first] if R != 300 else [first, first + 1, first + 2, first + 3]):
            case = io.mark_case(N, C_, Ho, Wo, R, first_kind=kind0)
            got = _mark(dev, case, C_, (Ho, Wo), outside)
            if R > 0 or outside:
                assert _lib.lib().unetpp_last_kernel_name() == b"target_ignore"
            want, mask = _want(case, C_, (Ho, Wo), outside)
            assert np.array_equal(got.view(I32), want.view(I32)), (shape, R, outside, case["kinds"],
                                                                    int((got.view(I32) != want.view(I32)).sum()))
            if R != 1:                                                   # (the windows lie inside their frames;
                assert mask.any() == (R > 0 or (outside and N >= 3))     # a turned window may miss the one rectangle)
            again = _mark(dev, case, C_, (Ho, Wo), outside)
            assert np.array_equal(got.view(I32), again.view(I32))
            if N >= 3:                                                   # an index outside [0, M)
                assert (got[1] == -1).all() if outside else (got[1].view(I32) == PATTERN.view(I32)).all()


def test_mark_outside_and_the_all_fill_sample(dev):
    case = io.outside_case()
    C_, size = case["C"], case["out_size"]
    for outside in (True, False):
        got = _mark(dev, case, C_, size, outside)
        want, mask = _want(case, C_, size, outside)
        assert np.array_equal(got.view(I32), want.view(I32)), outside
        assert mask[3].all() == outside and mask[3].any() == outside     # index = -1
    assert (got[0, 0, 4:12, 12:19] == -1).all()                          # (outside off) the rectangle alone, sample 0


def test_mark_wins_over_a_label_and_leaves_the_rest(dev):
    """on a real target: -1 where the oracle marks, every other element's bits as points_target wrote them"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    N, C_, Ho, Wo = 3, 4, 40, 48
    labels = co.target_case(N, C_, Ho, Wo, 7)
    case = io.mark_case(N, C_, Ho, Wo, 300)
    case["rects"][0, 0] = (co.X0 + Wo // 3 - 2, co.Y0 + Ho // 2 - 2, co.X0 + Wo // 3 + 2, co.Y0 + Ho // 2 + 2)   # over a label
    target = ops.points_target(_t(labels["labels"], dev), _t(labels["label_class"], dev), _t(case["index"], dev),
                               _t(case["rows"], dev), C_, (Ho, Wo), 3.0).cpu().numpy()
    assert target[0, 0, Ho // 2, Wo // 3] == 1.0
    got = _mark(dev, case, C_, (Ho, Wo), True, prefill=target)
    want, mask = _want(case, C_, (Ho, Wo), True, prefill=target)
    assert np.array_equal(got.view(I32), want.view(I32)) and got[0, 0, Ho // 2, Wo // 3] == -1.0
    # through ops, in place
    t2 = _t(target, dev)
    out = ops.target_ignore(t2, _t(case["rects"], dev), _t(case["rect_class"], dev), _t(case["index"], dev),
                            _t(case["rows"], dev), case["src_size"], outside=True)
    assert out.data_ptr() == t2.data_ptr() and np.array_equal(out.cpu().numpy().view(I32), want.view(I32))


def test_mark_small_grid_and_a_second_class_group(dev):
    from tests.helpers import usable_cus
    N, C_, Ho, Wo = 1, 40, 33, 70                                        # classes 32..39 take a second group
    case = io.mark_case(N, C_, Ho, Wo, 300)
    case["rect_class"][0, 1] = 35
    case["rect_class"][0, 8] = 32
    got = _mark(dev, case, C_, (Ho, Wo), True)
    want, mask = _want(case, C_, (Ho, Wo), True)
    assert np.array_equal(got.view(I32), want.view(I32))
    assert (mask[0, 35] & ~mask[0, 34]).any() and (mask[0, 32] & ~mask[0, 33]).any()
    big = io.mark_case(2, 3, 129, 257, 300, first_kind=3)               # 90 units of (sample, tile)
    full = _mark(dev, big, 3, (129, 257), True)
    with usable_cus(8):                                                  # 64 workgroups: some take a second unit
        small = _mark(dev, big, 3, (129, 257), True)
    assert np.array_equal(full.view(I32), small.view(I32))
    assert np.array_equal(full.view(I32), _want(big, 3, (129, 257), True)[0].view(I32))


def test_mark_refusals(dev):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    lib = _lib.lib()
    case = io.mark_case(2, 2, 33, 70, 1)
    rd, cd, idx, rows = (_t(case[k], dev) for k in ("rects", "rect_class", "index", "rows"))
    tgt = torch.full((2, 2, 33, 70), float(PATTERN), device=dev)
    good = dict(rects=rd.data_ptr(), rect_class=cd.data_ptr(), M=2, R=1, index=idx.data_ptr(), N=2, params=rows.data_ptr(),
                C=2, Ho=33, Wo=70, Hs=2400, Ws=2600, outside=1, target=tgt.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.unetpp_target_ignore(a["rects"], a["rect_class"], a["M"], a["R"], a["index"], a["N"], a["params"],
                                        a["C"], a["Ho"], a["Wo"], a["Hs"], a["Ws"], a["outside"], a["target"], None)

    for bad in (dict(rects=None), dict(rect_class=None), dict(index=None), dict(params=None), dict(target=None), dict(M=0),
                dict(R=-1), dict(N=0), dict(C=0), dict(C=65536), dict(Ho=0), dict(Wo=-1), dict(Hs=0), dict(Ws=0),
                dict(Ho=(1 << 24) + 1), dict(Ws=(1 << 24) + 1)):
        assert call(**bad) == -1, bad
    assert call(R=0, outside=0, rects=None, rect_class=None) == 0
    torch.cuda.synchronize()
    assert bool((tgt == float(PATTERN)).all())                           # nothing was touched


# (2) -----------------------------------------------------------------------------------------------------------------
SIZES = loss_oracle.TAIL_SIZES + (3 * loss_oracle.BLOCK + 5,)            # the tails, and several workgroups


def _dev_list(arrs, dev):
    return [_t(np.array(a, dtype=F32), dev) for a in arrs]


def _focal(dev, preds, target, rows, gamma=3.0, ignore=True):
    from unet_nested4tiny_objects_keypoints_amd import ops
    loss, grads = ops.focal_bce_heads(_dev_list(preds, dev), _t(target, dev), rows, gamma, ignore=ignore)
    return loss.cpu().numpy(), [g.cpu().numpy() for g in grads]


def _topk(dev, preds, target, k, denom, gamma=3.0, ignore=True):
    from unet_nested4tiny_objects_keypoints_amd import ops
    rows = target.shape[0]                                               # [R, P] as R maps of 1 x P pixels
    loss, grads, kth = ops.topk_focal_heads(_dev_list([p.reshape(rows, 1, -1) for p in preds], dev),
                                            _t(target.reshape(rows, 1, -1), dev), k, denom, gamma, ignore=ignore)
    return loss.cpu().numpy(), [g.cpu().numpy().reshape(rows, -1) for g in grads], kth.cpu().numpy()


def _pr(dev, preds, target, ignore=True, **params):
    from unet_nested4tiny_objects_keypoints_amd import ops
    kw = dict(prfocal_oracle.DEFAULTS, **params)
    loss, grads, n_pos = ops.pr_focal_heads(_dev_list(preds, dev), _t(target, dev), kw["alpha"], kw["beta"], kw["eps"],
                                            kw["positive"], ignore=ignore)
    return loss.cpu().numpy(), [g.cpu().numpy() for g in grads], int(n_pos)


def _plain_bits_outside(got, plain, ign, what):
    """the gradient at every non-ignored element is the plain entry point's, bit for bit"""
    keep = ~np.asarray(ign).ravel()
    for h, (a, b) in enumerate(zip(got, plain)):
        a, b = a.ravel().view(U32), b.ravel().view(U32)
        assert np.array_equal(a[keep], b[keep]), (what, h, int((a[keep] != b[keep]).sum()))


def _equal_results(a, b):
    for x, y in zip(a, b):
        if isinstance(x, list):
            assert all(np.array_equal(u.view(U32), v.view(U32)) for u, v in zip(x, y))
        elif isinstance(x, np.ndarray):
            assert np.array_equal(x.view(U32), y.view(U32)), (x, y)
        else:
            assert x == y


@pytest.mark.parametrize("heads", [1, 3])
def test_focal_ignore(dev, heads):
    failures = []
    for n in SIZES:
        preds, t = loss_oracle.heads_inputs(heads, n, seed=heads)
        ign = io.plant_negatives(preds, t, share=0.25, seed=heads) if n >= 2 else np.zeros(n, bool)
        for gamma, rows in ((3.0, 6), (2.0, 1), (0.5, 3)):
            loss, grads = _focal(dev, preds, t, rows, gamma)
            failures += ["n = %d, gamma = %r: %s" % (n, gamma, m) for m in io.check_focal(preds, t, gamma, rows, loss, grads)]
            # the plain call on the same inputs: its loss is a NaN (the poison), its gradients elsewhere are these bits
            _, plain = _focal(dev, preds, t, rows, gamma, ignore=False)
            _plain_bits_outside(grads, plain, ign, (n, gamma))
        assert ign.any() == (n >= 2) and not ign.all()
    assert not failures, failures[:10]


@pytest.mark.parametrize("heads", [1, 3])
def test_prfocal_ignore(dev, heads):
    failures = []
    for n in SIZES:
        preds, t = prfocal_oracle.inputs(n, heads=heads, seed=heads)
        ign = io.plant_negatives(preds, t, share=0.25, seed=heads) if n >= 2 else np.zeros(n, bool)
        for alpha, beta in ((2.0, 4.0), (2.5, 3.5), (0.0, 0.0)):
            got = _pr(dev, preds, t, alpha=alpha, beta=beta)
            failures += ["n = %d, (%r, %r): %s" % (n, alpha, beta, m)
                         for m in io.check_prfocal(preds, t, got, alpha=alpha, beta=beta)]
            plain = _pr(dev, preds, t, ignore=False, alpha=alpha, beta=beta)
            _plain_bits_outside(got[1], plain[1], ign, (n, alpha, beta))
            assert got[2] == plain[2] == int((t >= 1.0).sum())           # n_pos: exact, and the plain call's
    assert not failures, failures[:10]


TOPK_SHAPES = [(3, p) for p in (1, 3, 4, 5, 7, 8, 9, 2047, 2048, 2049, 2051, 4099)] + [(5, 3 * 1024 + 5)]


@pytest.mark.parametrize("heads", [1, 3])
def test_topk_ignore(dev, heads):
    """against the oracle, and bit for bit against the plain call on the sanitised inputs (ignored elements replaced by
    exact hits pred == target == 0: key 0, term 0 -- unlike the other two losses a top-k gradient depends on the other
    elements of its row, through the selection).  Rows of an odd length start off a 16-byte boundary."""
    failures = []
    for rows, pixels in TOPK_SHAPES:
        preds, t = topk_oracle.random_inputs(rows, pixels, seed=heads, heads=heads)
        if rows * pixels >= 2:
            io.plant_negatives(preds, t, share=0.25, seed=heads)
        for k in sorted({1, max(1, pixels // 4), max(1, pixels - 2), pixels}):
            denom = rows
            got = _topk(dev, preds, t, k, denom)
            failures += ["%dx%d, k = %d: %s" % (rows, pixels, k, m) for m in io.check_topk(preds, t, k, 3.0, denom, *got)]
            clean = [io.sanitise(p, t)[0] for p in preds]
            plain = _topk(dev, clean, io.sanitise(preds[0], t)[1], k, denom, ignore=False)
            _equal_results((got[0], got[2]), (plain[0], plain[2]))            # every loss and kth
            _plain_bits_outside(got[1], plain[1], io.ignored(t), (rows, pixels, k))   # (k >= P: the plain call writes -0.0 at a hit)
    assert not failures, failures[:10]


def test_topk_ignore_k_above_the_live_keys_a_dead_row_and_a_fraction(dev):
    from unet_nested4tiny_objects_keypoints_amd import TopKFocalLoss_BCE_2d
    # k above the number of non-zero keys: ignored elements are selected, and still contribute +0.0
    preds, t = topk_oracle.random_inputs(3, 300, seed=9, heads=2)
    io.plant_negatives(preds, t, share=0.4, seed=9)
    t[1, :] = np.where(np.arange(300) % 2 == 0, F32(-1.0), F32(-np.inf))     # all of a row ignored
    for p in preds:
        p[1, ::3] = np.nan
    live = int((~io.ignored(t[0])).sum())
    for k in (live + 5, 299, 300):
        got = _topk(dev, preds, t, k, 3)
        assert io.check_topk(preds, t, k, 3.0, 3, *got) == [], k
        assert (got[2][:, 1].view(U32) == 0).all()                           # the dead row: kth = +0.0
        assert all((g[1].view(U32) == 0).all() for g in got[1])
    # fraction = 0.01 on [2, 2, 33, 70]: k = 24 of 2310, rows off a 16-byte boundary
    preds, t = topk_oracle.random_inputs(4, 33 * 70, seed=10, heads=3)
    io.plant_negatives(preds, t, share=0.25, seed=10)
    crit = TopKFocalLoss_BCE_2d(fraction=0.01, ignore_negative=True)
    assert crit.k_for(33 * 70) == 24
    outs = [_t(p, dev).view(2, 2, 33, 70) for p in preds]
    value, grads = crit.mean_over_heads(outs, _t(t, dev).view(2, 2, 33, 70))
    loss = np.concatenate([[float(value)], [0.0] * 3]).astype(F32)
    want = [io.topk_expected(p, t, 24, 3.0, 4, 3) for p in preds]
    for h, (w, ign) in enumerate(want):
        loss[1 + h] = w.loss[0]                                               # (the heads' own values are checked through ops below)
        assert topk_oracle.check(w, grads[h].cpu().numpy().reshape(4, -1), crit.last_threshold[h].cpu().numpy(), w.loss[0]) == []
        assert io.plus_zero(grads[h].cpu().numpy(), ign) == []
    got = _topk(dev, preds, t, 24, 4)
    assert io.check_topk(preds, t, 24, 3.0, 4, *got) == [] and got[0][0].view(U32) == np.float32(float(value)).view(U32)


def test_without_a_negative_target_every_output_is_the_plain_call(dev):
    n = SIZES[-1]
    preds, t = loss_oracle.heads_inputs(3, n, seed=11)
    t[5] = F32(-0.0)
    for gamma in (3.0, 0.5):
        a, b = _focal(dev, preds, t, 6, gamma), _focal(dev, preds, t, 6, gamma, ignore=False)
        _equal_results(a, b)
    p2, t2 = [p.reshape(11, -1) for p in preds], t.reshape(11, -1)           # 6149 = 11 x 559
    for k in (7, t2.shape[1]):
        _equal_results(_topk(dev, p2, t2, k, 11), _topk(dev, p2, t2, k, 11, ignore=False))
    preds, t = prfocal_oracle.inputs(n, heads=3, seed=11)
    t[5] = F32(-0.0)
    for ab in ((2.0, 4.0), (2.5, 3.5)):
        _equal_results(_pr(dev, preds, t, alpha=ab[0], beta=ab[1]), _pr(dev, preds, t, ignore=False, alpha=ab[0], beta=ab[1]))


def test_a_nan_target_is_not_ignored(dev):
    preds, t = loss_oracle.heads_inputs(2, 2051, seed=12)
    io.plant_negatives(preds, t, share=0.25, seed=12, poison=False)
    j = int(np.flatnonzero(~io.ignored(t))[7])
    t[j] = np.nan
    loss, grads = _focal(dev, preds, t, 6)
    _, plain = _focal(dev, preds, t, 6, ignore=False)
    assert np.isnan(loss).all() and all(g.view(U32)[j] == q.view(U32)[j] and np.isnan(g[j]) for g, q in zip(grads, plain))
    preds, t = prfocal_oracle.inputs(2051, heads=2, seed=12)
    io.plant_negatives(preds, t, share=0.25, seed=12, poison=False)
    j = int(np.flatnonzero(~io.ignored(t))[40])
    t[j] = np.nan
    got, plain = _pr(dev, preds, t), _pr(dev, preds, t, ignore=False)
    assert np.isnan(got[0]).all() and got[2] == plain[2]
    assert all(g.view(U32)[j] == q.view(U32)[j] for g, q in zip(got[1], plain[1]))


@pytest.mark.parametrize("heads", [1, 3])
def test_topk_a_nan_target_ranks_first(dev, heads):
    """the top-k kernel has comparisons of its own (the key, and the emit pass): a NaN target at a non-ignored element of
    a row that also holds ignored elements, k < P.  Its key is a NaN's bits: it ranks first, the losses are NaN, kth is
    NaN at k = 1, and every gradient is the plain call's on the sanitised inputs (the NaN target kept)."""
    for rows, pixels in ((3, 300), (2, 2051)):
        preds, t = topk_oracle.random_inputs(rows, pixels, seed=20 + heads, heads=heads)
        io.plant_negatives(preds, t, share=0.25, seed=20 + heads)
        row = rows - 1
        j = int(np.flatnonzero(~io.ignored(t[row]))[pixels // 7])
        assert io.ignored(t[row]).any()
        t[row, j] = np.nan
        for k in (1, 5, pixels // 3):
            got = _topk(dev, preds, t, k, rows)
            assert io.check_topk_nan_target(preds, t, k, 3.0, rows, *got, row, j) == [], (rows, pixels, k)
            assert np.isnan(got[2][:, row]).all() == (k == 1)
            clean = [io.sanitise(p, t)[0] for p in preds]
            plain = _topk(dev, clean, io.sanitise(preds[0], t)[1], k, rows, ignore=False)
            _equal_results((got[0], got[2]), (plain[0], plain[2]))
            _plain_bits_outside(got[1], plain[1], io.ignored(t), (rows, pixels, k))


def test_criteria_forward_backward_and_the_switch(dev):
    from unet_nested4tiny_objects_keypoints_amd import (FocalLoss_BCE_2d, PenaltyReducedFocalLoss, TopKFocalLoss_BCE_2d,
                                                        ops)
    shape = (2, 3, 5, 13)
    n = int(np.prod(shape))
    (pred,), t = loss_oracle.heads_inputs(1, n, seed=13)
    ign = io.plant_negatives([pred], t, share=0.25, seed=13, poison=False)
    td = _t(t, dev).view(shape)

    def run(crit):
        p = _t(pred, dev).view(shape).requires_grad_(True)
        value = crit(p, td)
        (2.0 * value).backward()
        return value.detach(), p.grad

    # FocalLoss_BCE_2d
    value, grad = run(FocalLoss_BCE_2d(ignore_negative=True))
    loss, grads = ops.focal_bce_heads([_t(pred, dev).view(shape)], td, 6, 3.0, ignore=True)
    assert _same_bits(value, loss[0]) and _same_bits(grad, grads[0] * 2.0)
    assert io.plus_zero(grad.cpu().numpy(), ign) == []
    off, off_grad = run(FocalLoss_BCE_2d())
    plain, plain_grad = ops.focal_bce(_t(pred, dev).view(6, 5, 13), td.view(6, 5, 13), 6, 3.0)
    assert _same_bits(off, plain) and _same_bits(off_grad.view(6, 5, 13), plain_grad * 2.0)
    # TopKFocalLoss_BCE_2d
    crit = TopKFocalLoss_BCE_2d(k=9, ignore_negative=True)
    value, grad = run(crit)
    loss, grads, kth = ops.topk_focal_heads([_t(pred, dev).view(shape)], td, 9, 6, 3.0, ignore=True)
    assert _same_bits(value, loss[0]) and _same_bits(grad, grads[0] * 2.0) and _same_bits(crit.last_threshold, kth[0])
    off, off_grad = run(TopKFocalLoss_BCE_2d(k=9))
    loss, grads, _ = ops.topk_focal_heads([_t(pred, dev).view(shape)], td, 9, 6, 3.0)
    assert _same_bits(off, loss[0]) and _same_bits(off_grad, grads[0] * 2.0)
    # PenaltyReducedFocalLoss
    (pp,), pt = prfocal_oracle.inputs(n, seed=13)
    ign = io.plant_negatives([pp], pt, share=0.25, seed=14, poison=False)
    pred, td = pp, _t(pt, dev).view(shape)
    crit = PenaltyReducedFocalLoss(ignore_negative=True)
    value, grad = run(crit)
    loss, grads, n_pos = ops.pr_focal_heads([_t(pp, dev).view(shape)], td, 2.0, 4.0, 1e-4, 1.0, ignore=True)
    assert _same_bits(value, loss[0]) and _same_bits(grad, grads[0] * 2.0) and torch.equal(crit.last_num_positives, n_pos)
    assert io.plus_zero(grad.cpu().numpy(), ign) == []
    off, off_grad = run(PenaltyReducedFocalLoss())
    loss, grads, _ = ops.pr_focal_heads([_t(pp, dev).view(shape)], td, 2.0, 4.0, 1e-4, 1.0)
    assert _same_bits(off, loss[0]) and _same_bits(off_grad, grads[0] * 2.0)


# (3) -----------------------------------------------------------------------------------------------------------------
def _criteria():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, PenaltyReducedFocalLoss, TopKFocalLoss_BCE_2d
    return {"focal": lambda: FocalLoss_BCE_2d(ignore_negative=True),
            "topk": lambda: TopKFocalLoss_BCE_2d(fraction=0.1, ignore_negative=True),
            "prfocal": lambda: PenaltyReducedFocalLoss(ignore_negative=True)}


def _net(dev):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(81)
    m = UNet_Nested(in_channels=1, n_classes=2, feature_scale=8, depth=3).to(dev).train()
    m.drop_out.p = 0.0
    return m


def _batch(g, dev):
    x = torch.randn(2, 1, 32, 32, generator=g)
    t = torch.rand(2, 2, 32, 32, generator=g)
    t[torch.rand(t.shape, generator=g) < 0.01] = 1.0
    t[:, :, 4:12, 20:30] = -1.0                                   # an ignore rectangle, every class
    t[1, 1, 20:, :6] = -1.0                                       # and one of a single class
    return x.to(dev), t.to(dev)


def _formula(name, out, target):
    """the criterion's CPU formula restated in float64 torch on one head"""
    o, t = out.double(), target.double()
    ign = t < 0
    if name == "prfocal":
        lo = float(F32(1e-4))
        q = o.clamp(lo, float(F32(1.0) - F32(1e-4)))
        pos = t >= 1.0
        term = torch.where(pos, -(1 - q) ** 2 * torch.log(q), -(1 - torch.where(ign, torch.zeros_like(t), t)) ** 4 * q ** 2
                           * torch.log1p(-q))
        return torch.where(ign, torch.zeros_like(term), term).sum() / pos.sum().clamp(min=1)
    d = torch.where(ign, torch.zeros_like(o), o - t)
    err = 1 - d.abs() + 1e-20
    term = torch.where(ign, torch.zeros_like(d), -(1 - err) ** 3 * torch.log(err))
    rows = t.shape[0] * t.shape[1]
    if name == "topk":
        flat, key = term.reshape(rows, -1), d.abs().reshape(rows, -1)
        k = int(np.ceil(0.1 * flat.shape[1]))
        idx = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :k]
        return torch.gather(flat, 1, idx).sum() / rows
    return term.sum() / rows


@pytest.mark.parametrize("name", ["focal", "topk", "prfocal"])
def test_train_step_equals_the_written_out_loop(dev, monkeypatch, name):
    """the fused step against the loop over heads (criterion(o, target) per head, their mean, autograd): the same bits,
    as tests/test_gpu_prfocal.py holds that wiring to; and the loss against the formula over the non-ignored elements
    in float64, to float32 summation accuracy"""
    from unet_nested4tiny_objects_keypoints_amd import step, train_step
    model = _net(dev)
    twin = copy.deepcopy(model)
    x, target = _batch(torch.Generator().manual_seed(82), dev)
    crit, crit2 = _criteria()[name](), _criteria()[name]()
    opt, opt2 = torch.optim.SGD(model.parameters(), lr=0.05), torch.optim.SGD(twin.parameters(), lr=0.05)
    assert step._FUSED_HEAD_LOSS
    outs, loss = train_step(model, opt, crit, x, target)
    assert isinstance(outs, tuple) and len(outs) >= 2
    monkeypatch.setattr(step, "_FUSED_HEAD_LOSS", False)
    _, loss2 = train_step(twin, opt2, crit2, x, target)
    assert _same_bits(loss.detach(), loss2.detach())
    for (n, p), q in zip(model.named_parameters(), twin.parameters()):
        assert _same_bits(p.grad, q.grad) and _same_bits(p, q), n
    want = sum(_formula(name, o.detach(), target) for o in outs) / len(outs)
    # float32 terms of at most 17 roundings each (1e-6, tests/loss_oracle.py EPS and tests/prfocal_oracle.py rel_units)
    # on a summation path of about 32 float32 additions (1.9e-6), then the mean over heads
    assert abs(float(loss.detach()) - float(want)) <= 4e-6 * abs(float(want)), (float(loss.detach()), float(want))


@pytest.mark.parametrize("name", ["focal", "topk", "prfocal"])
def test_graphed_train_step_is_the_eager_step(dev, name):
    from unet_nested4tiny_objects_keypoints_amd import GraphedTrainStep, train_step
    a = _net(dev)
    b = copy.deepcopy(a)
    crit_a, crit_b = _criteria()[name](), _criteria()[name]()
    oa = torch.optim.SGD(a.parameters(), lr=2e-3, momentum=0.9)
    ob = torch.optim.SGD(b.parameters(), lr=2e-3, momentum=0.9)
    g = torch.Generator().manual_seed(83)
    batches = [_batch(g, dev) for _ in range(3)]
    batches[1][1][0, 0, 12:20, :] = -1.0                           # the ignored set changes between replays
    graphed = GraphedTrainStep(a, oa, crit_a, batches[0][0], batches[0][1], capture_optimizer=True)
    for x, t in batches:
        _, loss_g = graphed(x, t)
        _, loss_e = train_step(b, ob, crit_b, x, t)
        assert _same_bits(loss_g.detach().reshape(()), loss_e.detach().reshape(()))
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert _same_bits(p, q) and _same_bits(p.grad, q.grad), k


def _scene():
    S, H, W, per = 2, 80, 96, 9
    rng = np.random.default_rng(18)
    frames = rng.integers(0, 255, size=(S, H, W, 1), dtype=np.uint8)
    labels = np.zeros((S, per, 2), dtype=F32)
    classes = np.zeros((S, per), dtype=I32)
    for s in range(S):
        flat = rng.choice(H * W, per, replace=False)
        labels[s, :, 0], labels[s, :, 1] = flat % W, flat // W
        classes[s] = rng.integers(0, 2, per)
    labels[0, 0], classes[0, 0] = (30, 20), 0                      # a label inside rectangle 0 of frame 0
    rects = np.asarray([[[24, 14, 40, 28], [60, 50, 95, 79], [5, 5, 4, 4]],
                        [[0, 0, 20, 30], [50.5, 10.5, 70.5, 30.5], [10, 60, 30, 70]]], dtype=F32)
    rcls = np.asarray([[-1, 1, -1], [0, -1, 7]], dtype=I32)
    return frames, labels, classes, rects, rcls


def test_scene_crops_mark_their_targets(dev):
    """two 96 x 80 frames under 88 x 88 windows (a centred pad in y, flips and quarter turns): the target is the oracle's
    mark over the target of the same seed without ignore"""
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions, SceneCrops
    frames, labels, classes, rects, rcls = _scene()
    size = (88, 88)

    def make(**kw):
        return SceneCrops(_t(frames, dev), _t(labels, dev), _t(classes, dev), n_classes=2, crop=size, p_object=0.6,
                          jitter=(20, 20), radius=3.0, seed=5, **kw)

    plain = make()
    base = [v.cpu().numpy() for v in plain.batch(4)]
    for kw in (dict(ignore=IgnoreRegions(rects, rcls), ignore_outside=True), dict(ignore=IgnoreRegions(rects, rcls).to(dev)),
               dict(ignore_outside=True)):
        crops = make(**kw)
        got = [v.cpu().numpy() for v in crops.batch(4)]
        rows, index, origin = (v.cpu().numpy() for v in crops.last)
        for a, b in ((got[0], base[0]), (got[2], base[2]), (got[3], base[3])):      # inputs, points, inside: untouched
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        with_rects = "ignore" in kw
        mask = io.mark_mask(rects if with_rects else rects[:, :0], rcls if with_rects else rcls[:, :0], index, rows, 2, size,
                            (80, 96), kw.get("ignore_outside", False))
        assert np.array_equal(got[1].view(I32), io.apply_mark(base[1], mask).view(I32)), kw
        assert 0.01 < mask.mean() < 0.9
        want = co.points_target_ref(labels, classes, index, rows, 2, size, 3.0)     # oracle mark over oracle target
        keep = ~mask
        assert (got[1][mask] == -1).all() and float(ulps(got[1][keep & (want > 0)], want[keep & (want > 0)]).max()) <= 1.0
        assert np.array_equal(got[1][keep & (want == 0)], want[keep & (want == 0)])
    with pytest.raises(ValueError):
        make(ignore=IgnoreRegions(rects[:1], rcls[:1]))
    with pytest.raises(TypeError):
        make(ignore=rects)


def test_evaluate_drops_what_lies_in_a_region(dev):
    """create_heatmap-style blobs: two labelled objects detected, one blob without a label and one label without a blob
    both inside an ignore rectangle, one blob without a label outside every rectangle"""
    from unet_nested4tiny_objects_keypoints_amd import (IgnoreRegions, PeakDetector, evaluate, false_positive_centres)
    H = W = 64
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)

    def blob(cx, cy):
        return np.exp(-0.5 * np.sqrt((xs - cx) ** 2 + (ys - cy) ** 2) / 3.0)

    maps = np.zeros((1, 2, H, W), dtype=F32)
    maps[0, 0] = np.maximum.reduce([blob(10, 12), blob(40, 44), blob(50, 10)]).astype(F32)     # (50, 10): in the rectangle
    maps[0, 1] = np.maximum.reduce([blob(20, 50), blob(8, 30)]).astype(F32)                     # (8, 30): a false positive
    labels = np.asarray([[[10, 12], [40, 44], [20, 50], [55, 15], [-1, -1]]], dtype=F32)      # (55, 15): in the rectangle
    classes = np.asarray([[0, 0, 1, 0, -1]], dtype=I32)
    ign = IgnoreRegions(np.asarray([[[44, 4, 60, 20], [0, 24, 16, 36]]], dtype=F32), [0, 0])   # the second: class 0 only
    dets = PeakDetector(threshold=0.5, radius=2)(_t(maps, dev))
    plain = evaluate(dets, _t(labels, dev), _t(classes, dev), 3.0)
    assert (int(plain.tp_total), int(plain.fp_total), int(plain.fn_total)) == (3, 2, 1) and plain.served is not None
    assert float(plain.average_precision) < 1.0
    f, p = false_positive_centres(dets, plain)
    assert sorted(map(tuple, p.cpu().round().tolist())) == [(8.0, 30.0), (50.0, 10.0)]
    score = evaluate(dets, _t(labels, dev), _t(classes, dev), 3.0, ignore=ign)
    assert (int(score.tp_total), int(score.fp_total), int(score.fn_total)) == (3, 1, 0)
    assert score.tp.tolist() == [[2, 1]] and score.fp.tolist() == [[0, 1]] and score.fn.tolist() == [[0, 0]]
    assert int(score.served.sum()) == int(plain.served.sum()) - 1 and int(score.label_pred[0, 3]) == -1
    f, p = false_positive_centres(dets, score)
    assert f.tolist() == [0] and p.cpu().round().tolist() == [[8.0, 30.0]]       # nothing from the rectangle
    # with the class-1 false positive ignored as well, nothing is wrong: AP = 1
    both = IgnoreRegions(np.asarray([[[44, 4, 60, 20], [0, 24, 16, 36]]], dtype=F32), [0, -1])
    clean = evaluate(dets, _t(labels, dev), _t(classes, dev), 3.0, ignore=both)
    assert (int(clean.tp_total), int(clean.fp_total), int(clean.fn_total)) == (3, 0, 0)
    assert float(clean.average_precision) == 1.0 and float(clean.f1) == 1.0
    assert len(false_positive_centres(dets, clean)[0]) == 0
