"""Ignore regions on the CPU: ``IgnoreRegions.contains``, the scoring arithmetic with a served set, the mark oracle
against an exact construction, the CPU formulas of the three criteria, the refusals of unetpp_target_ignore, and every
planted mutation of tests/ignore_oracle.py caught by the checks the GPU tests apply."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ignore_oracle as io
from tests import loss_oracle, prfocal_oracle, topk_oracle

F32 = np.float32
NAN = float("nan")


# ---- contains -------------------------------------------------------------------------------------------------------
RECTS = np.asarray([[[2, 3, 6, 5], [10, 10, 10, 10], [8, 1, 7, 9], [NAN, 0, 50, 50], [20, 20, 24, 22], [0, 0, 99, 99]],
                    [[0, 0, 4, 4], [5, 5, 4, 9], [30, 30, 31, 31], [-5, -5, -1, -1], [0, 0, 0, 0], [0, 0, 0, 0]]], dtype=F32)
RCLS = np.asarray([[-1, -1, -1, -1, 1, 7], [0, -1, -2, -1, -3, -4]], dtype=np.int32)


def _regions():
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions
    return IgnoreRegions(torch.from_numpy(RECTS), torch.from_numpy(RCLS))


def test_contains_edges_pixels_padding_classes_nan():
    ign = _regions()
    pts = np.asarray([[2, 3], [6, 5], [1.5, 3], [6.5, 5], [2, 2.5], [6, 5.5], [4, 4],          # edges of rectangle 0
                      [10, 10], [10.5, 10], [9.5, 10], [10, 9.5],                               # a single pixel
                      [7.5, 5], [30, 30], [NAN, 4], [4, NAN],                                   # padding rows, NaN points
                      [22, 21], [20, 20], [24.5, 21]], dtype=F32)                               # a class-1 rectangle
    for cls in (0, 1, 2):
        got = ign.contains(0, cls, torch.from_numpy(pts)).numpy()
        want = io.contains(RECTS, RCLS, 0, cls, pts)
        assert np.array_equal(got, want), cls
        assert got[:7].tolist() == [True, True, False, False, False, False, True]
        assert got[7:11].tolist() == [True, False, False, False]
        assert not got[11:15].any()                        # x1 < x0, a NaN corner, NaN points; class 7 only matches 7
        assert got[15:].tolist() == [cls == 1, cls == 1, False]
    assert bool(ign.contains(0, 7, torch.tensor([50.0, 50.0])))          # (contains does not know C)
    # frame 1: class 0 against class -1 against padding classes; a frame outside [0, S) holds nothing
    p1 = torch.tensor([[2.0, 2.0], [30.0, 30.0], [-3.0, -3.0], [0.0, 0.0]])
    assert ign.contains(1, 0, p1).tolist() == [True, False, True, True]
    assert ign.contains(1, 1, p1).tolist() == [False, False, True, False]
    assert ign.contains(1, -2, p1).tolist() == [False, False, True, False]
    assert not ign.contains(2, 0, p1).any() and not ign.contains(-1, 0, p1).any()
    # broadcasting: frame [S, 1, 1], class [1, C, 1], xy [S, C, K, 2]
    xy = torch.rand(2, 3, 5, 2, generator=torch.Generator().manual_seed(1)) * 12
    got = ign.contains(torch.arange(2).view(2, 1, 1), torch.arange(3).view(1, 3, 1), xy).numpy()
    want = io.contains(RECTS, RCLS, np.arange(2).reshape(2, 1, 1), np.arange(3).reshape(1, 3, 1), xy.numpy())
    assert got.shape == (2, 3, 5) and np.array_equal(got, want) and got.any() and not got.all()


def test_regions_shapes_and_defaults():
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions
    ign = IgnoreRegions(np.zeros((3, 0, 4), dtype=F32))
    assert len(ign) == 3 and tuple(ign.rect_class.shape) == (3, 0)
    assert not ign.contains(0, 0, torch.zeros(4, 2)).any()
    one = IgnoreRegions([[[0, 0, 1, 1]], [[5, 5, 6, 6]]], rect_class=[2])         # [R] applies to every frame
    assert one.rect_class.tolist() == [[2], [2]] and one.rect_class.dtype == torch.int32
    assert IgnoreRegions([[[0, 0, 1, 1]]]).rect_class.tolist() == [[-1]]
    for bad in (np.zeros((2, 4)), np.zeros((2, 3, 5))):
        with pytest.raises(ValueError):
            IgnoreRegions(bad)
    with pytest.raises(ValueError):
        IgnoreRegions(np.zeros((2, 3, 4)), rect_class=np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        IgnoreRegions(np.zeros((2, 3, 4)), rect_class=np.zeros(3))                # floating point classes


# ---- scoring arithmetic ---------------------------------------------------------------------------------------------
def test_false_positive_centres_uses_the_served_set():
    from unet_nested4tiny_objects_keypoints_amd import false_positive_centres
    from unet_nested4tiny_objects_keypoints_amd.detect import DetectionScore, Detections
    xy = torch.arange(2 * 2 * 4 * 2, dtype=torch.float32).view(2, 2, 4, 2)
    score = torch.tensor([[[0.9, 0.8, 0.7, 0.6], [0.9, 0.5, 0.4, 0.3]], [[0.9, 0.8, 0.2, 0.1], [0.7, 0.6, 0.5, 0.4]]])
    dets = Detections(xy, score, torch.tensor([[3, 4], [2, 9]], dtype=torch.int32))
    pred_label = torch.tensor([[[0, -1, -1, -1], [-1, 1, -1, -1]], [[-1, -1, -1, -1], [2, -1, -1, 0]]], dtype=torch.int32)
    fields = [torch.zeros(())] * 15 + [pred_label, torch.zeros(2, 3, dtype=torch.int32)]
    plain = DetectionScore(*fields)
    assert plain.served is None
    f0, p0 = false_positive_centres(dets, plain)
    count_served = torch.arange(4).view(1, 1, 4) < dets.count.clamp(max=4).unsqueeze(-1)
    wrong = count_served & (pred_label == -1)
    assert f0.tolist() == wrong.nonzero()[:, 0].tolist() == [0] * 5 + [1] * 4 and torch.equal(p0, xy[wrong])
    # a served set with two of those detections dropped (as inside an ignore region)
    served = count_served.clone()
    served[0, 0, 1] = served[1, 1, 2] = False
    with_served = DetectionScore(*fields, served)
    f1, p1 = false_positive_centres(dets, with_served)
    keep = served & (pred_label == -1)
    assert f1.tolist() == [0] * 4 + [1] * 3 and torch.equal(p1, xy[keep])
    assert not any(torch.equal(r, xy[0, 0, 1]) or torch.equal(r, xy[1, 1, 2]) for r in p1)
    # min_score still narrows it
    f2, p2 = false_positive_centres(dets, with_served, min_score=0.5)
    assert torch.equal(p2, xy[keep & (score >= 0.5)]) and len(f2) == int((keep & (score >= 0.5)).sum())
    f3, _ = false_positive_centres(dets, plain, min_score=0.5)
    assert len(f3) == int((wrong & (score >= 0.5)).sum())
    with pytest.raises(ValueError):
        false_positive_centres(dets, DetectionScore(*fields, served[:, :, :3]))


# ---- the mark oracle against an exact construction ---------------------------------------------------------------------
EXT = 80     # the full mask covers EXT pixels around the frame: a rectangle may reach beyond it


def _full_mask(rects, classes, C, Hs, Ws, outside):
    """bool [C, Hs + 2 EXT, Ws + 2 EXT]: pixel (x - EXT, y - EXT) of class map c lies in a live rectangle (integer and
    half-integer edges alike: the comparison is on the pixel's whole coordinates), or, with `outside`, off the frame"""
    ys, xs = (np.mgrid[0:Hs + 2 * EXT, 0:Ws + 2 * EXT] - EXT).astype(F32)
    full = np.zeros((C, Hs + 2 * EXT, Ws + 2 * EXT), bool)
    if outside:
        full |= ~((0 <= xs) & (xs <= Ws - 1) & (0 <= ys) & (ys <= Hs - 1))[None]
    for (x0, y0, x1, y1), k in zip(rects, classes):
        with np.errstate(invalid="ignore"):
            inside = (x0 <= xs) & (xs <= x1) & (y0 <= ys) & (ys <= y1)
        if k == -1:
            full |= inside[None]
        elif 0 <= k < C:
            full[k] |= inside
    return full


EXACT = [("identity", (40, 48)), ("flip", (40, 48)), ("flip_y", (33, 70)), ("quarter", (40, 40)), ("three_quarters", (40, 40))]


@pytest.mark.parametrize("outside", [False, True])
@pytest.mark.parametrize("kind,size", EXACT, ids=[k for k, _ in EXACT])
def test_mark_oracle_equals_a_cut_of_the_full_frame_mask(kind, size, outside):
    """frames of 64 x 56 with the window overhanging the left / top, the right / bottom, or both in x: the oracle's mask is
    the full-frame mask padded with `outside` and cut by slice / rot90 / flip"""
    C, Hs, Ws = 3, 64, 56
    Ho, Wo = size
    rects = np.asarray([[[4, 6, 11, 9], [20, 30, 20, 30], [30.5, 12.5, 40.5, 20], [50, 50, 70, 70], [9, 8, 5, 20],
                         [NAN, 0, 9, 9], [0, 0, 55, 63], [14, 2, 22, 7], [0, 40, 3, 63]]], dtype=F32)
    classes = np.asarray([[-1, 1, 0, 2, -1, -1, 3, 2, -1]], dtype=np.int32)
    full = _full_mask(rects[0], classes[0], C, Hs, Ws, outside)
    assert full.any() and not full.all(axis=(1, 2)).any()
    origins = [(-7, -5), (Ws - Wo + 9, Hs - Ho + 6), (3, 11)]
    if Wo > Ws:
        origins = [(-((Wo - Ws) // 2), 10), (-((Wo - Ws) // 2), -4)]
    strict_caught = False
    for origin in origins:
        row = io.window_row(kind, origin, size).astype(F32)
        got = io.mark_mask(rects, classes, [0], row[None], C, size, (Hs, Ws), outside)[0]
        want = io.cut_window(full, kind, (origin[0] + EXT, origin[1] + EXT), size, pad_value=False)
        assert np.array_equal(got, want), (kind, origin, outside)
        assert got.any() and not got.all()
        if outside:     # mutations: the frame's edge pixels are inside; a class rectangle marks its own class only
            strict = io.mark_mask(rects, classes, [0], row[None], C, size, (Hs, Ws), True, "outside_uses_strict_bounds")[0]
            strict_caught |= not np.array_equal(strict, want)      # (a window off the frame's edge cannot tell)
        loose = io.mark_mask(rects, classes, [0], row[None], C, size, (Hs, Ws), outside, "class_filter_dropped")[0]
        assert not np.array_equal(loose, want)
    assert strict_caught == bool(outside)
    # an all-fill sample: everything with `outside`, nothing without
    row = io.window_row(kind, origins[0], size).astype(F32)
    dead = io.mark_mask(rects, classes, [-1], row[None], C, size, (Hs, Ws), outside)
    assert dead.all() if outside else not dead.any()


def test_mark_cases_hold_what_they_plant():
    """the GPU test's input sets: every planted rectangle kind is there to be seen in the oracle's mask"""
    for shape in io.MARK_SHAPES:
        N, C, Ho, Wo = shape
        case = io.mark_case(N, C, Ho, Wo, 300)
        mask = io.mark_mask(case["rects"], case["rect_class"], case["index"], case["rows"], C, (Ho, Wo), case["src_size"],
                            False)
        assert case["kinds"][0] == "identity"
        n = 0
        assert mask[n, :, 4:10, 5:13].all()                                   # 0: inside, every class
        assert mask[n, 0, 10:21, Wo - 6:].all() and not mask[n, C - 1, 12, Wo - 1] or C == 1   # 1: class 0 only
        assert mask[n, min(1, C - 1), 20, 20] and not mask[n, min(1, C - 1), 20, 21]            # 3: a single pixel
        assert not mask[n].all()                                              # 6, 7: padding classes mark nothing
        assert mask[n, :, 3:5, 31:34].all() and not mask[n, 0, 2, 31]         # 9: half-integer edges
        assert mask[n, :, Ho - 3:, 0:3].all()                                 # the last row, in the second chunk
        assert 0.005 < mask.mean() < 0.6
        if N >= 3:
            assert not mask[1].any()
        for R in (0, 1):
            small = io.mark_case(N, C, Ho, Wo, R)
            m = io.mark_mask(small["rects"], small["rect_class"], small["index"], small["rows"], C, (Ho, Wo),
                             small["src_size"], False)
            assert m.any() == (R == 1)
    oc = io.outside_case()
    on = io.mark_mask(oc["rects"], oc["rect_class"], oc["index"], oc["rows"], oc["C"], oc["out_size"], oc["src_size"], True)
    off = io.mark_mask(oc["rects"], oc["rect_class"], oc["index"], oc["rows"], oc["C"], oc["out_size"], oc["src_size"], False)
    assert on[3].all() and not off[3].any()                                   # index -1
    assert on[0, :, :, :9].all() and on[0, :, :, 39:].all() and not on[0, 1, 0, 9:39].any()   # the centred pad
    assert on[4, :, 25:].all() and off[1, 1].any() and not off[1, 0].any()
    strict = io.mark_mask(oc["rects"], oc["rect_class"], oc["index"], oc["rows"], oc["C"], oc["out_size"], oc["src_size"],
                          True, "outside_uses_strict_bounds")
    assert not np.array_equal(strict, on)


# ---- the loss oracles and the mutations -------------------------------------------------------------------------------
def _focal_inputs(n=2051, heads=2, share=0.25):
    preds, t = loss_oracle.heads_inputs(heads, n, seed=3)
    mask = io.plant_negatives(preds, t, share=share, seed=1)
    return preds, t, mask


def _topk_inputs(rows=3, pixels=300, heads=2):
    preds, t = topk_oracle.random_inputs(rows, pixels, seed=4, heads=heads)
    io.plant_negatives(preds, t, share=0.25, seed=2)
    return preds, t


def _pr_inputs(n=2051, heads=2):
    preds, t = prfocal_oracle.inputs(n, heads=heads, seed=2)
    io.plant_negatives(preds, t, share=0.25, seed=3)
    return preds, t


def test_planted_negatives_cover_the_special_values():
    preds, t, mask = _focal_inputs()
    assert 0.05 < mask.mean() < 0.5
    neg = t[mask]
    assert (neg == -1).any() and np.isneginf(neg).any() and (neg == F32(-1e-45)).any() and F32(-1e-45) < 0
    zeros = t[(t == 0) & ~mask]
    assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()            # -0.0 and +0.0, both not ignored
    assert all(np.isnan(p[mask]).any() and np.isinf(p[mask]).any() for p in preds)
    assert all(np.isfinite(p[~mask]).all() for p in preds)


def test_restatements_pass_and_every_loss_mutation_is_caught():
    caught = set()
    # FocalLoss_BCE_2d
    preds, t, mask = _focal_inputs()
    rows, gamma = 6, 3.0
    loss, grads = io.restate_focal_f32(preds, t, gamma, rows)
    assert io.check_focal(preds, t, gamma, rows, loss, grads) == []
    for m in ("ignored_term_counted", "ignored_gradient_stale", "zero_target_ignored", "negative_zero_ignored"):
        loss, grads = io.restate_focal_f32(preds, t, gamma, rows, mutation=m)
        assert io.check_focal(preds, t, gamma, rows, loss, grads), m
        caught.add(m)
    # top-k
    tp, tt = _topk_inputs()
    k, denom = 5, 3
    res = io.restate_topk_f32(tp, tt, k, gamma, denom)
    assert io.check_topk(tp, tt, k, gamma, denom, *res) == []
    for kk in (300, 280):               # k >= P, and k above the number of non-zero keys: ignored elements selected
        assert io.check_topk(tp, tt, kk, gamma, denom, *io.restate_topk_f32(tp, tt, kk, gamma, denom)) == []
    for m in ("ignored_ranked_first", "ignored_term_counted", "zero_target_ignored", "negative_zero_ignored"):
        kk = k if m == "ignored_ranked_first" else 280     # 280: every non-ignored element and some ignored ones
        res = io.restate_topk_f32(tp, tt, kk, gamma, denom, mutation=m)
        assert io.check_topk(tp, tt, kk, gamma, denom, *res), m
        caught.add(m)
    # penalty-reduced
    pp, pt = _pr_inputs()
    res = io.restate_prfocal_f32(pp, pt)
    assert io.check_prfocal(pp, pt, res) == []
    for m in ("ignored_counted_positive", "ignored_term_counted", "ignored_gradient_stale", "zero_target_ignored",
              "negative_zero_ignored"):
        res = io.restate_prfocal_f32(pp, pt, mutation=m)
        assert io.check_prfocal(pp, pt, res), m
        caught.add(m)
    # a NaN target is not ignored: the loss is NaN and so is that element's gradient, as in the plain call
    preds, t, _ = _focal_inputs(n=9)
    j = int(np.flatnonzero(~io.ignored(t))[0])
    t[j] = NAN
    loss, grads = io.restate_focal_f32(preds, t, gamma, rows)
    assert np.isnan(loss).all() and all(np.isnan(g[j]) for g in grads)
    loss, grads = io.restate_focal_f32(preds, t, gamma, rows, mutation="nan_target_ignored")
    assert not np.isnan(loss).any() and all(g[j] == 0 for g in grads)
    caught.add("nan_target_ignored")
    # the same for top-k, whose kernel has comparisons of its own: the NaN ranks first, in a row that holds ignored
    # elements as well
    for heads in (1, 3):
        tp, tt = topk_oracle.random_inputs(3, 300, seed=6, heads=heads)
        io.plant_negatives(tp, tt, share=0.25, seed=6)
        row = 1
        j = int(np.flatnonzero(~io.ignored(tt[row]))[11])
        assert io.ignored(tt[row]).any()
        tt[row, j] = NAN
        for k in (1, 5):
            res = io.restate_topk_f32(tp, tt, k, gamma, 3)
            assert io.check_topk_nan_target(tp, tt, k, gamma, 3, *res, row, j) == [], (heads, k)
            res = io.restate_topk_f32(tp, tt, k, gamma, 3, mutation="nan_target_ignored")
            assert io.check_topk_nan_target(tp, tt, k, gamma, 3, *res, row, j), (heads, k)
    # the two mutations of the mark rule are caught by test_mark_oracle_equals_a_cut_of_the_full_frame_mask, and
    # class_filter_dropped by contains as well
    pts = np.asarray([[22, 21]], dtype=F32)
    assert not io.contains(RECTS, RCLS, 0, 0, pts)[0] and io.contains(RECTS, RCLS, 0, 0, pts, "class_filter_dropped")[0]
    caught.add("class_filter_dropped")
    oc = io.outside_case()
    args = (oc["rects"], oc["rect_class"], oc["index"], oc["rows"], oc["C"], oc["out_size"], oc["src_size"], True)
    on, strict = io.mark_mask(*args), io.mark_mask(*args, "outside_uses_strict_bounds")
    assert not on[0, 1, 0, 9] and strict[0, 1, 0, 9] and not np.array_equal(on, strict)    # source pixel (0, 4): inside
    caught.add("outside_uses_strict_bounds")
    assert caught == set(io.MUTATIONS)


@pytest.mark.parametrize("n", [1, 3, 9, 2049])
def test_cpu_formulas_apply_where(n):
    """the CPU-tensor paths of the three criteria: torch.where(target < 0, 0, term), against the oracles' bounds"""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, PenaltyReducedFocalLoss, TopKFocalLoss_BCE_2d
    preds, t = loss_oracle.heads_inputs(1, n, seed=5)
    if n >= 2:
        io.plant_negatives(preds, t, share=0.3, seed=4)
    p4 = torch.from_numpy(preds[0]).view(1, 1, 1, n).requires_grad_(True)
    t4 = torch.from_numpy(t).view(1, 1, 1, n)
    loss = FocalLoss_BCE_2d(gamma=3, ignore_negative=True)(p4, t4)
    loss.backward()
    assert io.check_focal(preds, t, 3.0, 1, [loss.item(), loss.item()], [p4.grad.numpy().ravel()]) == []
    if n >= 2:
        off = FocalLoss_BCE_2d(gamma=3)(p4.detach(), t4)
        assert float(off.detach()) != float(loss.detach()) or np.isnan(float(off.detach()))
    k = max(1, n // 3)
    crit = TopKFocalLoss_BCE_2d(k=k, ignore_negative=True)
    value = crit(torch.from_numpy(preds[0]).view(1, 1, 1, n), t4)
    want, _ = io.topk_expected(preds[0].reshape(1, n), t.reshape(1, n), k, 3.0, 1)
    assert loss_oracle.loss_ratio(float(value), want.loss) <= 1.0
    assert np.array_equal(crit.last_threshold.numpy().view(np.uint32), want.kth.view(np.uint32))
    pp, pt = prfocal_oracle.inputs(n, heads=1, seed=6)
    if n >= 2:
        io.plant_negatives(pp, pt, share=0.3, seed=5)
    crit = PenaltyReducedFocalLoss(ignore_negative=True)
    pin = torch.from_numpy(pp[0]).requires_grad_(True)
    value = crit(pin, torch.from_numpy(pt))
    value.backward()
    assert io.check_prfocal(pp, pt, ([float(value.detach())] * 2, [pin.grad.numpy()], int(crit.last_num_positives))) == []
    exp, _ = io.prfocal_expected(pp[0], pt)
    assert prfocal_oracle.loss_ratio(float(value.detach()), exp.loss) <= 1.0 and int(crit.last_num_positives) == exp.n_pos


def test_defaults_are_off():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, PenaltyReducedFocalLoss, TopKFocalLoss_BCE_2d
    for crit in (FocalLoss_BCE_2d(), TopKFocalLoss_BCE_2d(k=3), PenaltyReducedFocalLoss()):
        assert crit.ignore_negative is False


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------
def test_target_ignore_refuses_bad_arguments():
    """unetpp_target_ignore returns UNETPP_EINVAL before it touches the device; R == 0 without `outside` is a no-op"""
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    lib = _lib.lib()
    for name in ("unetpp_target_ignore", "unetpp_focal_bce_heads_ignore", "unetpp_topk_focal_heads_ignore",
                 "unetpp_pr_focal_heads_ignore"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    good = dict(rects=0x1000, rect_class=0x2000, M=2, R=3, index=0x3000, N=2, params=0x4000, C=4, Ho=32, Wo=32, Hs=64,
                Ws=64, outside=1, target=0x5000)

    def call(**kw):
        a = dict(good, **kw)
        return lib.unetpp_target_ignore(a["rects"], a["rect_class"], a["M"], a["R"], a["index"], a["N"], a["params"],
                                        a["C"], a["Ho"], a["Wo"], a["Hs"], a["Ws"], a["outside"], a["target"], None)

    for bad in (dict(rects=None), dict(rect_class=None), dict(index=None), dict(params=None), dict(target=None),
                dict(M=0), dict(R=-1), dict(N=0), dict(C=0), dict(Ho=0), dict(Wo=0), dict(Hs=0), dict(Ws=-3),
                dict(C=65536), dict(Ho=(1 << 24) + 1), dict(Wo=(1 << 24) + 1), dict(Hs=(1 << 24) + 1),
                dict(Ws=(1 << 24) + 1), dict(R=0, outside=0, target=None), dict(R=0, outside=0, N=0)):
        assert call(**bad) == -1, bad
    assert call(R=0, outside=0) == 0                                  # a valid no-op: nothing is launched
    assert call(R=0, outside=0, rects=None, rect_class=None) == 0     # R == 0 needs no rectangle pointers
    # the loss twins refuse what the plain calls refuse
    hd = _lib.FocalHeads()
    hd.n_heads = 1
    hd.pred[0] = 0x1000
    assert lib.unetpp_focal_bce_heads_ignore(C.byref(hd), None, 8, 1, 3.0, 0x2000, 0x3000, None) == -1
    assert lib.unetpp_focal_bce_heads_ignore(C.byref(hd), 0x1004, 8, 1, 3.0, 0x2000, 0x3000, None) == -1    # misaligned
    assert lib.unetpp_topk_focal_heads_ignore(C.byref(hd), 0x1000, 2, 8, 0, 2, 3.0, 0x2000, 0x3000, 0x4000, None) == -1
    assert lib.unetpp_pr_focal_heads_ignore(C.byref(hd), 0x1000, 8, 2.0, 4.0, 0.7, 1.0, 0x2000, 0x3000, 0x4000, None) == -1
