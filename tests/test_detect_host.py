"""CPU-only checks of the detection path (detect.py, csrc/detect.hip): the two entry points refuse bad arguments without a
device; the numpy oracle (tests/detect_oracle.py) has the properties the rule promises; the arithmetic ``evaluate`` does
after the matcher (``detect.score_matches``) on hand-made match results; ``classes_from_pattern``."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import detect_oracle as orc

EINVAL = -1
P = ctypes.c_void_p(0x1000)   # a non-null pointer that is never followed: every call below is refused before a launch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib.lib()


# ------------------------------------------------------------------------------------- argument validation, no device
def peaks_call(lib, maps=P, M=1, H=8, W=8, thr=0.5, r=2, refine=1, cap=4, xy=P, score=P, count=P, ws=P):
    return lib.unetpp_peaks_detect(maps, M, H, W, thr, r, refine, cap, xy, score, count, ws, None)


@pytest.mark.parametrize("bad", [
    dict(maps=None), dict(xy=None), dict(score=None), dict(count=None), dict(ws=None),
    dict(M=0), dict(H=0), dict(W=0), dict(M=-1), dict(H=-3), dict(W=-3),
    dict(r=0), dict(r=9), dict(r=-1), dict(cap=0), dict(cap=-5), dict(thr=float("nan")),
    dict(H=1 << 24), dict(W=1 << 24), dict(M=65536),
], ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_peaks_detect_refuses_without_a_device(lib, bad):
    assert peaks_call(lib, **bad) == EINVAL


def test_peaks_workspace_bytes(lib):
    q = lib.unetpp_peaks_workspace_bytes
    assert q(1, 8, 8) > 0
    assert q(2, 70, 90) == 2 * q(1, 70, 90)
    assert q(1, 4096, 4096) >= 4096 * 4096 // 8          # one bit per pixel at the least
    assert q(1, 4096, 4096) <= 4096 * 4096 // 4          # and small beside the map (4 bytes per pixel)
    assert q(1, 46400, 46400) > 0                        # H * W beyond 2^31
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (65536, 8, 8), (1, 1 << 24, 8), (1, 8, 1 << 24)):
        assert q(*bad) == 0


def match_call(lib, xy=P, n_pred=P, order=P, S=1, C=1, cap=4, labels=P, cls=P, L=3, tol=1.0, pl=P, lp=P, stats=P):
    return lib.unetpp_detect_match(xy, n_pred, order, S, C, cap, labels, cls, L, tol, pl, lp, stats, None)


@pytest.mark.parametrize("bad", [
    dict(xy=None), dict(n_pred=None), dict(order=None), dict(labels=None), dict(cls=None), dict(pl=None), dict(lp=None),
    dict(stats=None), dict(S=0), dict(C=0), dict(cap=0), dict(L=0), dict(S=-1), dict(C=-2), dict(cap=-1), dict(L=-1),
    dict(tol=-0.5), dict(tol=float("nan")), dict(S=1 << 16, C=1 << 16),
], ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_detect_match_refuses_without_a_device(lib, bad):
    assert match_call(lib, **bad) == EINVAL


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from unet_nested4tiny_objects_keypoints_amd import PeakDetector, ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.peaks_detect(torch.zeros(1, 8, 8), 0.5, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.detect_match(torch.zeros(1, 1, 4, 2), torch.zeros(1, 1, dtype=torch.int32),
                         torch.zeros(1, 1, 4, dtype=torch.int32), torch.zeros(1, 3, 2),
                         torch.zeros(1, 3, dtype=torch.int32), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PeakDetector()(torch.zeros(1, 1, 8, 8))
    for kw in (dict(radius=0), dict(radius=9), dict(radius=2.0), dict(max_points=0), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            PeakDetector(**kw)


# ---------------------------------------------------------------------------------------------------- oracle sanity
def test_oracle_blob_at_an_integer_centre_is_reported_there():
    a = orc.blob(40, 48, 20, 17)
    for refine in (True, False):
        peaks = orc.peaks_of_map(a, 0.5, 2, refine)
        assert len(peaks) == 1
        x, y, v = peaks[0]
        assert x.dtype == np.float32 and x == np.float32(20.0) and y == np.float32(17.0) and v == np.float32(1.0)


@pytest.mark.parametrize("centre", [(20.3, 17.0), (20.5, 17.25), (20.4, 16.6), (19.8, 17.45)])
def test_oracle_refinement_halves_the_error(centre):
    cx, cy = centre
    a = orc.blob(40, 48, cx, cy)
    (rx, ry, _), = orc.peaks_of_map(a, 0.5, 2, True)
    (ix, iy, _), = orc.peaks_of_map(a, 0.5, 2, False)
    refined = math.hypot(float(rx) - cx, float(ry) - cy)
    integer = math.hypot(float(ix) - cx, float(iy) - cy)
    print("centre %s: refined %.3f px, integer %.3f px" % (centre, refined, integer))
    assert refined <= 0.5 * integer
    assert abs(float(rx) - float(ix)) <= 0.5 and abs(float(ry) - float(iy)) <= 0.5


def test_oracle_plateau_gives_one_peak_at_its_first_pixel():
    a = np.zeros((12, 14), dtype=np.float32)
    a[4:6, 5:8] = 0.8                                     # 3 wide, 2 high
    for r in (1, 2, 4):
        assert orc.peaks_of_map(a, 0.5, r, False) == [(np.float32(5.0), np.float32(4.0), np.float32(0.8))]
        # The parabola rule as stated, at the first pixel of an interior plateau: a = 0, b = c = 0.8 on both axes, so
        # den = a - b < 0 and the offset is 0.5 (a - c) / (a - b) = +0.5 exactly: half a pixel INTO the plateau, never
        # out of it.  The offset is 0 only where the rule says so: refine off, den >= 0, or a neighbour beyond the edge.
        assert orc.peaks_of_map(a, 0.5, r, True) == [(np.float32(5.5), np.float32(4.5), np.float32(0.8))]
    b = np.zeros((12, 14), dtype=np.float32)
    b[0:2, 0:3] = 0.8                                     # the same plateau in the map's corner: no left / upper neighbour
    c = np.full((2, 3), 0.8, dtype=np.float32)            # a map that is one plateau
    for r in (1, 2, 4):
        assert orc.peaks_of_map(b, 0.5, r, True) == [(np.float32(0.0), np.float32(0.0), np.float32(0.8))]
        assert orc.peaks_of_map(c, 0.5, r, True) == [(np.float32(0.0), np.float32(0.0), np.float32(0.8))]


@pytest.mark.parametrize("r", [1, 2, 4, 8])
def test_oracle_equal_maxima_at_r_and_r_plus_one(r):
    a = np.zeros((30, 40), dtype=np.float32)
    a[10, 5] = a[10, 5 + r] = 0.9                         # Chebyshev distance r: the later one is beaten
    assert [(float(x), float(y)) for x, y, _ in orc.peaks_of_map(a, 0.5, r, False)] == [(5.0, 10.0)]
    b = np.zeros((30, 40), dtype=np.float32)
    b[10, 5] = b[10 + r + 1, 5 + r + 1] = 0.9             # r + 1 on both axes: two peaks
    assert [(float(x), float(y)) for x, y, _ in orc.peaks_of_map(b, 0.5, r, False)] == [(5.0, 10.0), (6.0 + r, 11.0 + r)]


def test_oracle_nan_is_neither_peak_nor_winner():
    a = np.zeros((10, 10), dtype=np.float32)
    a[4, 4] = 0.7
    a[4, 5] = np.nan                                      # beside the peak: does not beat it
    a[8, 8] = np.nan                                      # alone: is no peak
    peaks = orc.peaks_of_map(a, 0.5, 2, True)
    assert len(peaks) == 1
    x, y, v = peaks[0]
    assert (float(x), float(y), v) == (4.0, 4.0, np.float32(0.7))    # den is NaN along x: offset 0
    assert orc.peaks_of_map(np.full((5, 5), np.nan, dtype=np.float32), -np.inf, 1) == []


def test_oracle_values_at_the_threshold_and_capacity():
    a = np.zeros((1, 9, 30), dtype=np.float32)
    a[0, 4, 3], a[0, 4, 12], a[0, 4, 21] = 0.5, np.nextafter(np.float32(0.5), np.float32(0)), 0.75
    xy, score, count = orc.peaks_detect(a, 0.5, 2, cap=1, refine=False)
    assert count.tolist() == [2] and xy[0].tolist() == [[3.0, 4.0]] and score[0].tolist() == [0.5]
    xy, score, count = orc.peaks_detect(a, 0.5, 2, cap=4, refine=False)
    assert xy[0].tolist() == [[3.0, 4.0], [21.0, 4.0], [-1.0, -1.0], [-1.0, -1.0]]
    assert score[0, 2:].tolist() == [-np.inf, -np.inf]


def test_oracle_matcher_rule():
    # one group; predictions served in the order 2, 0, 1.  Labels 0 and 1 are equidistant from prediction 2: label 0.
    xy = np.array([[[[4.0, 0.0], [9.0, 9.0], [1.0, 0.0], [-1.0, -1.0]]]], dtype=np.float32)
    labels = np.array([[[0.0, 0.0], [2.0, 0.0], [5.5, 0.0], [3.0, 0.0]]], dtype=np.float32)
    cls = np.array([[0, 0, 0, -1]], dtype=np.int32)       # label 3 is padding although it is the nearest to slot 0
    order = np.array([[[2, 0, 1, 3]]], dtype=np.int32)
    pl, lp, st = orc.detect_match(xy, np.array([[3]], dtype=np.int32), order, labels, cls, 2.0)
    # slot 2 -> label 0 (tie with 1, lower index); slot 0 -> label 2 at 1.5 (label 1 at 2.0 is farther); slot 1: none
    assert pl[0, 0].tolist() == [2, -1, 0, -1] and lp[0].tolist() == [2, -1, 0, -1] and st[0, 0].tolist() == [2, 1, 1]
    # d == tolerance^2 is a match; the next smaller float32 tolerance is not
    pl, _, st = orc.detect_match(xy[:, :, :1], np.array([[1]], dtype=np.int32), order[:, :, :1] * 0, labels[:, 1:2],
                                 cls[:, 1:2], 2.0)
    assert pl[0, 0].tolist() == [0] and st[0, 0].tolist() == [1, 0, 0]
    pl, _, st = orc.detect_match(xy[:, :, :1], np.array([[1]], dtype=np.int32), order[:, :, :1] * 0, labels[:, 1:2],
                                 cls[:, 1:2], float(np.nextafter(np.float32(2.0), np.float32(0))))
    assert pl[0, 0].tolist() == [-1] and st[0, 0].tolist() == [0, 1, 1]


# --------------------------------------------------------------------------- the arithmetic after the matcher (CPU torch)
def hand_made(seed, S=2, C=3, cap=7, L=9):
    """random but consistent match results: every hit names a distinct label of its own (frame, class)"""
    rng = np.random.RandomState(seed)
    xy = rng.randint(0, 40, size=(S, C, cap, 2)).astype(np.float32)
    score = np.round(rng.rand(S, C, cap), 1).astype(np.float32)          # one decimal: equal scores occur
    n = rng.randint(0, cap + 1, size=(S, C))
    served = np.arange(cap)[None, None, :] < n[..., None]
    cls = rng.randint(-1, C, size=(S, L)).astype(np.int32)
    labels = rng.randint(0, 40, size=(S, L, 2)).astype(np.float32)
    pred_label = np.full((S, C, cap), -1, dtype=np.int32)
    label_pred = np.full((S, L), -1, dtype=np.int32)
    stats = np.zeros((S, C, 3), dtype=np.int32)
    for s in range(S):
        for c in range(C):
            free = [l for l in range(L) if cls[s, l] == c]
            n_lab = len(free)
            for k in range(n[s, c]):
                if free and rng.rand() < 0.6:
                    l = free.pop(rng.randint(len(free)))
                    pred_label[s, c, k], label_pred[s, l] = l, k
            tp = int((pred_label[s, c] >= 0).sum())
            stats[s, c] = (tp, n[s, c] - tp, n_lab - tp)
    return xy, score, served, pred_label, label_pred, stats, labels, cls


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_score_matches_against_the_oracle(seed):
    from unet_nested4tiny_objects_keypoints_amd.detect import score_matches
    arrays = hand_made(seed)
    xy, score, served, pred_label, label_pred, stats, labels, cls = arrays
    r = score_matches(*(torch.from_numpy(a) for a in arrays))
    S, C, cap = score.shape
    tp, fp, fn = (int(stats[..., i].sum()) for i in range(3))
    assert (int(r.tp_total), int(r.fp_total), int(r.fn_total)) == (tp, fp, fn)
    assert r.tp.tolist() == stats[..., 0].tolist() and r.fn.tolist() == stats[..., 2].tolist()
    div = lambda a, b: a / b if b else 0.0
    assert r.precision.dtype == torch.float64
    assert float(r.precision) == div(tp, tp + fp) and float(r.recall) == div(tp, tp + fn)
    assert float(r.f1) == div(2 * tp, 2 * tp + fp + fn)
    hit = pred_label >= 0
    for c in range(C):
        t, p, n = (int(stats[:, c, i].sum()) for i in range(3))
        assert float(r.class_precision[c]) == div(t, t + p) and float(r.class_recall[c]) == div(t, t + n)
        assert float(r.class_f1[c]) == div(2 * t, 2 * t + p + n)
        want = orc.average_precision(score[:, c].reshape(-1), served[:, c].reshape(-1), hit[:, c].reshape(-1), t + n)
        assert abs(float(r.class_average_precision[c]) - want) <= 1e-12
    want = orc.average_precision(score.reshape(-1), served.reshape(-1), hit.reshape(-1), tp + fn)
    assert abs(float(r.average_precision) - want) <= 1e-12
    dist = [math.hypot(float(xy[s, cls[s, l], label_pred[s, l], 0] - labels[s, l, 0]),
                       float(xy[s, cls[s, l], label_pred[s, l], 1] - labels[s, l, 1]))
            for s in range(S) for l in range(labels.shape[1]) if label_pred[s, l] >= 0]
    assert abs(float(r.mean_distance) - sum(dist) / len(dist)) <= 1e-12


def test_score_matches_zero_over_zero():
    from unet_nested4tiny_objects_keypoints_amd.detect import score_matches
    S, C, cap, L = 1, 2, 3, 2
    r = score_matches(torch.zeros(S, C, cap, 2), torch.full((S, C, cap), float("-inf")),
                      torch.zeros(S, C, cap, dtype=torch.bool), torch.full((S, C, cap), -1, dtype=torch.int32),
                      torch.full((S, L), -1, dtype=torch.int32), torch.zeros(S, C, 3, dtype=torch.int32),
                      torch.full((S, L, 2), -1.0), torch.full((S, L), -1, dtype=torch.int32))
    assert float(r.precision) == 0.0 and float(r.recall) == 0.0 and float(r.f1) == 0.0
    assert float(r.average_precision) == 0.0 and r.class_average_precision.tolist() == [0.0, 0.0]
    assert math.isnan(float(r.mean_distance))


def test_average_precision_by_hand():
    # scores 0.9 hit, 0.8 miss, 0.7 hit, 0.6 miss; 3 labels: precisions 1, 1/2, 2/3, 1/2 -> envelope 1, 2/3, 2/3, 1/2
    want = (1.0 + 2.0 / 3.0) / 3.0
    score = np.array([0.6, 0.9, 0.7, 0.8, 0.99], dtype=np.float32)
    served = np.array([1, 1, 1, 1, 0], dtype=bool)
    hit = np.array([0, 1, 1, 0, 1], dtype=bool)
    assert abs(orc.average_precision(score, served, hit, 3) - want) <= 1e-15
    from unet_nested4tiny_objects_keypoints_amd.detect import _average_precision
    got = _average_precision(torch.from_numpy(score), torch.from_numpy(served), torch.from_numpy(hit), torch.tensor(3))
    assert abs(float(got) - want) <= 1e-12


def test_classes_from_pattern():
    from unet_nested4tiny_objects_keypoints_amd import classes_from_pattern
    row = classes_from_pattern([[0, 3], [2], [5, 1]], 7)
    assert row.dtype == torch.int32 and row.tolist() == [0, 2, 1, 0, -1, 2, -1]
    with pytest.raises(ValueError):
        classes_from_pattern([[0, 7]], 7)
    with pytest.raises(ValueError):
        classes_from_pattern([[0, 1], [1]], 7)
