"""Detection on the GPU (detect.py, csrc/detect.hip) against the numpy restatement of tests/detect_oracle.py.

(a) unetpp_peaks_detect: xy, score and count equal the oracle bit for bit -- maps whose width is no multiple of 4 or 64 and
    whose size is no multiple of a workgroup's 2048 pixels, several workgroups per map, radius 1 / 2 / 4, refinement on and
    off, blobs in the corners and on the edges, a plateau, equal maxima r and r + 1 apart, NaNs, values at the threshold;
    a map without a peak; the dense case; truncation at the capacity; 3000 peaks over 512 workgroups; a map of 2.15e9
    pixels (64-bit raster indices); two runs give the same bits.
(b) unetpp_detect_match: pred_label, label_pred and stats equal the oracle exactly.
(c) PeakDetector and evaluate end to end on the project's own target maps, and SceneInference.detect.
"""
import numpy as np
import pytest
import torch

from tests import detect_oracle as orc

pytestmark = pytest.mark.gpu

THR = 0.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def run_peaks(maps_np, thr, r, cap, refine, dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    xy, score, count = ops.peaks_detect(torch.from_numpy(maps_np).to(dev), thr, r, cap, refine)
    return xy.cpu(), score.cpu(), count.cpu()


def assert_equals_oracle(got, want):
    (xy, score, count), (wxy, wscore, wcount) = got, want
    assert count.tolist() == wcount.tolist()
    assert same_bits(score, torch.from_numpy(wscore))
    assert same_bits(xy, torch.from_numpy(wxy))


# ------------------------------------------------------------------------------------------------ (a)
def seeded_maps(M, H, W, r, seed):
    """[M, H, W]: noise below the threshold; blobs (sub-pixel centres) in the four corners, on each edge and, where the map
    is high enough, at seeded places of its lower part; a 3x2 plateau; equal single pixels r apart and r + 1 apart; a NaN
    beside a blob's peak and a lone NaN; a pixel exactly at the threshold and one an ulp below it"""
    rng = np.random.RandomState(seed)
    maps = (rng.rand(M, H, W) * 0.3).astype(np.float32)
    for m in range(M):
        a = maps[m]
        centres = [(0.2, 0.3), (W - 1.3, 0.0), (0.0, H - 1.2), (W - 1.0, H - 1.0),                   # corners
                   (W / 2 + 0.4, 0.0), (W / 2 - 3.3, H - 1.0), (0.0, H / 2 + 0.3), (W - 1.0, H / 2 - 0.4)]   # edges
        centres.append((62.3, 15.6))
        if H >= 60:
            centres += [(5 + rng.rand() * (W - 10), 30 + rng.rand() * (H - 40)) for _ in range(6)]
        for cx, cy in centres:
            np.maximum(a, orc.blob(H, W, cx, cy, radius=1.5), out=a)
        a[8:10, 20:23] = 0.8                                # plateau
        a[12, 30] = a[12, 30 + r] = 0.9                     # r apart: one peak
        a[12, 45] = a[12 + r + 1, 45 + r + 1] = 0.9         # r + 1 apart: two
        a[16, 63] = np.nan                                  # right neighbour of the blob's peak pixel (62, 16)
        a[4, 60] = np.nan
        a[20, 70] = np.float32(THR)
        a[20, 78] = np.nextafter(np.float32(THR), np.float32(0))
    return maps


SHAPES = [(3, 70, 90), (1, 24, 88), (2, 129, 257)]   # 6300 / 2112 / 33153 pixels a map: 4, 2 and 17 workgroups, all ragged


@pytest.mark.parametrize("refine", [True, False], ids=["refine", "integer"])
@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_peaks_equal_the_oracle(dev, shape, r, refine):
    M, H, W = shape
    maps = seeded_maps(M, H, W, r, seed=100 * r + H)
    cap = 64
    want = orc.peaks_detect(maps, THR, r, cap, refine)
    assert 12 <= int(want[2].min()) and int(want[2].max()) <= cap            # the structure is there and nothing truncated
    peaks0 = {(float(x), float(y)) for x, y, _ in orc.peaks_of_map(maps[0], THR, r, False)}
    assert (20.0, 8.0) in peaks0 and (21.0, 8.0) not in peaks0               # the plateau: its first pixel only
    assert (30.0, 12.0) in peaks0 and (30.0 + r, 12.0) not in peaks0         # equal, r apart
    assert (45.0, 12.0) in peaks0 and (46.0 + r, 13.0 + r) in peaks0         # equal, r + 1 apart
    assert (62.0, 16.0) in peaks0 and (70.0, 20.0) in peaks0 and (78.0, 20.0) not in peaks0   # NaN neighbour; threshold
    assert_equals_oracle(run_peaks(maps, THR, r, cap, refine, dev), want)


def test_a_map_without_a_peak_is_all_padding(dev):
    maps = np.full((3, 24, 88), 0.2, dtype=np.float32)
    maps[1, 5, 5] = 0.9
    maps[2, :, :] = np.nan
    xy, score, count = run_peaks(maps, THR, 2, 8, True, dev)
    assert count.tolist() == [0, 1, 0]
    for m in (0, 2):
        assert bool((xy[m] == -1).all()) and bool((score[m] == float("-inf")).all())
    assert_equals_oracle((xy, score, count), orc.peaks_detect(maps, THR, 2, 8, True))


@pytest.mark.parametrize("r", [1, 3])
def test_dense_map_every_pixel_takes_the_window_test(dev, r):
    rng = np.random.RandomState(7)
    maps = rng.rand(1, 70, 90).astype(np.float32)
    maps[0, 30:34, 40:50] = np.round(maps[0, 30:34, 40:50] * 4) / 4          # ties among neighbours
    cap = 2048
    want = orc.peaks_detect(maps, 0.0, r, cap, True)
    assert 50 < int(want[2][0]) <= cap
    assert_equals_oracle(run_peaks(maps, 0.0, r, cap, True, dev), want)


def test_truncation_keeps_the_first_in_raster_order(dev):
    maps = np.zeros((1, 70, 90), dtype=np.float32)
    rng = np.random.RandomState(3)
    spots = [(6 + 16 * (i // 4) + (i % 3), 8 + 20 * (i % 4)) for i in range(12)]   # (y, x), at least 16 apart
    for y, x in spots:
        maps[0, y, x] = 0.5 + 0.5 * rng.rand()
    xy, score, count = run_peaks(maps, THR, 4, 5, False, dev)
    assert count.tolist() == [12]
    assert xy[0].tolist() == [[float(x), float(y)] for y, x in sorted(spots)[:5]]
    assert_equals_oracle((xy, score, count), orc.peaks_detect(maps, THR, 4, 5, False))


def test_ranks_across_many_workgroups(dev):
    H = W = 1024                                                       # 512 workgroups of 2048 pixels
    r, n = 2, 3000
    rng = np.random.RandomState(11)
    cells = rng.choice(128 * 128, size=n, replace=False)               # 8x8 cells, spike in the cell's first 4x4:
    ys = 8 * (cells // 128) + rng.randint(0, 4, size=n)                # two spikes are at least 5 = 2r + 1 apart
    xs = 8 * (cells % 128) + rng.randint(0, 4, size=n)
    maps = np.zeros((1, H, W), dtype=np.float32)
    maps[0, ys, xs] = (0.5 + 0.5 * rng.rand(n)).astype(np.float32)
    cap = 4096
    peaks = orc.peaks_of_map(maps[0], THR, r, True, candidates=zip(ys.tolist(), xs.tolist()))
    assert len(peaks) == n
    assert_equals_oracle(run_peaks(maps, THR, r, cap, True, dev), orc.pack_peaks([peaks], cap))
    xy, score, count = run_peaks(maps, THR, r, 1000, True, dev)        # and truncated in the middle of the map
    assert_equals_oracle((xy, score, count), orc.pack_peaks([peaks], 1000))


def test_raster_indices_beyond_2_31(dev):
    side, crop, r, cap = 46400, 128, 2, 16
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip("needs 12 GB of free device memory, %.1f GB are free" % (free / 2 ** 30))
    from unet_nested4tiny_objects_keypoints_amd import ops
    maps = torch.zeros(1, side, side, device=dev)                     # 8.6 GB
    assert maps.numel() > 2 ** 31
    corner = np.zeros((crop, crop), dtype=np.float32)
    for cx, cy in ((70.3, 72.6), (100.0, 90.5), (126.2, 80.0), (90.4, 127.0), (127.0, 127.0)):   # last 64 pixels; edges
        np.maximum(corner, orc.blob(crop, crop, cx, cy, radius=1.5), out=corner)
    corner[110, 75] = corner[110, 75 + r + 1] = 0.95
    maps[0, side - crop:, side - crop:] = torch.from_numpy(corner).to(dev)
    peaks = orc.peaks_of_map(corner, THR, r, True, origin=(side - crop, side - crop))
    assert len(peaks) == 7 and all(float(x) >= side - 64 and float(y) >= side - 64 for x, y, _ in peaks)
    xy, score, count = ops.peaks_detect(maps, THR, r, cap, True)
    assert_equals_oracle((xy.cpu(), score.cpu(), count.cpu()), orc.pack_peaks([peaks], cap))
    del maps
    torch.cuda.empty_cache()


def test_two_runs_give_the_same_bits(dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    maps = torch.from_numpy(seeded_maps(2, 129, 257, 2, seed=5)).to(dev)
    a = ops.peaks_detect(maps, THR, 2, 64, True)
    b = ops.peaks_detect(maps, THR, 2, 64, True)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2].tolist() == b[2].tolist()


# ------------------------------------------------------------------------------------------------ (b)
def run_match(xy, n_pred, order, labels, cls, tol, dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = ops.detect_match(t(xy), t(n_pred), t(order), t(labels), t(cls), tol)
    return [o.cpu().numpy() for o in out]


def assert_match_equals_oracle(args, dev):
    got = run_match(*args, dev)
    want = orc.detect_match(*args)
    for g, w, name in zip(got, want, ("pred_label", "label_pred", "stats")):
        assert g.dtype == np.int32 and g.shape == w.shape and (g == w).all(), name
    return want


def random_match_case(seed, S, C, cap, L, span, tol):
    """coordinates on the half-integer grid 0, 0.5, ..., span: equal distances and d == tol^2 occur for real; classes
    interleaved with -1 padding; a random serving order per group"""
    rng = np.random.RandomState(seed)
    xy = (rng.randint(0, 2 * span + 1, size=(S, C, cap, 2)) / 2.0).astype(np.float32)
    labels = (rng.randint(0, 2 * span + 1, size=(S, L, 2)) / 2.0).astype(np.float32)
    cls = rng.randint(-1, C, size=(S, L)).astype(np.int32)
    n_pred = rng.randint(0, cap + 1, size=(S, C)).astype(np.int32)
    order = np.stack([rng.permutation(cap) for _ in range(S * C)]).reshape(S, C, cap).astype(np.int32)
    return xy, n_pred, order, labels, cls, tol


def test_match_rule_by_hand(dev):
    xy = np.array([[[[4.0, 0.0], [9.0, 9.0], [1.0, 0.0], [-1.0, -1.0]]]], dtype=np.float32)
    labels = np.array([[[0.0, 0.0], [2.0, 0.0], [5.5, 0.0], [3.0, 0.0]]], dtype=np.float32)
    cls = np.array([[0, 0, 0, -1]], dtype=np.int32)
    order = np.array([[[2, 0, 1, 3]]], dtype=np.int32)
    pl, lp, st = assert_match_equals_oracle((xy, np.array([[3]], dtype=np.int32), order, labels, cls, 2.0), dev)
    assert pl[0, 0].tolist() == [2, -1, 0, -1]      # slot 2: labels 0 and 1 equidistant, the lower index; slot 0: label 2
    assert lp[0].tolist() == [2, -1, 0, -1] and st[0, 0].tolist() == [2, 1, 1]
    # slot 0 served first takes label 1?  no: label 2 at 1.5 is nearer; then slot 2 finds labels 0 and 1 free again
    order2 = np.array([[[0, 2, 1, 3]]], dtype=np.int32)
    assert_match_equals_oracle((xy, np.array([[3]], dtype=np.int32), order2, labels, cls, 2.0), dev)
    # a prediction whose nearest label is spent takes the next one within the tolerance
    xy3 = np.array([[[[1.0, 0.0], [1.5, 0.0], [0.0, 0.0], [0.0, 0.0]]]], dtype=np.float32)
    lab3 = np.array([[[1.0, 0.0], [3.0, 0.0], [9.0, 0.0], [9.0, 9.0]]], dtype=np.float32)
    cls3 = np.array([[0, 0, 0, 0]], dtype=np.int32)
    pl, lp, st = assert_match_equals_oracle((xy3, np.array([[2]], dtype=np.int32), np.array([[[0, 1, 2, 3]]], dtype=np.int32),
                                             lab3, cls3, 2.0), dev)
    assert pl[0, 0].tolist() == [0, 1, -1, -1] and st[0, 0].tolist() == [2, 0, 2]
    # d == tolerance^2 matches, the next float32 below does not
    for tol, hit in ((1.5, True), (float(np.nextafter(np.float32(1.5), np.float32(0))), False)):
        pl, _, _ = assert_match_equals_oracle((xy3[:, :, 1:2], np.array([[1]], dtype=np.int32),
                                               np.array([[[0]]], dtype=np.int32), lab3[:, 1:2], cls3[:, 1:2], tol), dev)
        assert (pl[0, 0, 0] == 0) == hit


@pytest.mark.parametrize("case", [
    dict(seed=1, S=2, C=3, cap=20, L=30, span=10, tol=1.5),       # 2 frames x 3 classes, interleaved classes and padding
    dict(seed=2, S=1, C=1, cap=40, L=5, span=6, tol=2.0),         # more predictions than labels
    dict(seed=3, S=1, C=2, cap=5, L=40, span=6, tol=2.0),         # more labels than predictions
    dict(seed=4, S=1, C=1, cap=300, L=300, span=30, tol=1.0),     # the label loop strides more than once
    dict(seed=5, S=2, C=3, cap=64, L=700, span=40, tol=2.5),
    dict(seed=6, S=1, C=1, cap=7, L=9, span=1, tol=0.0),          # tolerance 0: exact coincidence only
], ids=lambda c: "S%d-C%d-cap%d-L%d" % (c["S"], c["C"], c["cap"], c["L"]))
def test_match_equals_the_oracle(dev, case):
    args = random_match_case(**case)
    if case["cap"] == 300:
        args[1][...] = 300                                         # all 300 predictions are served
    want = assert_match_equals_oracle(args, dev)
    assert int(want[2][..., 0].sum()) > 0


def test_match_empty_groups(dev):
    xy, n_pred, order, labels, cls, tol = random_match_case(8, S=2, C=3, cap=12, L=20, span=8, tol=2.0)
    cls[cls == 1] = -1             # class 1 has no labels at all: an empty group where it has no predictions either
    n_pred[0, 1] = 0
    n_pred[1, 1] = 6               # predictions but no labels: all false positives
    n_pred[0, 2] = 0               # labels but no predictions: all false negatives
    pl, lp, st = assert_match_equals_oracle((xy, n_pred, order, labels, cls, tol), dev)
    assert st[0, 1].tolist() == [0, 0, 0] and st[1, 1].tolist() == [0, 6, 0]
    assert st[0, 2].tolist() == [0, 0, int((cls[0] == 2).sum())] and st[0, 2, 2] > 0
    assert (pl[0, 1] == -1).all() and (lp[cls == -1] == -1).all()


# ------------------------------------------------------------------------------------------------ (c)
def test_detector_and_evaluate_on_the_projects_own_targets(dev):
    from unet_nested4tiny_objects_keypoints_amd import Heatmap, PeakDetector, classes_from_pattern, evaluate
    pattern = [[0, 3], [1, 4], [2, 5]]
    # the two blobs of a map are over 150 pixels apart: the tail of one, exp(-25), is far below half an ulp of the
    # other's values next to its peak, so each peak's neighbours are exactly symmetric and the offset is exactly 0
    targets = torch.tensor([[[20.0, 30.0], [50.0, 200.0], [120.0, 20.0], [200.0, 40.0], [220.0, 180.0], [100.0, 220.0]]])
    hm = Heatmap(pattern, 256, 256)
    maps = hm.create_heatmap(targets)
    assert tuple(maps.shape) == (1, 3, 256, 256)
    dets = PeakDetector(threshold=0.5, radius=2, max_points=32)(maps)
    assert dets.count.tolist() == [[2, 2, 2]] and not bool(dets.truncated().any())
    assert sorted(dets.tolist(0, 0)) == [(20.0, 30.0, 1.0), (200.0, 40.0, 1.0)]
    r = evaluate(dets, targets, classes_from_pattern(pattern, 6), tolerance=1.0)
    assert (int(r.tp_total), int(r.fp_total), int(r.fn_total)) == (6, 0, 0)
    assert float(r.precision) == 1.0 and float(r.recall) == 1.0 and float(r.f1) == 1.0
    assert float(r.average_precision) == 1.0 and r.class_average_precision.tolist() == [1.0, 1.0, 1.0]
    assert float(r.mean_distance) == 0.0
    assert r.label_pred.min() >= 0 and r.tp.tolist() == [[2, 2, 2]]
    # a label that is not there, a score threshold above every score
    moved = targets.clone()
    moved[0, 0] = torch.tensor([60.0, 60.0])
    r = evaluate(dets, moved, classes_from_pattern(pattern, 6), tolerance=1.0)
    assert (int(r.tp_total), int(r.fp_total), int(r.fn_total)) == (5, 1, 1)
    r = evaluate(dets, targets, classes_from_pattern(pattern, 6), tolerance=1.0, score_threshold=2.0)
    assert (int(r.tp_total), int(r.fp_total), int(r.fn_total)) == (0, 0, 6) and float(r.average_precision) == 0.0


def test_detector_sorts_by_score_and_keeps_raster_order_among_equals(dev):
    from unet_nested4tiny_objects_keypoints_amd import PeakDetector
    maps = np.zeros((1, 2, 40, 50), dtype=np.float32)
    for (y, x), v in zip(((5, 5), (5, 30), (20, 10), (30, 40)), (0.7, 0.9, 0.7, 0.95)):
        maps[0, 0, y, x] = v
    dets = PeakDetector(threshold=0.5, radius=2, refine=False, max_points=6)(torch.from_numpy(maps).to(dev))
    assert dets.count.tolist() == [[4, 0]]
    assert dets.xy[0, 0].tolist() == [[40.0, 30.0], [30.0, 5.0], [5.0, 5.0], [10.0, 20.0], [-1.0, -1.0], [-1.0, -1.0]]
    assert dets.score[0, 0, 4:].tolist() == [float("-inf")] * 2 and dets.tolist(0, 1) == []


def test_scene_detect_is_the_detector_on_the_scene_maps(dev):
    from unet_nested4tiny_objects_keypoints_amd import PeakDetector, SceneInference, UNet_Nested
    torch.manual_seed(3)
    model = UNet_Nested(in_channels=1, n_classes=4, feature_scale=8, depth=2).to(dev).eval()
    frames = torch.randint(0, 256, (2, 96, 112, 1), dtype=torch.uint8).to(dev)
    scene = SceneInference(model, tile=64)
    maps = scene(frames)
    det = PeakDetector(threshold=float(maps.median()), radius=2, max_points=512)
    a, b = scene.detect(frames, det), det(maps)
    assert int(b.count.sum()) > 0
    assert same_bits(a.xy, b.xy) and same_bits(a.score, b.score) and a.count.tolist() == b.count.tolist()
