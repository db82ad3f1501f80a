"""csrc/keypoints.hip against oracle/keypoints_oracle.py on the shape corpus of tests/keypoints_corpus.py (-m gpu): holes
that only the watershed's level-255 phase reaches, maps whose host-driven loops run past their first batches, the
smallest legal shapes, both paths of the selection kernel at their boundary with tied peaks.  Everything is integers or
bit patterns: distances, label maps (as partitions), points, their order and the counts are compared EXACTLY, and every
device call is made twice and must give the same bits."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from oracle.keypoints_oracle import _extract_once, chamfer_distance, region_mask, transfer_points, watershed_regions
from tests import keypoints_corpus as corpus
from tests.test_keypoints import _same_partition

pytestmark = pytest.mark.gpu
SEGMENTATIONS = ("watershed", "components")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _oracle_points(heat, num, thr, segmentation):
    """oracle.extract_points with the number of regions found beside the points (retry at 0.9 * threshold included)"""
    points, count = _extract_once(heat, num, thr, segmentation)
    if count == 0:
        points, count = _extract_once(heat, num, thr * 0.9, segmentation)
    return points, count


def _regions_twice(ops, t, thr, segmentation):
    labels, dist = ops.keypoints_regions(t, thr, segmentation=segmentation)
    again, dist2 = ops.keypoints_regions(t, thr, segmentation=segmentation)
    assert torch.equal(labels, again) and torch.equal(dist, dist2)
    return labels.cpu().numpy(), dist.cpu().numpy()


def _extract_twice(ops, t, num, thr, segmentation, **kw):
    points, counts = ops.keypoints_extract(t, num, thr, segmentation=segmentation, **kw)
    again, counts2 = ops.keypoints_extract(t, num, thr, segmentation=segmentation, **kw)
    assert torch.equal(points.view(torch.int32), again.view(torch.int32)) and torch.equal(counts, counts2)
    return points.cpu().numpy(), counts.cpu().numpy()


def _check_points(points, count, want, want_count, num, where):
    assert int(count) == want_count, (where, int(count), want_count)
    assert [[int(x), int(y)] for x, y in points[:len(want)]] == want, where
    assert len(want) == min(want_count, num) and (points[len(want):] == -1).all(), where


def _check_batch(dev, names, heats, thr, num=5):
    """one device call per step for the whole batch [maps, H, W]: chamfer distance, both partitions, points and counts"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    t = torch.from_numpy(heats).to(dev)
    masks = [region_mask(h, thr) for h in heats]
    labels, dist = _regions_twice(ops, t, thr, "watershed")
    comp, zero = _regions_twice(ops, t, thr, "components")
    assert not zero.any()
    for m, name in enumerate(names):
        np.testing.assert_array_equal(dist[m], chamfer_distance(masks[m]), err_msg=name)
        want, present = watershed_regions(masks[m])
        _same_partition(labels[m], want, present)
        cl, cc = ndimage.label(masks[m], structure=np.ones((3, 3), dtype=int))
        _same_partition(comp[m], cl, list(range(1, cc + 1)))
    for seg in SEGMENTATIONS:
        points, counts = _extract_twice(ops, t, num, thr, seg)
        for m, name in enumerate(names):
            want, want_count = _oracle_points(heats[m], num, thr, seg)
            _check_points(points[m], counts[m], want, want_count, num, (name, seg))


@pytest.mark.parametrize("shape", corpus.BUCKETS)
def test_random_blobs_with_holes(dev, shape):
    names, heats = corpus.random_batches()[shape]
    assert len(names) >= 10
    _check_batch(dev, names, heats, corpus.THRESHOLD)


def test_hole_cases(dev):
    for name, heat, thr in corpus.hole_cases():
        _check_batch(dev, [name], heat[None], thr)


@pytest.mark.parametrize("shape", corpus.DEGENERATE_SHAPES)
def test_degenerate_shapes(dev, shape):
    """H * W < 256 is one partial workgroup; below 3x3 the frame is everything: no watershed region, while the mask's
    components still give theirs"""
    cases = [c for c in corpus.degenerate_cases() if c[1].shape == shape]
    assert [c[0].split()[-1] for c in cases] == ["full", "zero", "random"]
    heats = np.stack([c[1] for c in cases])
    _check_batch(dev, [c[0] for c in cases], heats, corpus.THRESHOLD, num=3)
    for name, heat, thr in cases:                      # and one by one: grid y = 1
        _check_batch(dev, [name], heat[None], thr, num=3)
    from unet_nested4tiny_objects_keypoints_amd import ops
    full = torch.from_numpy(heats[:1]).to(dev)
    for seg in SEGMENTATIONS:
        points, counts = ops.keypoints_extract(full, 1, corpus.THRESHOLD, segmentation=seg)
        want = [[0, 0]] if seg == "components" else ([[1, 1]] if min(shape) >= 3 else [])
        assert [[int(x), int(y)] for x, y in points[0, :int(counts[0])].cpu().tolist()] == want, (shape, seg)


def test_long_loops_run_past_their_first_batches(dev, monkeypatch):
    """the host loops of ops._keypoints_stages double their batches between blocking reads of the flag: the serpentine
    needs at least five batches of flood rounds, the solid blob at least four of distance sweeps"""
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    lib = _lib.lib()
    real, calls = lib.unetpp_keypoints_extract, {}

    def counted(stage, *args):
        calls[stage] = calls.get(stage, 0) + 1
        return real(stage, *args)

    monkeypatch.setattr(lib, "unetpp_keypoints_extract", counted)
    batches = {}
    singles = []
    for name, heat, thr in (corpus.serpentine(), corpus.solid_blob()):
        calls.clear()
        t = torch.from_numpy(heat[None]).to(dev)
        singles.append(ops.keypoints_regions(t, thr))
        batches[name] = dict(calls)
        _check_batch(dev, [name], heat[None], thr)
    assert batches["serpentine corridor"][7] >= 5, batches
    assert batches["solid blob"][4] >= 4, batches
    both = torch.from_numpy(np.stack([corpus.serpentine()[1], corpus.solid_blob()[1]])).to(dev)
    labels, dist = ops.keypoints_regions(both, corpus.THRESHOLD)
    for m, (one, d1) in enumerate(singles):            # the batch of the two gives what each gives alone
        assert torch.equal(one[0], labels[m]) and torch.equal(d1[0], dist[m])
    a_pts, a_cnt = ops.keypoints_extract(both, 3, corpus.THRESHOLD)
    for m in range(2):
        b_pts, b_cnt = ops.keypoints_extract(both[m:m + 1], 3, corpus.THRESHOLD)
        assert torch.equal(a_pts[m], b_pts[0]) and int(a_cnt[m]) == int(b_cnt[0])


@pytest.mark.parametrize("segmentation", SEGMENTATIONS)
def test_selection_paths_agree_on_tied_peaks(dev, segmentation):
    """kp_select_kernel ranks up to max_regions candidates against each other and takes the exact arg-max rounds above
    that: with max_regions = the region count (ranked), one less (uncapped) and 4096 the points and counts are the
    same bits, in the oracle's order -- peak descending, ties by the raster order of the regions' first pixels"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    num = 4
    for name, heat, thr in corpus.tie_cases():
        count = dict(zip(("components", "watershed"), corpus.TIE_COUNTS[name]))[segmentation]
        t = torch.from_numpy(heat[None]).to(dev)
        want, want_count = _oracle_points(heat, num, thr, segmentation)
        assert want_count == count
        if count <= num:                               # fewer regions than points asked for: padded with -1
            limits = (num, 4096)
            assert len(want) == count
        else:
            limits = (count, count - 1, 4096)
            peaks = [float(heat[y, x]) for x, y in want]
            assert peaks == sorted(peaks, reverse=True) and len(set(peaks)) < len(peaks), (name, peaks)   # a tie on top
        results = [_extract_twice(ops, t, num, thr, segmentation, max_regions=limit) for limit in limits]
        for points, counts in results:
            _check_points(points[0], counts[0], want, want_count, num, (name, segmentation))
            assert np.array_equal(points.view(np.int32), results[0][0].view(np.int32))


def test_holes_end_to_end_through_the_heatmap_front(dev):
    """Heatmap.transfer_points on a batch of the constructed hole cases (set into the top left corner of 64x72 maps)
    reports the points of the published algorithm: the plus-shaped hole's bright centre, (11, 11), is its blob's point"""
    from unet_nested4tiny_objects_keypoints_amd import Heatmap
    cases = corpus.hole_cases()
    maps = np.zeros((3, 2, 64, 72), dtype=np.float32)
    for k, (name, heat, thr) in enumerate(cases):
        maps[k // 2, k % 2, :heat.shape[0], :heat.shape[1]] = heat
    pattern = [[0], [1, 2]]
    hm = Heatmap(pattern, 72, 64)
    points, found = hm.transfer_points(torch.from_numpy(maps), threshold=corpus.THRESHOLD)
    again, found2 = hm.transfer_points(torch.from_numpy(maps), threshold=corpus.THRESHOLD)
    assert torch.equal(points, again) and torch.equal(found, found2)
    points, found = points.cpu().numpy(), found.cpu().numpy()
    want = transfer_points(maps, pattern, corpus.THRESHOLD)
    for n in range(3):
        for c in range(2):
            got = [[int(x), int(y)] for x, y in points[n, c, :int(found[n, c])]]
            assert got == want[n][c], (cases[2 * n + c][0], got)
            assert (points[n, c, int(found[n, c]):] == -1).all()
    assert want[0][0] == [[11, 11]] and want[0][1] == [[16, 15]]                 # plus, ring
    assert want[1][0] == [[40, 22]] and want[1][1] == [[21, 31]]                 # neck (one point asked for), no background
