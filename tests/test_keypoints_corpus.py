"""The oracle's flood (oracle/keypoints_oracle.py: synchronous rounds, level 0 and level 255 in turn -- what the device
kernel follows) against the sequential statement of the published watershed, ``watershed_fifo``, on the shape corpus of
tests/keypoints_corpus.py; and the host-side facts the device tests of tests/test_gpu_keypoints.py rely on (how many
rounds a map needs, how many regions it has).  CPU only."""
import numpy as np
from scipy import ndimage

from oracle.keypoints_oracle import (chamfer_distance, extract_points, flood_round, region_markers, region_mask,
                                     watershed_fifo, watershed_flood, watershed_regions)
from tests import keypoints_corpus as corpus


def _fifo_regions(mask):
    flooded = watershed_fifo(mask, region_markers(mask)[0])
    labels = np.where(flooded >= 2, flooded - 1, 0)
    return labels, [int(v) for v in np.unique(labels[labels > 0])]


def _single_phase_regions(mask):
    """the flood before it had a level-255 phase: level-0 rounds only"""
    mk, _ = region_markers(mask)
    mk[0, :] = mk[-1, :] = -1
    mk[:, 0] = mk[:, -1] = -1
    moved = True
    while moved:
        mk, moved = flood_round(mk, mask)
    labels = np.where(mk >= 2, mk - 1, 0)
    return labels, [int(v) for v in np.unique(labels[labels > 0])]


def _peaks(labels, present, heat, thr):
    """(peak, raster index of its first pixel) per region, as the extraction reports them"""
    hz = np.where(heat < thr, 0, heat)
    inside = [np.where(labels == lab, hz, 0) for lab in present]
    return [(float(a.max()), int(np.argmax(a))) for a in inside]


def test_hole_cases_equal_the_sequential_watershed():
    """identical label maps, identical (peak, position) per region; and the published points"""
    points = {}
    for name, heat, thr in corpus.hole_cases():
        mask = region_mask(heat, thr)
        labels, present = watershed_regions(mask)
        fifo, fifo_present = _fifo_regions(mask)
        np.testing.assert_array_equal(labels, fifo, err_msg=name)
        assert present == fifo_present and _peaks(labels, present, heat, thr) == _peaks(fifo, present, heat, thr), name
        points[name] = (extract_points(heat, 3, thr), labels)
    assert points["plus-shaped hole, bright centre"][0] == [[11, 11]]          # the hole's bright pixel is the region's
    assert points["ring, bright centre"][0] == [[16, 15]]
    assert points["holes at the neck between two squares that touch"][0] == [[40, 22], [27, 21]]
    full, labels = points["4x4 hole in a blob without background"]
    assert full == [[21, 31]] and (labels[1:-1, 1:-1] == 1).all()              # the two-pixel ring included
    assert points["hole dimmer than the blob's peak"][0] == [[9, 8]]           # the point does not move
    wide, labels = points["hole wider than 5 px"]
    assert wide == [[5, 4]] and labels[19, 20] == 0                            # the background marker owns the hole


def test_the_corpus_sees_the_missing_level_255_phase():
    """the single-phase flood reports another point than the sequential watershed on the plus hole and on the ring"""
    cases = {name: (heat, thr) for name, heat, thr in corpus.hole_cases()}
    for name in ("plus-shaped hole, bright centre", "ring, bright centre"):
        heat, thr = cases[name]
        mask = region_mask(heat, thr)
        old, old_present = _single_phase_regions(mask)
        fifo, fifo_present = _fifo_regions(mask)
        assert old_present == fifo_present == [1]
        assert _peaks(old, [1], heat, thr) != _peaks(fifo, [1], heat, thr), name


def test_random_cases_against_the_sequential_watershed():
    """points on all but 2 % of the maps; labels within twice the share measured on this corpus (corpus docstring)"""
    cases = corpus.random_cases()
    assert len(cases) == 200
    moved, differ, twice, region, worst = [], 0, 0, 0, 0
    for name, heat, thr in cases:
        mask = region_mask(heat, thr)
        labels, present = watershed_regions(mask)
        fifo, fifo_present = _fifo_regions(mask)
        if present != fifo_present or _peaks(labels, present, heat, thr) != _peaks(fifo, fifo_present, heat, thr):
            moved.append(name)
        d = int((labels != fifo).sum())
        differ, worst = differ + d, max(worst, d)
        twice += int(((labels > 0) & (fifo > 0) & (labels != fifo)).sum())
        region += int((labels > 0).sum())
    print("points differ on %d of %d maps: %s" % (len(moved), len(cases), moved))
    print("labels differ on %d of %d region pixels (%.3f %%), %d in two regions, worst map %d" % (
        differ, region, 100.0 * differ / region, twice, worst))
    assert len(moved) <= 0.02 * len(cases), moved
    assert differ <= 2 * 0.0026 * region      # measured 111 of 42903 = 0.26 %
    assert twice <= 2 * 16 and worst <= 2 * 9


def test_long_loop_cases_need_the_later_batches():
    """the host loops double their batches (8, 16, 32, 64 distance sweeps; 8, 16, 32, 64, 128 flood rounds)"""
    name, heat, thr = corpus.serpentine()
    mask = region_mask(heat, thr)
    _, rounds, crossings = watershed_flood(mask)
    assert rounds > 128, rounds                                     # 8 + 16 + 32 + 64 = 120: a fifth batch
    assert watershed_regions(mask)[1] == [1] and extract_points(heat, 3, thr) == [[27, 26]]
    name, heat, thr = corpus.solid_blob()
    assert chamfer_distance(region_mask(heat, thr)).max() > 60 * 65536   # one sweep per pixel: 8 + 16 + 32 = 56, a fourth


def test_tie_cases_have_the_stated_region_counts():
    for name, heat, thr in corpus.tie_cases():
        mask = region_mask(heat, thr)
        components = ndimage.label(mask, structure=np.ones((3, 3), dtype=int))[1]
        assert (components, len(watershed_regions(mask)[1])) == corpus.TIE_COUNTS[name], name
        assert set(np.unique(heat)) <= {np.float32(0), np.float32(0.75), np.float32(0.8), np.float32(0.9)}
    # ties are what these maps are for: more regions than distinct peak values
    assert all(c > 3 for n, (c, _) in corpus.TIE_COUNTS.items() if n.startswith("speckle"))


def test_degenerate_shapes_on_the_oracle():
    for name, heat, thr in corpus.degenerate_cases():
        h, w = heat.shape
        watershed, components = extract_points(heat, 3, thr), extract_points(heat, 3, thr, "components")
        if min(h, w) < 3:
            assert watershed == [], name                            # nothing but frame
        if name.endswith("full"):
            assert components == [[0, 0]] and watershed == ([[1, 1]] if min(h, w) >= 3 else []), name
        if name.endswith("zero"):
            assert watershed == [] and components == [], name
