"""Shape corpus for the heat map -> key points extraction (oracle/keypoints_oracle.py, csrc/keypoints.hip): seeded,
deterministic, every map as (name, heat float32 [H, W], threshold).  tests/test_keypoints_corpus.py holds the oracle's
synchronous flood against the sequential ``watershed_fifo`` on it (CPU); tests/test_gpu_keypoints.py the device against
the oracle, exactly.

What is left between the synchronous rounds of ``watershed_regions`` and ``watershed_fifo`` (known difference (2) of
unet_nested4tiny_objects_keypoints_amd/keypoints.py: which of two pixels of equal priority is served first), MEASURED on
the 200 maps of ``random_cases()`` as committed (seed 20), on the CPU:
  * region count or a region's (peak, first position) differ on 3 maps of 200 (1.5 %): random 075 (5x11), 085 (8x88) and
    134 (23x61).  In all three the pixels in question are ring pixels (mask value 0) beside the frame that one statement
    gives to a region and the other to its neighbour or to the line, and one of them carries a value above the
    threshold that the median took out of the mask.  The cap of the test is 2 % of the maps.
  * label maps: 111 of 42903 region pixels differ (0.26 %); 16 pixels are claimed by two different regions; the worst
    single map differs in 9 pixels.  The test asserts twice these figures (the seed is arbitrary) over the corpus as a
    whole, not per map.
  * on the six maps of ``hole_cases()`` the label maps are identical.
The single-phase flood this replaces reported a different point than ``watershed_fifo`` on 42 of the 200 maps.
"""
import numpy as np

THRESHOLD = 0.5
RANDOM_SEED = 20
RANDOM_COUNT = 200


def _square(h, w, y0, y1, x0, x1, value):
    heat = np.zeros((h, w), dtype=np.float32)
    heat[y0:y1, x0:x1] = value
    return heat


def hole_cases():
    """holes that a region encloses: narrower than 5 px they carry no background marker (the reference leaves two
    dilations around the mask unknown), so only the level-255 phase of the watershed reaches them"""
    plus = _square(24, 24, 5, 18, 5, 18, 0.7)            # the median turns the 3x3 patch into a plus-shaped hole
    plus[10:13, 10:13] = 0
    plus[11, 11] = 0.95
    yy, xx = np.mgrid[0:32, 0:32]
    rr = np.sqrt((yy - 15) ** 2 + (xx - 16) ** 2)
    ring = np.where((rr <= 9.2) & (rr >= 2.2), 0.7, 0).astype(np.float32)
    ring[15, 16] = 0.95
    pair = np.zeros((48, 72), dtype=np.float32)          # two squares joined by a two-pixel neck: two regions, and a hole
    pair[10:34, 6:30] = 0.8                              # at each mouth of the neck, each enclosed by ONE region.  (A
    pair[10:34, 38:62] = 0.7                             # hole on the line where the two floods meet is served in queue
    pair[21:23, 30:38] = 0.6                             # order: known difference (2), not a case for equal labels.)
    pair[20:23, 26:29] = 0
    pair[21, 27] = 0.95
    pair[21:24, 39:42] = 0
    pair[22, 40] = 0.97
    full = _square(64, 64, 2, 62, 2, 62, 0.8)            # no background marker anywhere: the ring is the region's
    full[30:34, 20:24] = 0
    full[31, 21] = 0.9
    dim = _square(28, 30, 4, 22, 5, 24, 0.7)             # the hole's bright pixel stays below the blob's own peak
    dim[8, 9] = 0.9
    dim[12:15, 14:17] = 0
    dim[13, 15] = 0.8
    wide = _square(40, 40, 4, 36, 4, 36, 0.7)            # wider than 5 px: the background marker sits in the hole
    wide[15:24, 16:25] = 0
    wide[19, 20] = 0.95
    return [("plus-shaped hole, bright centre", plus, THRESHOLD), ("ring, bright centre", ring, THRESHOLD),
            ("holes at the neck between two squares that touch", pair, THRESHOLD),
            ("4x4 hole in a blob without background", full, THRESHOLD),
            ("hole dimmer than the blob's peak", dim, THRESHOLD), ("hole wider than 5 px", wide, THRESHOLD)]


def random_cases(seed=RANDOM_SEED, count=RANDOM_COUNT):
    """`count` maps of 3..70 x 3..90 with 1..6 flat-topped discs (radius 1.5..9, every disc pixel above the threshold,
    one maximum at the centre) and up to 5 punched squares of side 1..4 centred on a blob pixel, every second one with a
    bright pixel in its middle"""
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(count):
        h, w = int(rng.integers(3, 71)), int(rng.integers(3, 91))
        yy, xx = np.mgrid[0:h, 0:w]
        heat = np.zeros((h, w), dtype=np.float64)
        for _ in range(int(rng.integers(1, 7))):
            cx, cy, r, a = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1.5, 9), rng.uniform(0.65, 0.94)
            d = np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)
            heat = np.maximum(heat, np.where(d <= r, a * (1 - 0.2 * (d / r) ** 2), 0))
        for j in range(int(rng.integers(0, 6))):
            ys, xs = np.nonzero(heat)
            if len(ys) == 0:
                break
            pick, side = int(rng.integers(0, len(ys))), int(rng.integers(1, 5))
            y0, x0 = max(int(ys[pick]) - side // 2, 0), max(int(xs[pick]) - side // 2, 0)
            heat[y0:y0 + side, x0:x0 + side] = 0
            if j % 2 == 0:
                heat[min(y0 + side // 2, h - 1), min(x0 + side // 2, w - 1)] = rng.uniform(0.95, 0.99)
        cases.append(("random %03d (%dx%d)" % (k, h, w), heat.astype(np.float32), THRESHOLD))
    return cases


BUCKETS = [(24, 32), (40, 48), (56, 64), (72, 96)]


def random_batches(seed=RANDOM_SEED, count=RANDOM_COUNT):
    """the random maps grouped for the device (one call per shape, grid y = map): every map is set into the smallest
    shape of BUCKETS that holds it, into one of its four corners in turn, so that each side of the frame keeps maps
    that touch it.  A padded map is a map of its own: the oracle runs on it as it stands.
    -> {shape: (names, float32 [maps, H, W])}"""
    groups = {shape: ([], []) for shape in BUCKETS}
    for k, (name, heat, _) in enumerate(random_cases(seed, count)):
        h, w = heat.shape
        bh, bw = next(s for s in BUCKETS if s[0] >= h and s[1] >= w)
        padded = np.zeros((bh, bw), dtype=np.float32)
        y0, x0 = (bh - h) * (k // 2 % 2), (bw - w) * (k % 2)
        padded[y0:y0 + h, x0:x0 + w] = heat
        groups[(bh, bw)][0].append(name)
        groups[(bh, bw)][1].append(padded)
    return {shape: (names, np.stack(maps)) for shape, (names, maps) in groups.items()}


def serpentine():
    """a 50x50 square with a 3-pixel corridor winding through a 128x128 map.  The corridor's thickest pixels are
    the inner corners of its bends (one straight + one diagonal step, 2.32 px) -- below a tenth of the square's 23.9 px,
    so the corridor has no core of its own and is flooded from the square's, one pixel per round."""
    heat = _square(128, 128, 4, 54, 4, 54, 0.8)          # the shape of solid_blob(): the two also run as one batch
    heat[26, 27] = 0.9
    heat[4:7, 54:64] = 0.7                                # out of the square's top right corner, bends only: a junction
    heat[4:92, 61:64] = 0.7                               # would be thick enough for a core.  Down, across, up again
    heat[89:92, 61:70] = 0.7
    heat[4:92, 67:70] = 0.7
    return "serpentine corridor", heat, THRESHOLD


def solid_blob():
    """a 126x126 square in a 128x128 map: the distance transform peaks 63 pixels from the rim"""
    return "solid blob", _square(128, 128, 1, 127, 1, 127, 0.8), THRESHOLD


TIE_THRESHOLD = 0.7
# (name, regions as 8-connected components of the mask, regions of the watershed): checked on the host
TIE_COUNTS = {"speckle 24x32": (19, 14), "speckle 33x47": (15, 15), "speckle 40x40": (38, 33), "three regions, two tie": (3, 3)}


def tie_cases():
    """speckled maps whose values come from {0.75, 0.8, 0.9}: the peaks of many regions tie, so the order of the points
    is the raster order of the regions' first pixels; and a map with fewer regions than points are asked for"""
    rng = np.random.default_rng(5)
    cases = []
    for name, (h, w), fill in [("speckle 24x32", (24, 32), 0.45), ("speckle 33x47", (33, 47), 0.5), ("speckle 40x40", (40, 40), 0.4)]:
        value = rng.choice(np.array([0.75, 0.8, 0.9], dtype=np.float32), size=(h, w))
        heat = np.where(rng.uniform(size=(h, w)) < fill, value, 0).astype(np.float32)
        cases.append((name, heat, TIE_THRESHOLD))
    few = np.zeros((20, 30), dtype=np.float32)
    few[3:8, 3:8] = 0.8
    few[10:16, 18:25] = 0.8
    few[12:17, 4:9] = 0.9
    cases.append(("three regions, two tie", few, TIE_THRESHOLD))
    return cases


DEGENERATE_SHAPES = [(1, 1), (1, 17), (23, 1), (2, 2), (3, 3), (4, 31), (31, 4)]


def degenerate_cases():
    """the smallest legal shapes, each all above the threshold, all zero, and random"""
    rng = np.random.default_rng(6)
    cases = []
    for h, w in DEGENERATE_SHAPES:
        cases.append(("%dx%d full" % (h, w), np.full((h, w), 0.9, dtype=np.float32), THRESHOLD))
        cases.append(("%dx%d zero" % (h, w), np.zeros((h, w), dtype=np.float32), THRESHOLD))
        cases.append(("%dx%d random" % (h, w), rng.uniform(0.2, 1.0, (h, w)).astype(np.float32), THRESHOLD))
    return cases
