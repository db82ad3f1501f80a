"""Ignore masks without a GPU, against tests/mask_oracle.py: the rules (which sides of an axis-aligned ring are
inclusive, the partition property of two rings that share an edge, the rule in whole numbers), IgnoreMask / IgnoreUnion
on CPU tensors, the filter ``evaluate`` applies, the ABI entries, what the generated cases exercise, and that every
planted mutation of the oracle changes a case the GPU tests hold the kernels to."""
import os
import re

import numpy as np
import pytest
import torch

from tests import ignore_oracle as io
from tests import mask_oracle as mo

F32, I32 = np.float32, np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("unetpp_mask_pack", "unetpp_mask_polygons", "unetpp_target_ignore_mask")


def _mask(raster, plane_class=None):
    from unet_nested4tiny_objects_keypoints_amd import IgnoreMask
    return IgnoreMask.from_raster(torch.from_numpy(np.ascontiguousarray(raster)), plane_class)


# the rules -----------------------------------------------------------------------------------------------------------
def test_an_axis_aligned_ring_is_closed_on_the_left_and_top_and_open_on_the_right_and_bottom():
    """ring (x0, y0) - (x1, y1) on whole numbers: the pixels x0 <= px < x1, y0 <= py < y1 -- the left and top sides
    are inclusive, the right and bottom sides exclusive.  That is IgnoreRegions' rectangle (x0, y0, x1 - 1, y1 - 1)."""
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions
    H, W = 20, 30
    ys, xs = np.mgrid[0:H, 0:W]
    pts = torch.from_numpy(np.stack([xs, ys], axis=-1).astype(F32))
    for x0, y0, x1, y1 in ((3, 2, 11, 9), (0, 0, 30, 20), (5, 5, 6, 6), (-4, 7, 12, 40)):
        for ring in ([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], [(x0, y1), (x1, y1), (x1, y0), (x0, y0)]):     # both ways round
            got = mo.ring_inside(np.asarray(ring, F32), (H, W))
            want = IgnoreRegions(np.asarray([[[x0, y0, x1 - 1, y1 - 1]]], F32)).contains(0, 0, pts).numpy()
            assert np.array_equal(got, want), ring
            assert np.array_equal(got, (x0 <= xs) & (xs < x1) & (y0 <= ys) & (ys < y1))
    got = mo.ring_inside(np.asarray([(3, 2), (11, 2), (11, 9), (3, 9)], F32), (H, W))
    assert got[2, 3] and got[5, 3] and got[2, 7]                      # the left and top sides, and their corner
    assert not got[5, 11] and not got[9, 7] and not got[9, 11]        # the right and bottom sides
    assert got[8, 10] and not got[2, 11] and not got[9, 3]            # the last pixel inside; the other two corners


@pytest.mark.parametrize("seed", range(6))
def test_two_rings_that_share_an_edge_partition_the_ring_they_were_cut_from(seed):
    c = mo.partition_case(seed)
    size = mo.PARTITION_SIZE
    whole, left, right = (mo.ring_inside(c[k], size) for k in ("whole", "left", "right"))
    assert not (left & right).any()                                  # a pixel is in at most one of the halves
    assert np.array_equal(left | right, whole)                       # and in one of them iff it is in the uncut ring
    assert left.any() and right.any() and not whole.all()
    for k, got in (("whole", whole), ("left", left), ("right", right)):
        assert np.array_equal(got, mo.ring_inside_int(c[k + "_q"], size)), k
    # the chord passes through pixel centres: d == 0 there, and those pixels belong to exactly one half
    on_chord = [(20 + 4 * t, 18 + 3 * t) for t in range(-2, 3)]
    assert all(left[y, x] != right[y, x] for x, y in on_chord)
    # reversing a ring changes nothing
    assert np.array_equal(mo.ring_inside(c["left"][::-1], size), left)


# the container on CPU tensors ------------------------------------------------------------------------------------------
def _raster(seed=0, S=2, P=3, H=17, W=70):
    return np.random.default_rng(300 + seed).random((S, P, H, W)) < 0.3


def test_from_raster_to_raster_coverage_and_union_on_the_cpu():
    from unet_nested4tiny_objects_keypoints_amd import IgnoreMask
    for W in (1, 31, 32, 33, 64, 65, 130):
        r = _raster(W, W=W)
        m = _mask(r, [-1, 0, 2])
        assert m.bits.dtype == torch.int32 and tuple(m.bits.shape) == (2, 3, 17, (W + 31) // 32)
        assert np.array_equal(m.bits.numpy(), mo.pack(r)) and mo.tails(m.bits.numpy(), W) == 0
        assert np.array_equal(m.to_raster().numpy(), r) and len(m) == 2 and m.device.type == "cpu" and m.to("cpu") is m
        assert np.allclose(m.coverage().numpy(), r.mean(axis=(2, 3)), rtol=0, atol=1e-15)
        other = _raster(W + 1000, W=W)
        assert np.array_equal(m.union(_mask(other, [-1, 0, 2])).to_raster().numpy(), r | other)
        with pytest.raises(ValueError):
            m.union(_mask(other, [-1, 0, 1]))                        # other plane classes
        with pytest.raises(ValueError):
            m.union(_mask(other[:, :2], [-1, 0]))                    # other geometry
    # dtypes: uint8, bool and float with a NaN and a -0.0; [S, H, W] is one plane of every class
    f = np.zeros((1, 4, 40), F32)
    f[0, 1, 3], f[0, 2, 39], f[0, 3, 0], f[0, 0, 5] = np.nan, -0.0, 1e-45, -2.5
    m = _mask(f)
    assert tuple(m.bits.shape) == (1, 1, 4, 2) and m.plane_class.tolist() == [-1]
    assert np.array_equal(m.to_raster().numpy()[:, 0], mo.nonzero(f)) and int(m.to_raster().sum()) == 3
    for dtype in (np.uint8, bool, np.float64, np.int64):
        assert np.array_equal(_mask(mo.nonzero(f).astype(dtype)).bits.numpy(), m.bits.numpy())
    with pytest.raises(ValueError):
        IgnoreMask(m.bits, (4, 70))                                  # bits that do not hold such frames
    with pytest.raises(ValueError):
        _mask(f, [0, 1])                                             # plane_class of another length
    with pytest.raises(ValueError):
        _mask(f, [0.5])


def test_contains_is_the_lookup_rule():
    r = _raster(5, S=3)
    classes = [-1, 1, 7]
    m = _mask(r, classes)
    rng = np.random.default_rng(6)
    xy = rng.uniform(-3, 73, (4, 500, 2)).astype(F32)
    xy[..., 1] = rng.uniform(-3, 20, (4, 500))
    xy[0, :8] = [(0, 0), (69, 16), (69.4, 16), (69.5, 16), (-0.4, 3), (10.5, 3.5), (np.nan, 2), (4, np.nan)]
    xy[1, :200] = np.round(xy[1, :200] * 2) / 2                       # whole and half-way positions
    frame = rng.integers(-1, 5, (4, 500))
    cls = rng.integers(0, 3, (4, 500))
    got = m.contains(torch.from_numpy(frame), torch.from_numpy(cls), torch.from_numpy(xy)).numpy()
    want = mo.contains(r, classes, frame, cls, xy)
    assert np.array_equal(got, want) and 0.05 < want.mean() < 0.6
    assert not got[0, 3] and not got[0, 4] and not got[0, 6] and not got[0, 7]      # outside the frame, and NaN
    # broadcasting as IgnoreRegions.contains: ints, and [S, 1] against [S, L]
    assert np.array_equal(m.contains(1, 1, torch.from_numpy(xy)).numpy(), mo.contains(r, classes, 1, 1, xy))
    f3 = torch.arange(3).view(3, 1)
    pts = torch.from_numpy(xy[:3, :9])
    assert np.array_equal(m.contains(f3, torch.from_numpy(cls[:3, :9]), pts).numpy(),
                          mo.contains(r, classes, np.arange(3).reshape(3, 1), cls[:3, :9], xy[:3, :9]))
    for mutation in ("floor_not_nearest", "class_plane_for_every_class"):
        assert not np.array_equal(mo.contains(r, classes, frame, cls, xy, mutation), want), mutation


def test_a_union_contains_what_one_of_its_parts_contains():
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions, IgnoreUnion
    r = _raster(8)
    m, m2 = _mask(r, [-1, 0, 1]), _mask(_raster(9)[:, :1])
    rects = IgnoreRegions(np.asarray([[[2, 2, 30, 9], [40, 0, 69, 3]], [[0, 0, 5, 16], [9, 9, 8, 8]]], F32), [[-1, 2], [0, -1]])
    rng = np.random.default_rng(10)
    xy = torch.from_numpy(np.stack([rng.uniform(-2, 72, (2, 3, 50)), rng.uniform(-2, 19, (2, 3, 50))], -1).astype(F32))
    frame, cls = torch.arange(2).view(2, 1, 1), torch.arange(3).view(1, 3, 1)
    u = IgnoreUnion(rects, m, m2)
    want = rects.contains(frame, cls, xy) | m.contains(frame, cls, xy) | m2.contains(frame, cls, xy)
    assert torch.equal(u.contains(frame, cls, xy), want) and len(u) == 2 and u.to("cpu") is u
    assert bool((want != rects.contains(frame, cls, xy)).any()) and bool((want != m.contains(frame, cls, xy)).any())
    assert torch.equal(IgnoreUnion(IgnoreUnion(rects, m), m2).contains(frame, cls, xy), want)       # nesting flattens
    assert torch.equal(IgnoreUnion([m]).contains(frame, cls, xy), m.contains(frame, cls, xy))
    with pytest.raises(ValueError):
        IgnoreUnion(rects, _mask(r[:1]))                             # another number of frames
    with pytest.raises(TypeError):
        IgnoreUnion(rects, r)
    with pytest.raises(ValueError):
        IgnoreUnion()


def test_the_filter_evaluate_applies():
    """``evaluate`` matches on the GPU only; the two ``contains`` calls it makes, with its shapes: labels [S, L, 2] with
    frame [S, 1] and cls [S, L]; detections [S, C, cap, 2] with frame [S, 1, 1] and cls [1, C, 1]"""
    S, C, L, cap = 2, 2, 5, 4
    r = np.zeros((S, 2, 64, 64), bool)
    r[0, 0, 4:21, 44:61] = True                                      # class 0 only
    r[0, 1, 24:37, 0:17] = True                                      # every class
    m = _mask(r, [0, -1])
    labels = torch.tensor([[[10., 12.], [55., 15.], [8., 30.], [-1., -1.], [50., 10.]]] * S)
    cls = torch.tensor([[0, 0, 1, -1, 1]] * S)
    dropped = m.contains(torch.arange(S).view(S, 1), cls, labels)
    assert dropped.tolist() == [[False, True, True, False, False], [False] * 5]
    xy = torch.zeros(S, C, cap, 2)
    xy[0, 0, :3] = torch.tensor([[50., 10.], [10., 12.], [8., 30.]])
    xy[0, 1, :2] = torch.tensor([[50., 10.], [8.4, 30.4]])
    served = ~m.contains(torch.arange(S).view(S, 1, 1), torch.arange(C).view(1, C, 1), xy)
    assert served[0, 0, :3].tolist() == [False, True, False] and served[0, 1, :2].tolist() == [True, False]
    assert bool(served[1].all())


def test_from_polygons_has_no_cpu_path():
    from unet_nested4tiny_objects_keypoints_amd import IgnoreMask, ops
    c = mo.polygon_case(33, 70, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IgnoreMask.from_polygons(torch.from_numpy(np.array(c["vertices"])), torch.from_numpy(np.array(c["counts"])), (33, 70))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_pack(torch.zeros(2, 3, 40, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.target_ignore_mask(torch.zeros(1, 1, 4, 4), None, None, torch.zeros(1, dtype=torch.int64), torch.zeros(1, 16),
                               (8, 8), True, n_frames=1)


# the ABI ---------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_listed_and_built():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unetpp_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert "mask.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "mask.hip"))
    assert _lib.lib().unetpp_abi_version() == _lib.ABI_VERSION == 14
    text = open(os.path.join(_lib.CSRC, "mask.hip")).read()
    assert "#pragma clang fp contract(off)" in text
    assert int(re.search(r"kEdgeChunk = (\d+)", text).group(1)) == mo.EDGE_CHUNK
    lib = _lib.lib()                                                 # refusals that never touch a device
    assert lib.unetpp_mask_pack(None, 0, 4, 4, None, None) == -1
    assert lib.unetpp_mask_polygons(None, None, None, None, 1, 0, 0, 1, 4, 4, None, None) == -1
    assert lib.unetpp_target_ignore_mask(None, None, 1, 0, 4, 4, None, 1, None, 1, 4, 4, 1, None, None) == -1


# the cases -------------------------------------------------------------------------------------------------------------
def test_what_the_polygon_cases_exercise():
    for H, W in mo.POLY_FRAMES:
        facts = mo.case_facts(mo.polygon_case(H, W, 40))
        assert facts["level_edge"] and facts["vertex_on_centre"] and facts["d_zero"] and facts["long_ring"], facts
        assert facts["outside_ring"] and facts["nan_ring"] and facts["inf_ring"] and facts["clear_ring"], facts
        assert facts["planes_used"] == mo.POLY_PLANES
        assert mo.LONG_RING == mo.EDGE_CHUNK + 44
        want = mo.polygon_expected(H, W, 40)
        for s in range(2):
            for p in range(mo.POLY_PLANES):
                assert want[s, p].any() and not want[s, p].all(), (H, W, s, p)
        c = mo.polygon_case(H, W, 40)
        # the hole and the island: the clearing ring removed pixels of the star, the island put some back
        star = mo.ring_inside(c["vertices"][0, 3, :c["counts"][0, 3]], (H, W))
        hole = mo.ring_inside(c["vertices"][0, 4, :c["counts"][0, 4]], (H, W))
        island = mo.ring_inside(c["vertices"][0, 5, :c["counts"][0, 5]], (H, W))
        assert (star & hole & ~island).any() and island.any() and (island & ~hole).sum() == 0
        # the padding rings would have covered the frame
        for g in (7, 13, 18):
            assert mo.ring_is_padding(c["vertices"][0, g], int(c["counts"][0, g]), c["vertices"].shape[2])
        one = mo.polygon_expected(H, W, 1)
        assert all(one[s, 0].any() and not one[s, 0].all() for s in range(2)) and not one[:, 1:].any()
        assert not mo.polygon_expected(H, W, 0).any()
        # permuting the setting rings between two clearing rings changes nothing
        perm = mo.permuted_sets(c)
        assert not np.array_equal(perm["counts"], c["counts"])
        assert np.array_equal(mo.polygons(perm["vertices"], perm["counts"], (H, W), perm["poly_plane"], perm["poly_clear"],
                                          mo.POLY_PLANES), want)


POLYGON_MUTATIONS = ("endpoints_not_ordered", "d_ge_zero", "straddle_upper_inclusive", "closing_edge_dropped",
                     "clear_rings_ignored", "list_order_reversed", "cull_drops_touching_row")


@pytest.mark.parametrize("mutation", mo.MUTATIONS)
def test_every_planted_mutation_changes_a_case_of_the_gpu_suite(mutation):
    assert set(POLYGON_MUTATIONS) < set(mo.MUTATIONS) and len(mo.MUTATIONS) == 10
    if mutation in POLYGON_MUTATIONS:
        H, W = mo.POLY_FRAMES[0]
        assert not np.array_equal(mo.polygon_expected(H, W, 40, mutation=mutation), mo.polygon_expected(H, W, 40))
        if mutation == "cull_drops_touching_row":                    # exactly the planted rows are lost
            lost = mo.polygon_expected(H, W, 40) & ~mo.polygon_expected(H, W, 40, mutation=mutation)
            assert lost[0, 0, 15].any() and lost[0, 1, H - 1].any()
    elif mutation == "tail_bits_not_zeroed":
        for W in (1, 31, 33, 65, 130):
            r = _raster(W, W=W)
            assert not np.array_equal(mo.pack(r, mutation), mo.pack(r)) and mo.tails(mo.pack(r, mutation), W) != 0
    else:
        c = mo.dihedral_case(40, 48)
        args = (c["raster"], c["plane_class"], c["index"], c["rows"], c["C"], c["out_size"], True)
        assert not np.array_equal(mo.mark_mask_bits(*args, mutation=mutation), mo.mark_mask_bits(*args))
        N, C, Ho, Wo = io.MARK_SHAPES[0]
        c = mo.mark_case(N, C, Ho, Wo, 4, first_kind=1)                 # flip, (an index outside), general
        args = (c["raster"], c["plane_class"], c["index"], c["rows"], C, (Ho, Wo), False)
        assert not np.array_equal(mo.mark_mask_bits(*args, mutation=mutation), mo.mark_mask_bits(*args))


def test_what_the_mark_cases_exercise():
    c = mo.dihedral_case(40, 48)
    for outside in (False, True):
        mask = mo.mark_mask_bits(c["raster"], c["plane_class"], c["index"], c["rows"], c["C"], c["out_size"], outside)
        assert mask[-1].all() == outside and mask[-1].any() == outside                  # index = -1
        assert all(0.02 < mask[n].mean() < 0.98 for n in range(10)), [float(mask[n].mean()) for n in range(10)]
        assert (mask[:10, 0] != mask[:10, 2]).any() and (mask[:10, 1] != mask[:10, 2]).any()   # the class planes matter
    # the windows overhang the frame, and the general one lands between pixels
    xs, ys = io.source_positions(c["rows"][9], 40, 48)
    assert (xs != np.round(xs)).any() and (xs < 0).any()
    # rectangles as a raster: what IgnoreRegions contains at whole-number positions
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions
    rects = np.asarray([[[3, 8, 9, 15], [10.5, 2, 12.5, 4], [5, 5, 4, 4], [np.nan, 0, 3, 3], [20, 40, 40, 60]]], F32)
    rcls = np.asarray([[-1, 1, -1, -1, 2]], I32)
    raster, classes = mo.rects_raster(rects, rcls, 2, (50, 30))
    ys_, xs_ = np.mgrid[0:50, 0:30]
    pts = torch.from_numpy(np.stack([xs_, ys_], -1).astype(F32))
    for k in range(2):
        want = IgnoreRegions(rects, rcls).contains(0, k, pts).numpy()
        assert np.array_equal(mo.contains(raster, classes, 0, k, pts.numpy()), want) and want.any()
