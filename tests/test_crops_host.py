"""CPU checks of training on scenes (crops.py, csrc/crops.hip) and of the restatement the GPU tests hold the kernels
against (tests/crops_oracle.py):
  (1) argument checks of the two entry points (status codes, no device touched);
  (2) the culling rule of the target kernel, restated in numpy, gives the brute-force minima bit for bit;
  (3) the draw's restatement: whole-number rows for the exact family, origins inside the frame or a centred pad;
  (4) false_positive_centres on hand-made detections;
  (5) the Python argument errors and no CPU fallback."""
import ctypes

import numpy as np
import pytest
import torch

from tests import crops_oracle as co


def _lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


# (1) -----------------------------------------------------------------------------------------------------------------
def test_points_target_argument_checks_touch_no_device():
    L = _lib()
    lib = L.lib()
    p = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host

    def target(labels=p, label_class=p, M=2, L=5, index=p, N=3, params=p, C=4, Ho=8, Wo=8, radius=3.0, out=p):
        return lib.unetpp_points_target(labels, label_class, M, L, index, N, params, C, Ho, Wo, radius, out, None)

    for name in ("labels", "label_class", "index", "params", "out"):
        assert target(**{name: None}) == -1, name
    for name in ("M", "L", "N", "C", "Ho", "Wo"):
        assert target(**{name: 0}) == -1, name
        assert target(**{name: -2}) == -1, name
    assert target(C=65536) == -1
    assert target(Ho=(1 << 24) + 1) == -1 and target(Wo=(1 << 24) + 1) == -1
    for radius in (0.0, -1.0, float("nan")):
        assert target(radius=radius) == -1, radius


def test_crops_draw_argument_checks_touch_no_device():
    L = _lib()
    lib = L.lib()
    p = ctypes.c_void_p(0x1000)

    def aug(**kw):
        d = dict(p_flip_h=0.5, p_flip_v=0.5, rot90=1, max_deg=0.0, scale_lo=1.0, scale_hi=1.0, max_tx=0.0, max_ty=0.0,
                 gain_lo=1.0, gain_hi=1.0, max_bias=0.0, reserved=0)
        d.update(kw)
        return L.AugmentDesc(**d)

    def draw(params=p, index=p, origin=p, N=4, M=2, Hs=64, Ws=64, Ho=16, Wo=16, frame=p, xy=p, V=3, p_object=0.5,
             jx=2.0, jy=2.0, a=None, null_aug=False):
        a = aug() if a is None else a
        return lib.unetpp_crops_draw(params, index, origin, N, 7, M, Hs, Ws, Ho, Wo, frame, xy, V, p_object, jx, jy,
                                     None if null_aug else ctypes.byref(a), None)

    for name in ("params", "index", "origin", "frame", "xy"):
        assert draw(**{name: None}) == -1, name
    assert draw(null_aug=True) == -1
    for name in ("N", "M", "Hs", "Ws", "Ho", "Wo"):
        assert draw(**{name: 0}) == -1, name
        assert draw(**{name: -1}) == -1, name
    assert draw(V=-1) == -1
    assert draw(Ws=(1 << 24) + 1) == -1
    assert draw(a=aug(max_tx=1.0)) == -1 and draw(a=aug(max_ty=2.0)) == -1
    assert draw(Ho=16, Wo=24) == -1                          # quarter turns need a square window
    assert draw(a=aug(scale_lo=0.0)) == -1
    for bad in (-0.1, float("nan")):
        assert draw(p_object=bad) == -1 and draw(jx=bad) == -1 and draw(jy=bad) == -1


# (2) -----------------------------------------------------------------------------------------------------------------
def test_culled_minima_are_the_brute_force_minima():
    most = {}
    for name, Ho, Wo, xo, yo in co.cull_cases():
        want = co.brute_minima(xo, yo, Ho, Wo)
        for tile in ((co.TILE_H, co.TILE_W), (8, 8), (16, 16)):
            got, kept = co.culled_minima(xo, yo, Ho, Wo, tile)
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (name, tile)
            most[name, tile] = kept
    print("labels kept per tile at most:", most)
    kernel_tile = (co.TILE_H, co.TILE_W)
    assert most["300 coincident", kernel_tile] == 300          # coincident labels all survive, as they must
    assert most["2000 over 4096 px", kernel_tile] <= 32         # ... and a scattered crowd is cut to a handful


def test_target_restatement_by_hand():
    labels = np.array([[[5.0, 3.0], [-1.0, -1.0], [9.0, 3.0], [2.0, 2.0]]], dtype=np.float32)
    classes = np.array([[0, 0, 0, 5]], dtype=np.int32)
    row = np.zeros((1, 16), dtype=np.float32)
    row[0, [0, 4, 6, 10, 12]] = 1.0
    out = co.points_target_ref(labels, classes, [0], row, 2, (6, 12), 2.0)
    assert out.shape == (1, 2, 6, 12) and out.dtype == np.float32
    assert out[0, 0, 3, 5] == 1.0 and out[0, 0, 3, 9] == 1.0 and not out[0, 1].any()
    assert out[0, 0, 3, 7] == np.float32(np.exp(-0.5 * 2.0 / 2.0)) == out[0, 0, 3, 3]
    assert not co.points_target_ref(labels, classes, [1], row, 2, (6, 12), 2.0).any()      # an index outside [0, M)


# (3) -----------------------------------------------------------------------------------------------------------------
def test_draw_restatement_rows_origins_and_pads():
    frames = np.array([0, 1, 2, 2, 7], dtype=np.int64)
    xy = np.array([[0.0, 0.0], [89.0, 69.0], [40.4, 30.6], [12.0, 66.0], [5.0, 5.0]], dtype=np.float32)
    got = co.crops_draw_ref(300, 99, 3, (70, 90), (32, 32), frames, xy, 0.6, (5, 7))
    rows, origin = got["rows"], got["origin"]
    assert np.array_equal(rows[:, :12], np.round(rows[:, :12]))                 # the exact family: whole numbers
    assert (origin[:, 0] >= 0).all() and (origin[:, 0] <= 90 - 32).all()
    assert (origin[:, 1] >= 0).all() and (origin[:, 1] <= 70 - 32).all()
    assert (origin[:, 0] == 0).any() and (origin[:, 0] == 58).any()             # the clamp acted on both sides
    assert got["object"].any() and not got["object"].all()
    assert (got["index"][got["object"]] == -1).any()                            # the table row of frame 7
    assert set(np.unique(got["index"])) <= {-1, 0, 1, 2}
    # the inverse map sends the window's corner pixels to frame pixels of the window
    for i in range(20):
        inv = rows[i, :6].reshape(2, 3)
        for corner in ((0, 0), (31, 0), (0, 31), (31, 31)):
            sx, sy = inv @ np.array([corner[0], corner[1], 1.0])
            assert origin[i, 0] <= sx <= origin[i, 0] + 31 and origin[i, 1] <= sy <= origin[i, 1] + 31
    pad = co.crops_draw_ref(64, 5, 2, (24, 40), (32, 48), frames[:3], xy[:3], 0.5, (3, 3), rot90=False)
    assert (pad["origin"] == np.array([-4, -4])).all()                          # a centred pad on both axes
    none = co.crops_draw_ref(64, 5, 2, (70, 90), (32, 32), [], np.zeros((0, 2)), 0.9, (3, 3))
    assert not none["object"].any() and set(np.unique(none["index"])) == {0, 1}


# (4) -----------------------------------------------------------------------------------------------------------------
def test_false_positive_centres_by_hand():
    from unet_nested4tiny_objects_keypoints_amd import Detections, false_positive_centres
    from unet_nested4tiny_objects_keypoints_amd.detect import score_matches
    S, C, cap = 2, 2, 3
    xy = torch.full((S, C, cap, 2), -1.0)
    score = torch.full((S, C, cap), float("-inf"))
    count = torch.tensor([[2, 0], [5, 1]], dtype=torch.int32)                   # (1, 0) is truncated: 5 peaks, 3 slots
    xy[0, 0, :2] = torch.tensor([[10.0, 10.0], [50.0, 60.0]])
    score[0, 0, :2] = torch.tensor([0.9, 0.8])
    xy[1, 0] = torch.tensor([[5.0, 5.0], [20.0, 20.0], [30.0, 31.0]])
    score[1, 0] = torch.tensor([0.9, 0.7, 0.3])
    xy[1, 1, 0], score[1, 1, 0] = torch.tensor([7.0, 8.0]), 0.6
    dets = Detections(xy, score, count)
    pred_label = torch.full((S, C, cap), -1, dtype=torch.int32)
    pred_label[0, 0, 0] = 0                                                    # matched: not a false positive
    pred_label[1, 0, 1] = 1
    labels = torch.tensor([[[10.0, 10.0], [-1.0, -1.0]], [[70.0, 70.0], [20.0, 20.0]]])
    label_class = torch.tensor([[0, -1], [1, 0]], dtype=torch.int32)
    label_pred = torch.tensor([[0, -1], [-1, 1]], dtype=torch.int32)
    stats = torch.tensor([[[1, 1, 0], [0, 0, 0]], [[1, 2, 0], [0, 1, 1]]], dtype=torch.int32)
    served = torch.arange(cap).view(1, 1, cap) < count.clamp(max=cap).unsqueeze(-1)
    result = score_matches(xy, score, served, pred_label, label_pred, stats, labels, label_class)
    frame, centres = false_positive_centres(dets, result)
    assert frame.dtype == torch.int32 and centres.dtype == torch.float32
    assert frame.tolist() == [0, 1, 1, 1]
    assert centres.tolist() == [[50.0, 60.0], [5.0, 5.0], [30.0, 31.0], [7.0, 8.0]]
    assert int(result.fp_total) == len(frame)
    frame, centres = false_positive_centres(dets, result, min_score=0.5)       # the 0.3 one was not served
    assert frame.tolist() == [0, 1, 1] and centres.tolist() == [[50.0, 60.0], [5.0, 5.0], [7.0, 8.0]]
    result.pred_label = pred_label[:, :, :2]
    with pytest.raises(ValueError):
        false_positive_centres(dets, result)
    assert "SYNCHRONISES" in false_positive_centres.__doc__


# (5) -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_no_cpu_fallback():
    from unet_nested4tiny_objects_keypoints_amd import Augment, SceneCrops, ops
    from unet_nested4tiny_objects_keypoints_amd.crops import _centre_table
    frames = torch.zeros(2, 40, 40, 1, dtype=torch.uint8)
    labels = torch.tensor([[[3.0, 4.0]], [[5.0, 6.0]]])
    cls = torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="translate"):
        SceneCrops(frames, labels, cls, 2, crop=(16, 16), augment=Augment(translate=(2, 0)))
    with pytest.raises(ValueError, match="square"):
        SceneCrops(frames, labels, cls, 2, crop=(16, 24))
    with pytest.raises(ValueError):
        SceneCrops(frames, labels, cls, 2, crop=(16, 16), p_object=1.5)
    with pytest.raises(ValueError):
        SceneCrops(frames, labels, cls, 2, crop=(16, 16), radius=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SceneCrops(frames, labels, cls, 2, crop=(16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SceneCrops(frames, labels, cls, 2, crop=(16, 24), augment=Augment(rot90=False))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.points_target(labels, cls, torch.zeros(1, dtype=torch.int64), torch.zeros(1, 16), 2, (8, 8), 3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.crops_draw(4, 0, 2, (40, 40), (16, 16), None, None, 0.5, (1, 1), Augment().desc(), "cpu")
    # the centre table: frames outside [0, S) and malformed rows are refused
    frame, xy = _centre_table([0, 1, 1], [[1, 2], [3, 4], [5.5, 6]], 2, "cpu")
    assert frame.dtype == torch.int32 and xy.dtype == torch.float32 and tuple(xy.shape) == (3, 2)
    for bad in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match=r"\[0, 2\)"):
            _centre_table(bad, [[1, 2], [3, 4]], 2, "cpu")
    with pytest.raises(ValueError):
        _centre_table([0], [[1, 2], [3, 4]], 2, "cpu")
    with pytest.raises(ValueError):
        _centre_table([0], [[float("nan"), 2]], 2, "cpu")
    empty = _centre_table([], torch.zeros(0, 2), 2, "cpu")
    assert empty[0].numel() == 0 and tuple(empty[1].shape) == (0, 2)
