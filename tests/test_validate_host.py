"""CPU checks of the validation step (validate.py, csrc/validate.hip): exports, no CPU fallback, the host-side
ValueErrors raised before anything is launched, and the matcher's C entry point rejecting bad arguments without a GPU."""
import pytest
import torch

PATTERN = [[0], [1, 2, 3], [4], [5, 6]]


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


@pytest.fixture
def no_launch(monkeypatch):
    """every device-side entry point of the validation path fails the test if it is reached"""
    from unet_nested4tiny_objects_keypoints_amd import ops

    def launched(*a, **k):
        raise AssertionError("a launch was reached before the host-side checks")
    for name in ("heatmap_pattern", "focal_bce_heads", "focal_bce", "keypoints_extract", "match_points"):
        monkeypatch.setattr(ops, name, launched)


def _model(n_classes=4):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    return UNet_Nested(in_channels=1, n_classes=n_classes, feature_scale=8).eval()


def _heads(n=2, c=4, h=32, w=32, k=3):
    return tuple(torch.rand(n, c, h, w) for _ in range(k))


def test_exports():
    import unet_nested4tiny_objects_keypoints_amd as pkg
    from unet_nested4tiny_objects_keypoints_amd import Heatmap
    assert "validate_step" in pkg.__all__ and "validate_outputs" in pkg.__all__
    assert callable(pkg.validate_step) and callable(pkg.validate_outputs)
    assert callable(Heatmap.match_points) and callable(Heatmap.match_distmin)


def test_cpu_tensors_have_no_fallback(no_launch):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, Heatmap, validate_outputs, validate_step
    hm, crit = Heatmap(PATTERN, 32, 32), FocalLoss_BCE_2d()
    labels = torch.rand(2, 7, 2) * 31
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        validate_step(_model(), crit, hm, torch.randn(2, 1, 32, 32), labels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        validate_outputs(_heads(), crit, hm, labels)


def test_training_mode_is_refused(no_launch):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, Heatmap, validate_step
    with pytest.raises(RuntimeError, match="eval"):
        validate_step(_model().train(), FocalLoss_BCE_2d(), Heatmap(PATTERN, 32, 32), torch.randn(2, 1, 32, 32),
                      torch.rand(2, 7, 2))


@pytest.mark.parametrize("case", ["index_beyond_labels", "map_over_64", "class_count", "map_size", "batch"])
def test_host_side_value_errors_come_before_any_launch(no_launch, case):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, Heatmap, validate_outputs, validate_step
    crit = FocalLoss_BCE_2d()
    pattern, h, w, s, n_classes, n_labels_batch = PATTERN, 32, 32, 7, 4, 2
    heads = _heads()
    if case == "index_beyond_labels":
        s = 6                                   # pattern index 6 >= S
    elif case == "map_over_64":
        pattern = [list(range(65)), [65], [66], [67]]
        s = 68
    elif case == "class_count":
        n_classes = 3
        heads = _heads(c=3)
    elif case == "map_size":
        h = 40
    else:
        n_labels_batch = 3
    hm = Heatmap(pattern, w, h)
    labels = torch.rand(n_labels_batch, s, 2) * 31
    with pytest.raises(ValueError):
        validate_step(_model(n_classes), crit, hm, torch.randn(2, 1, 32, 32), labels)
    with pytest.raises(ValueError):
        validate_outputs(heads, crit, hm, labels)


def test_matcher_limits_on_the_host(no_launch):
    from unet_nested4tiny_objects_keypoints_amd import Heatmap, ops
    with pytest.raises(ValueError, match="at most 64"):
        ops.check_match_pattern([list(range(65))], 65)
    with pytest.raises(ValueError, match="twice"):
        ops.check_match_pattern([[0, 1], [1]], 3)
    with pytest.raises(ValueError, match="labels 0..2"):
        ops.check_match_pattern([[0, 3]], 3)
    ops.check_match_pattern([list(range(64))], 64)
    hm = Heatmap([[0, 1]], 16, 16)
    with pytest.raises(ValueError):
        hm.match_distmin([[1, 1]] * 65, [[0, 0], [1, 1]], [0, 1])
    with pytest.raises(ValueError):
        hm.match_distmin([[1, 1]], [[0, 0], [1, 1]], [0, 2])


def test_match_points_entry_point_rejects_bad_arguments(built_lib):
    lib = built_lib.lib()
    host = torch.zeros(64)
    buf = host.data_ptr()   # host memory: never touched, every call below is rejected before a launch
    args = [buf, buf, 1, 2, 4, 3, buf, 7, buf, buf, buf, buf, buf, buf, None]
    for i in range(9):                       # every pointer but the stream is required
        a = list(args)
        a[[0, 1, 6, 8, 9, 10, 11, 12, 13][i]] = None
        assert lib.unetpp_match_points(*a) == -1
    for pos, bad in ((2, 0), (3, 0), (4, 0), (5, 0), (5, 65), (7, 0)):   # heads, N, C, K (1..64), S
        a = list(args)
        a[pos] = bad
        assert lib.unetpp_match_points(*a) == -1
