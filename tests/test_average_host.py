"""CPU checks of weight averaging (averaging.py, csrc/average.hip): the C entry point's argument checks without a GPU,
the segment struct's layout, the constructor contract of WeightAverager, and the node list of the statistics pass."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


def test_abi_version_is_unchanged(built_lib):
    assert built_lib.lib().unetpp_abi_version() == built_lib.ABI_VERSION == 14


def test_entry_point_rejects_bad_arguments(built_lib):
    L = built_lib.lib()
    segs = (built_lib.AvgSegment * 1)()
    cmap = (ctypes.c_int32 * 1)()
    cnt = ctypes.c_float(0)
    hyp = ctypes.c_double(0.5)
    done = ctypes.c_int32(0)
    S, M = ctypes.byref(segs), ctypes.byref(cmap)
    N, H, D = ctypes.byref(cnt), ctypes.byref(hyp), ctypes.byref(done)
    MEAN, EMA, SWAP, CAP = built_lib.AVG_MEAN, built_lib.AVG_EMA, built_lib.AVG_SWAP, built_lib.AVG_CAPTURABLE
    assert (MEAN, EMA, SWAP, CAP) == (0, 1, 2, 1)
    bad = [
        # kind, flags, segments, n_segments, chunk map, n_chunks, count, decay, count_dev, hyper_dev, done
        (MEAN, 0, None, 1, M, 1, 0, 0.0, None, None, None),       # null table
        (MEAN, 0, S, 0, M, 1, 0, 0.0, None, None, None),          # zero segments
        (MEAN, 0, S, -1, M, 1, 0, 0.0, None, None, None),
        (MEAN, 0, S, 1, None, 1, 0, 0.0, None, None, None),       # null chunk map
        (MEAN, 0, S, 1, M, 0, 0, 0.0, None, None, None),          # zero chunks
        (3, 0, S, 1, M, 1, 0, 0.0, None, None, None),             # unknown kind
        (-1, 0, S, 1, M, 1, 0, 0.0, None, None, None),
        (MEAN, 2, S, 1, M, 1, 0, 0.0, None, None, None),          # unknown flag
        (MEAN, 0, S, 1, M, 1, -1, 0.0, None, None, None),         # eager: a negative count
        (MEAN, 0, S, 1, M, 1, 0, 0.0, N, None, None),             # eager takes no device count ...
        (MEAN, 0, S, 1, M, 1, 0, 0.0, None, H, None),             # ... no device decay ...
        (MEAN, 0, S, 1, M, 1, 0, 0.0, None, None, D),             # ... and no arrival counter
        (EMA, 0, S, 1, M, 1, 1, 1.0, None, None, None),           # eager ema: decay outside [0, 1)
        (EMA, 0, S, 1, M, 1, 1, -0.1, None, None, None),
        (EMA, 0, S, 1, M, 1, 1, float("nan"), None, None, None),
        (MEAN, CAP, S, 1, M, 1, 0, 0.0, None, H, D),              # capturable needs the device count ...
        (MEAN, CAP, S, 1, M, 1, 0, 0.0, N, H, None),              # ... and the arrival counter
        (EMA, CAP, S, 1, M, 1, 0, 0.5, N, None, D),               # capturable ema needs the device decay
        (SWAP, CAP, S, 1, M, 1, 0, 0.0, None, None, None),        # a swap has no capturable form
        (SWAP, 0, S, 1, M, 1, 0, 0.0, N, None, None),             # ... and takes no device pointer
        (SWAP, 0, S, 1, M, 1, 0, 0.0, None, H, None),
        (SWAP, 0, S, 1, M, 1, 0, 0.0, None, None, D),
    ]
    for args in bad:
        assert L.unetpp_avg_update(*args, None) == -1, args


def test_segment_layout_matches_header(built_lib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "unetpp_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(unetpp_avg_segment),'
                   'offsetof(unetpp_avg_segment, avg), offsetof(unetpp_avg_segment, src),'
                   'offsetof(unetpp_avg_segment, numel), offsetof(unetpp_avg_segment, chunk_begin),'
                   'offsetof(unetpp_avg_segment, vec), offsetof(unetpp_avg_segment, copy),'
                   'UNETPP_AVG_MEAN, UNETPP_AVG_EMA, UNETPP_AVG_SWAP, UNETPP_AVG_CAPTURABLE);return 0;}')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = built_lib.AvgSegment
    want = [ctypes.sizeof(S), S.avg.offset, S.src.offset, S.numel.offset, S.chunk_begin.offset, S.vec.offset,
            S.copy.offset, built_lib.AVG_MEAN, built_lib.AVG_EMA, built_lib.AVG_SWAP, built_lib.AVG_CAPTURABLE]
    assert got == want
    assert ctypes.sizeof(S) == 40


def test_cpu_model_has_no_fallback(built_lib):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, WeightAverager
    m = UNet_Nested(in_channels=1, n_classes=4, feature_scale=8)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WeightAverager(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WeightAverager(torch.nn.Sequential(torch.nn.Linear(3, 2)), kind="ema")
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


def test_other_dtypes_raise(built_lib):
    from unet_nested4tiny_objects_keypoints_amd import WeightAverager
    with pytest.raises((RuntimeError, TypeError)):
        WeightAverager(torch.nn.Linear(3, 2).double())


@pytest.mark.parametrize("kw", [dict(kind="median"), dict(kind="MEAN"), dict(kind=None), dict(kind=0),
                                dict(kind="ema", decay=1.0), dict(kind="ema", decay=-0.1), dict(decay=1.5),
                                dict(kind="ema", decay=float("nan")), dict(kind="ema", decay="0.9"),
                                dict(kind="ema", decay=True)])
def test_bad_kind_or_decay_is_a_value_error(kw):
    """Raised before anything else is looked at: the model here is on the CPU and would itself be refused."""
    from unet_nested4tiny_objects_keypoints_amd import WeightAverager
    with pytest.raises(ValueError):
        WeightAverager(torch.nn.Linear(3, 2), **kw)


def test_exported_under_a_qualified_name():
    import unet_nested4tiny_objects_keypoints_amd as pkg
    assert "WeightAverager" in pkg.__all__ and pkg.WeightAverager is pkg.averaging.WeightAverager


@pytest.mark.parametrize("depth", [2, 3, 4, 5])
def test_statistics_pass_runs_the_encoder_column_only(depth):
    from unet_nested4tiny_objects_keypoints_amd import engine
    nodes = engine.stats_nodes(depth)
    assert nodes == [(i, 0) for i in range(depth)]
    assert nodes == [n for n in engine.needed_nodes(depth, depth - 1) if n[1] == 0]   # column 0 of the whole graph, top down
    # every BatchNorm layer of the model sits in one of these nodes
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    from unet_nested4tiny_objects_keypoints_amd.unet import BatchNormParams
    m = UNet_Nested(in_channels=1, n_classes=2, feature_scale=8, depth=depth)
    holders = {k.split(".")[0] for k, mod in m.named_modules() if isinstance(mod, BatchNormParams)}
    assert holders == {"conv%d0" % i for i, _ in nodes}
    # a plan phase of its own: neither the whole forward's nor a pruned pass's
    assert engine.STATS_PHASE not in {engine.plan_phase(depth, h) for h in range(1, depth)} | {"bwd"}


def test_checkpoint_keywords_are_additive(tmp_path):
    """A .tar saved without an averager has exactly the reference's keys."""
    from unet_nested4tiny_objects_keypoints_amd import checkpoint
    m = torch.nn.Linear(3, 2)
    path = checkpoint.save_checkpoint(m, None, 2, str(tmp_path / "c.tar"))
    assert list(torch.load(path)) == ["model_state_dict", "optimizer_state_dict", "epoch"]
    assert checkpoint.average_model_name(3, 0.5, 1.5) == "average_epoch_3_heatmaploss_0.5_landmarkloss_1.5.pth"
