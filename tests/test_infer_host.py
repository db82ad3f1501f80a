"""Host side of the inference modes (no GPU): the node selection of a network cut at a head, pruned checkpoints, the
error paths of ``UNet_Nested.infer`` that must fire before any device work, and the C ABI of the ensemble head kernel
(argument checks that never touch the device, descriptor layout against a gcc compile of the header)."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def full_order(d):
    """The order engine._forward_impl has always visited the nodes in: encoder column, then the decoder columns."""
    return [(i, 0) for i in range(d)] + [(i, j) for j in range(1, d) for i in range(d - j)]


def inputs_of(i, j):
    if j == 0:
        return [(i - 1, 0)] if i else []
    return [(i + 1, j - 1)] + [(i, jj) for jj in range(j)]


@pytest.mark.parametrize("d", [2, 3, 4, 5])
def test_needed_nodes(d):
    from unet_nested4tiny_objects_keypoints_amd.engine import needed_nodes
    assert needed_nodes(d, d - 1) == full_order(d)
    for head in range(1, d):
        nodes = needed_nodes(d, head)
        assert len(set(nodes)) == len(nodes)
        assert set(nodes) == {(i, j) for i in range(d) for j in range(d - i) if i + j <= head and j <= head}
        it = iter(full_order(d))
        assert all(n in it for n in nodes), "not a subsequence of the full order"
        for k, (i, j) in enumerate(nodes):
            assert all(src in nodes[:k] for src in inputs_of(i, j)), (i, j)
    for bad in (0, d, -1, True, False, 1.0, "1"):
        with pytest.raises(ValueError):
            needed_nodes(d, bad)


def _numel(state):
    return sum(v.numel() for k, v in state.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))


@pytest.mark.parametrize("ctor,counts", [((1, 4, 1), (101444, 512232, 2207244)), ((), (25924, 128920, 553260))])
def test_pruned_state_dict_keys_and_parameter_counts(ctor, counts):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, count_param
    from unet_nested4tiny_objects_keypoints_amd.checkpoint import pruned_state_dict
    m = UNet_Nested(*ctor)
    full = m.state_dict()
    assert count_param(m) == counts[-1]
    prev = set()
    for head, want in zip((1, 2, 3), counts):
        sd = pruned_state_dict(m, head)
        assert _numel(sd) == want
        assert prev < set(sd) <= set(full)             # nested in head
        assert list(sd) == [k for k in full if k in sd]  # the full dict's order
        assert all(sd[k] is full[k] or torch.equal(sd[k], full[k]) for k in sd)
        prev = set(sd)
    assert list(pruned_state_dict(m, 3)) == list(full)
    with pytest.raises(ValueError):
        pruned_state_dict(m, 4)


def test_load_pruned_round_trip_and_key_checks(tmp_path):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    from unet_nested4tiny_objects_keypoints_amd.checkpoint import load_pruned, pruned_state_dict, save_pruned
    kw = dict(in_channels=1, n_classes=4, feature_scale=8)
    torch.manual_seed(0)
    src = UNet_Nested(**kw)
    torch.manual_seed(1)
    dst = UNet_Nested(**kw)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    assert src.pruned_to is None and dst.pruned_to is None
    path = save_pruned(src, 2, str(tmp_path / "h2.pth"))
    assert load_pruned(dst, path) == 2 and dst.pruned_to == 2
    kept = set(pruned_state_dict(src, 2))
    for k, v in dst.state_dict().items():
        assert torch.equal(v, src.state_dict()[k] if k in kept else before[k]), k
    assert os.path.getsize(path) < os.path.getsize(save_pruned(src, 3, str(tmp_path / "h3.pth")))   # a strict subset
    with pytest.raises(RuntimeError, match="pruned to head 2"):
        dst(torch.randn(1, 1, 16, 16))                       # (before the input checks: nothing here needs a GPU)
    dst.eval()
    with pytest.raises(RuntimeError, match="pruned to head 2"):
        dst.infer(torch.randn(1, 1, 16, 16), 3)
    # one key removed / one key added: an error that names the key
    sd = dict(pruned_state_dict(src, 2))
    gone = sd.pop("up_concat11.up.weight")
    torch.save(sd, str(tmp_path / "short.pth"))
    with pytest.raises(RuntimeError, match="up_concat11.up.weight"):
        load_pruned(UNet_Nested(**kw), str(tmp_path / "short.pth"))
    sd["up_concat11.up.weight"] = gone
    sd["conv30.conv1.0.bias"] = src.state_dict()["conv30.conv1.0.bias"]
    torch.save(sd, str(tmp_path / "long.pth"))
    with pytest.raises(RuntimeError, match="conv30.conv1.0.bias"):
        load_pruned(UNet_Nested(**kw), str(tmp_path / "long.pth"))
    # a full load lifts the restriction; a partial one does not
    dst.load_state_dict(pruned_state_dict(src, 1), strict=False)
    assert dst.pruned_to == 2
    dst.load_state_dict(src.state_dict())
    assert dst.pruned_to is None
    assert load_pruned(dst, str(tmp_path / "h3.pth")) == 3 and dst.pruned_to is None   # every node was loaded


def test_infer_error_paths_without_gpu():
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    m = UNet_Nested(in_channels=1, feature_scale=8)
    x = torch.randn(1, 1, 16, 16)
    for bad in (0, 4, -1, True, 1.0, "2"):
        with pytest.raises(ValueError, match="head"):
            m.infer(x, bad)                     # (whatever the mode and the device: checked first)
    with pytest.raises(RuntimeError, match="eval"):
        m.infer(x, 1)                           # a fresh module is in training mode
    m.eval()
    for kw in (dict(), dict(head=1), dict(head=2, ensemble=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.infer(x, **kw)
    with pytest.raises(ValueError):
        m.infer(torch.randn(1, 16, 16), 1)      # the input checks of forward, in forward's order
    assert m.is_ds is True                      # stored, unused by forward: infer(ensemble=...) is where its meaning lives


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


def test_heads_mean_abi_argument_checks(built_lib):
    L = built_lib
    lib = L.lib()
    assert lib.unetpp_abi_version() == L.ABI_VERSION == 14     # additive entry points: the version stays
    out = ctypes.c_void_p(0x1000)                             # never dereferenced: every call below fails its checks
    for fn in (lib.unetpp_heads_mean_fwd, lib.unetpp_heads_mean_fwd_bf16):
        d = L.HeadsMean()
        for h in range(L.MAX_HEADS):
            d.head[h].x, d.head[h].weight, d.head[h].bias = 0x1000, 0x2000, 0x3000
        ok = (1, 8, 8, 32, 4)
        assert fn(None, *ok, out, None) == -1                 # null descriptor
        for n_heads in (0, -1, L.MAX_HEADS + 1):
            d.n_heads = n_heads
            assert fn(ctypes.byref(d), *ok, out, None) == -1
        d.n_heads = 3
        assert fn(ctypes.byref(d), *ok, None, None) == -1     # null output
        assert fn(ctypes.byref(d), 0, 8, 8, 32, 4, out, None) == -1   # N = 0
        assert fn(ctypes.byref(d), 1, 8, 8, 32, 9, out, None) == -1   # more classes than the head kernels take
        assert fn(ctypes.byref(d), 1, 8, 8, 32, 0, out, None) == -1
        assert fn(ctypes.byref(d), 1, 8, 8, 0, 4, out, None) == -1
        assert fn(ctypes.byref(d), 1, 8, 8, 136, 4, out, None) == -1  # more channels than the head kernels take
        d.head[2].weight = None
        assert fn(ctypes.byref(d), *ok, out, None) == -1      # a null pointer inside the used triples
        d.head[2].weight = 0x2000
        d.head[1].x = None
        assert fn(ctypes.byref(d), *ok, out, None) == -1


def test_heads_mean_descriptor_layout_matches_header(built_lib, tmp_path):
    """sizeof / offsetof from a C compile of the header against the ctypes mirror (as tests/test_abi.py does)."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "unetpp_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(unetpp_head_src), offsetof(unetpp_head_src, weight),'
                   'offsetof(unetpp_head_src, bias), sizeof(unetpp_heads_mean), offsetof(unetpp_heads_mean, head),'
                   'offsetof(unetpp_heads_mean, n_heads), offsetof(unetpp_heads_mean, reserved), UNETPP_MAX_HEADS);'
                   'return 0;}')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    L = built_lib
    want = [ctypes.sizeof(L.HeadSrc), L.HeadSrc.weight.offset, L.HeadSrc.bias.offset, ctypes.sizeof(L.HeadsMean),
            L.HeadsMean.head.offset, L.HeadsMean.n_heads.offset, L.HeadsMean.reserved.offset, L.MAX_HEADS]
    assert got == want
