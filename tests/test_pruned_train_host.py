"""Host side of training the network cut at a head (no GPU): the gradient-ready order and the parameter set of a cut, the
error paths of ``UNet_Nested.forward_pruned`` that fire before any device work, the C ABI of the ensemble mean's backward
(argument checks that never touch the device, descriptor layout against a gcc compile of the header), head_select's
answers for the new operation against its rules restated here, and the flat gradient buffer of a cut's data-parallel
averager over gloo."""
import ctypes
import os
import socket
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unet_nested4tiny_objects_keypoints_amd", "csrc")


# ------------------------------------------------------------------------------------------------ ordering
@pytest.mark.parametrize("depth", [3, 4, 5])
@pytest.mark.parametrize("is_deconv", [True, False])
@pytest.mark.parametrize("is_batchnorm", [True, False])
def test_ready_order_of_a_cut_is_the_full_order_restricted_to_it(depth, is_deconv, is_batchnorm):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, dp
    from unet_nested4tiny_objects_keypoints_amd.checkpoint import _pruned_prefixes
    from unet_nested4tiny_objects_keypoints_amd.engine import pruned_parameters
    assert pkg.pruned_parameters is pruned_parameters          # re-exported from the package
    m = UNet_Nested(in_channels=1, n_classes=2, feature_scale=8, is_deconv=is_deconv, is_batchnorm=is_batchnorm, depth=depth)
    name_of = {id(p): k for k, p in m.named_parameters()}
    full = dp.ready_order(m)
    assert [id(p) for p in dp.ready_order(m, head=None)] == [id(p) for p in full]
    for head in range(1, depth):
        prefixes = _pruned_prefixes(depth, head)
        want = [name_of[id(p)] for p in full if name_of[id(p)].startswith(prefixes)]
        got = [name_of[id(p)] for p in dp.ready_order(m, head=head)]
        assert got == want, head
        groups = dp.ready_groups(m, head=head)
        assert [name_of[id(p)] for grp in groups for p in grp] == want
        assert len(groups[0]) == 2 * head                     # every head of the cut is reported by the first flush
        inside = [name_of[id(p)] for p in pruned_parameters(m, head)]
        assert inside == [k for k, _ in m.named_parameters() if k.startswith(prefixes)]     # state_dict order
        assert inside == [k for k in m.state_dict() if k in set(inside)]
        assert sorted(inside) == sorted(want)
    assert [id(p) for p in pruned_parameters(m, depth - 1)] == [id(p) for p in m.parameters()]
    assert [id(p) for p in pruned_parameters(m)] == [id(p) for p in m.parameters()]
    for bad in (0, depth, True, 1.0):
        with pytest.raises(ValueError, match="head"):
            dp.ready_order(m, head=bad)
        with pytest.raises(ValueError, match="head"):
            pruned_parameters(m, bad)


# ------------------------------------------------------------------------------------------------ error paths
def test_forward_pruned_error_paths_without_gpu():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet_Nested, train_step
    m = UNet_Nested(in_channels=1, feature_scale=8)
    x = torch.randn(1, 1, 16, 16)
    for bad in (0, 4, -1, True, 1.0, "2"):
        with pytest.raises(ValueError, match="head"):
            m.forward_pruned(x, bad)                        # whatever the mode and the device: checked first
    assert m.training and m.drop_out.training and m.drop_out.p > 0
    with pytest.raises(RuntimeError, match=r"model\.drop_out\.eval\(\)"):
        m.forward_pruned(x, 2, ensemble=True)               # the mean kernel has no dropout
    m.drop_out.eval()
    for kw in (dict(), dict(head=1), dict(head=2, ensemble=True)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.forward_pruned(x, **kw)                       # past the argument checks: the input checks of forward
    with pytest.raises(ValueError):
        m.forward_pruned(torch.randn(1, 16, 16), 1)
    m.pruned_to = 1                                         # what checkpoint.load_pruned records
    for head in (2, 3, None):
        with pytest.raises(RuntimeError, match="pruned to head 1"):
            m.forward_pruned(x, head)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_pruned(x, 1)                              # head <= pruned_to is the supported way to train it
    with pytest.raises(RuntimeError, match="pruned to head 1"):
        m(x)                                                # forward() keeps refusing
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    with pytest.raises(RuntimeError, match="pruned to head 1"):
        train_step(m, opt, FocalLoss_BCE_2d(gamma=3, size_average=False), x, torch.rand(1, 4, 16, 16), head=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        train_step(m, opt, FocalLoss_BCE_2d(gamma=3, size_average=False), x, torch.rand(1, 4, 16, 16), head=1)


def test_load_pruned_docstring_names_the_training_entry_points():
    from unet_nested4tiny_objects_keypoints_amd.checkpoint import load_pruned
    assert "forward_pruned" in load_pruned.__doc__ and "train_step" in load_pruned.__doc__


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


def _descriptors(L, n_heads):
    d, g = L.HeadsMean(), L.HeadsMeanGrad()
    for h in range(L.MAX_HEADS):                              # never dereferenced: every call below fails its checks
        d.head[h].x, d.head[h].weight, d.head[h].bias = 0x1000, 0x2000, 0x3000
        g.head[h].dx, g.head[h].partial = 0x4000, 0x5000
    d.n_heads = g.n_heads = n_heads
    return d, g


def test_heads_mean_bwd_abi_argument_checks(built_lib):
    L = built_lib
    lib = L.lib()
    assert lib.unetpp_abi_version() == L.ABI_VERSION == 14     # additive entry points: the version stays
    d_out = ctypes.c_void_p(0x6000)
    ok = (1, 8, 8, 32, 4)
    for fn in (lib.unetpp_heads_mean_bwd, lib.unetpp_heads_mean_bwd_bf16):
        d, g = _descriptors(L, 3)
        assert fn(None, ctypes.byref(g), d_out, *ok, None) == -1              # null descriptors, null gradient
        assert fn(ctypes.byref(d), None, d_out, *ok, None) == -1
        assert fn(ctypes.byref(d), ctypes.byref(g), None, *ok, None) == -1
        for n_heads in (0, 9, -1):
            d.n_heads = g.n_heads = n_heads
            assert fn(ctypes.byref(d), ctypes.byref(g), d_out, *ok, None) == -1
        d.n_heads, g.n_heads = 3, 2                                              # the two descriptors disagree
        assert fn(ctypes.byref(d), ctypes.byref(g), d_out, *ok, None) == -1
        d.n_heads = g.n_heads = 3
        assert fn(ctypes.byref(d), ctypes.byref(g), d_out, 1, 8, 8, 136, 4, None) == -1   # C > 128
        assert fn(ctypes.byref(d), ctypes.byref(g), d_out, 1, 8, 8, 0, 4, None) == -1
        assert fn(ctypes.byref(d), ctypes.byref(g), d_out, 1, 8, 8, 32, 0, None) == -1    # n_cls of 0 and 9
        assert fn(ctypes.byref(d), ctypes.byref(g), d_out, 1, 8, 8, 32, 9, None) == -1
        assert fn(ctypes.byref(d), ctypes.byref(g), d_out, 0, 8, 8, 32, 4, None) == -1
        for role in ("x", "weight", "bias"):                                     # a null pointer inside the used entries
            setattr(d.head[2], role, None)
            assert fn(ctypes.byref(d), ctypes.byref(g), d_out, *ok, None) == -1, role
            setattr(d.head[2], role, 0x1000)
        for role in ("dx", "partial"):
            setattr(g.head[1], role, None)
            assert fn(ctypes.byref(d), ctypes.byref(g), d_out, *ok, None) == -1, role
            setattr(g.head[1], role, 0x4000)
    # what unetpp_head_bwd_bf16 refuses for one head is refused here: channel counts off 8 * 2^k, misaligned x or dx
    fn = lib.unetpp_heads_mean_bwd_bf16
    d, g = _descriptors(L, 2)
    for c in (4, 12, 24, 36):
        assert fn(ctypes.byref(d), ctypes.byref(g), d_out, 1, 8, 8, c, 4, None) == -1, c
    d.head[1].x = 0x1008
    assert fn(ctypes.byref(d), ctypes.byref(g), d_out, *ok, None) == -1
    d.head[1].x = 0x1000
    g.head[0].dx = 0x4002
    assert fn(ctypes.byref(d), ctypes.byref(g), d_out, *ok, None) == -1


def test_heads_mean_grad_descriptor_layout_matches_header(built_lib, tmp_path):
    """sizeof / offsetof from a C compile of the header against the ctypes mirror (as tests/test_infer_host.py does)."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "unetpp_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(unetpp_head_grad), offsetof(unetpp_head_grad, partial),'
                   'offsetof(unetpp_head_grad, accumulate), offsetof(unetpp_head_grad, gate_x), sizeof(unetpp_heads_mean_grad),'
                   'offsetof(unetpp_heads_mean_grad, head), offsetof(unetpp_heads_mean_grad, n_heads),'
                   'offsetof(unetpp_heads_mean_grad, reserved), UNETPP_MAX_HEADS);'
                   'return 0;}')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    L = built_lib
    want = [ctypes.sizeof(L.HeadGrad), L.HeadGrad.partial.offset, L.HeadGrad.accumulate.offset, L.HeadGrad.gate_x.offset,
            ctypes.sizeof(L.HeadsMeanGrad), L.HeadsMeanGrad.head.offset, L.HeadsMeanGrad.n_heads.offset,
            L.HeadsMeanGrad.reserved.offset, L.MAX_HEADS]
    assert got == want
    assert "unetpp_heads_mean_bwd" in L.SIGNATURES and "unetpp_heads_mean_bwd_bf16" in L.SIGNATURES


# ------------------------------------------------------------------------------------------------ head_select
OK, EINVAL = 0, -1
MEAN_BWD = 3                  # HeadOp HEADS_MEAN_BWD: the driver casts any integer to HeadOp
MAX_C, MAX_CLS, MAX_HEADS = 128, 8, 8
LIMIT = 0x7fffffff
REFUSED = ("-", 0, 0, 0, 0)


def cdiv(a, b):
    return -(-a // b)


def pow2(v):
    return v > 0 and v & (v - 1) == 0


def a16(lo):
    return lo & 15 == 0


def mean_bwd_rule(q):
    """The new operation's rules: the argument limits of the head kernels and of the mean, no dropout; bf16 takes what
    unetpp_head_bwd_bf16 takes for one head (octets, aligned x and dx, pixels counted in 32 bits), fp32 everything -- in
    16-byte pieces where the rows and the pointers allow.  Grid and partial rows are unetpp_head_bwd_blocks; the LDS holds
    the x tile [64][C+1], dlogit [64][8], W [8][C] and the two halves of the weight-gradient rows."""
    if not (q["N"] >= 1 and q["H"] >= 1 and q["W"] >= 1 and 1 <= q["C"] <= MAX_C and 1 <= q["n_cls"] <= MAX_CLS and
            1 <= q["heads"] <= MAX_HEADS and q["p"] == 0.0):
        return EINVAL, REFUSED
    pixels, c, k = q["N"] * q["H"] * q["W"], q["C"], q["n_cls"]
    grid = min(cdiv(pixels, 64), 4096)
    lds = (64 * (c + 1) + 64 * MAX_CLS + MAX_CLS * c + 2 * k * c) * 4
    if q["bf16"]:
        if not (c % 8 == 0 and pow2(c >> 3) and a16(q["x"]) and a16(q["dx"]) and pixels < LIMIT):
            return EINVAL, REFUSED
        return OK, ("heads_mean_bwd_bf16", grid, 256, lds, 0)
    if c % 4 == 0 and a16(q["x"]) and a16(q["dx"]):
        return OK, ("heads_mean_bwd_vec", grid, 256, lds, 0)
    return OK, ("heads_mean_bwd", grid, 256, lds, 0)


def _query(bf16, c, k, pixels=65, heads=3, p=0.0, mask=0, x=0, w=0, dx=0, mask_lo=0, wgs=4, cus=256, n=1, h=1):
    return dict(op=MEAN_BWD, bf16=bf16, N=n, H=h, W=pixels, C=c, n_cls=k, heads=heads, p=p, mask=mask, x=x, w=w, dx=dx,
                mask_lo=mask_lo, wgs=wgs, cus=cus)


def _queries():
    qs = []
    for bf16 in (0, 1):
        for c in (3, 4, 8, 12, 16, 20, 32, 64, 128, 132, 256):
            for k in range(10):
                for pixels in (1, 63, 64, 65, 4096 * 64 + 1, LIMIT - 1, LIMIT):
                    qs.append(_query(bf16, c, k, pixels))
            for k in (1, 5, 8):
                for role in (dict(x=4), dict(x=8), dict(x=2), dict(w=4), dict(dx=4), dict(dx=8), dict(mask_lo=1)):
                    qs.append(_query(bf16, c, k, **role))
            for cus in (0, 8, 256):                        # no device is asked: the CU count must not matter
                for wgs in (0, 4):
                    qs.append(_query(bf16, c, 5, cus=cus, wgs=wgs))
        for bad in (dict(n=0), dict(h=0), dict(pixels=0), dict(p=0.4), dict(p=1.0), dict(p=-0.25), dict(heads=0),
                    dict(heads=9), dict(heads=8), dict(heads=1), dict(p=0.4, mask=1)):
            qs.append(_query(bf16, 32, 5, **bad))
    return qs


def _line(q):
    return "%d %d %d %d %d %d %d %d %.9g %d %d %d %d %d %d %d" % (
        q["op"], q["bf16"], q["N"], q["H"], q["W"], q["C"], q["n_cls"], q["heads"], q["p"], q["mask"], q["x"], q["w"],
        q["dx"], q["mask_lo"], q["wgs"], q["cus"])


def test_head_select_answers_for_the_mean_backward(tmp_path):
    exe = str(tmp_path / "head_select_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "head_select_main.cpp"), "-o", exe], check=True)
    qs = _queries()
    out = subprocess.run([exe], input="\n".join(_line(q) for q in qs) + "\n", capture_output=True, text=True,
                         check=True).stdout.splitlines()
    assert len(out) == len(qs)
    seen = set()
    for q, got in zip(qs, out):
        rc, (label, grid, block, lds, active) = mean_bwd_rule(q)
        want = "%d %s %d %d %d %d" % (rc, label, grid, block, lds, active)
        assert got == want, (_line(q), got, want)
        seen.add((q["bf16"], rc, label))
    assert {s[2] for s in seen} == {"-", "heads_mean_bwd", "heads_mean_bwd_vec", "heads_mean_bwd_bf16"}
    assert all((bf16, EINVAL, "-") in seen for bf16 in (0, 1))


# ------------------------------------------------------------------------------------------------ data parallel (gloo)
CTOR = dict(in_channels=1, n_classes=2, feature_scale=8)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, out_dir):
    """No kernel runs: the gradients a cut backward would report are written into the averager's flat buffer by hand, in
    the groups and the order dp.ready_groups(model, head) names."""
    import torch.distributed as dist

    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, dp
    from unet_nested4tiny_objects_keypoints_amd.engine import pruned_parameters
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(40 + rank)
        m = UNet_Nested(**CTOR)
        head = 2
        avg = dp.make_data_parallel(m, bucket_bytes=4 << 10, head=head)
        inside = pruned_parameters(m, head)
        assert avg.flat.numel() == sum(p.numel() for p in inside)
        assert [id(p) for p in avg.params] == [id(p) for p in dp.ready_order(m, head=head)]
        assert m._grad_head == head
        g = torch.Generator().manual_seed(500 + rank)
        mine = {}
        for grp in dp.ready_groups(m, head=head):
            fresh = []
            for p in grp:
                buf = m._grad_alloc(p)
                buf.copy_(torch.randn(p.shape, generator=g))
                mine[id(p)] = buf.clone()
                fresh.append((p, buf))
            m._grad_sink(fresh)
        assert m._grad_done() is True
        names = {id(p): k for k, p in m.named_parameters()}
        torch.save({"mine": {names[i]: v for i, v in mine.items()},
                    "delivered": {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()},
                    "buckets": list(avg.buckets_last_step), "flat": avg.flat.numel(),
                    "params": {k: p.detach().clone() for k, p in m.named_parameters()}},
                   os.path.join(out_dir, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_cut_averager_over_gloo_world_of_two(tmp_path):
    import torch.multiprocessing as mp

    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    from unet_nested4tiny_objects_keypoints_amd.checkpoint import _pruned_prefixes
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    prefixes = _pruned_prefixes(4, 2)
    m = UNet_Nested(**CTOR)
    inside = [k for k, _ in m.named_parameters() if k.startswith(prefixes)]
    assert r0["flat"] == sum(p.numel() for k, p in m.named_parameters() if k in set(inside))
    assert len(r0["buckets"]) >= 2 and r0["buckets"][0][0] == 0 and r0["buckets"][-1][1] == r0["flat"]
    for k, _ in m.named_parameters():
        assert torch.equal(r0["params"][k], r1["params"][k]), k              # the broadcast covers the whole model
        if k in set(inside):
            want = (r0["mine"][k] + r1["mine"][k]) / 2
            for r in (r0, r1):
                assert torch.allclose(r["delivered"][k], want, rtol=0, atol=1e-6), k
        else:
            assert r0["delivered"][k] is None and r1["delivered"][k] is None, k   # outside the cut: no gradient
