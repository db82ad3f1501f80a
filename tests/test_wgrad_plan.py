"""CPU-only: unetpp_wgrad_plan makes the decisions the four places it replaces made (which kernel, n_split, planes per
slab, tile pairs per workgroup).  Planning touches no device memory, so descriptors with made-up pointers do."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


def _view(v, c, c_len=None, hs=0, ws=0, sy=1, sx=1, oy=0, ox=0, fold=False):
    v.ptr = 0x100000   # never dereferenced; 16-byte aligned
    v.C, v.c_off, v.c_len = c, 0, (c if c_len is None else c_len)
    v.Hs, v.Ws, v.sy, v.sx, v.oy, v.ox = hs, ws, sy, sx, oy, ox
    if fold:
        v.scale = v.shift = 0x200000
        v.relu = 1


def _desc(L, n, h, w, taps, xs, dys, flags="", deconv=False, fold=False, x_len=None, dy_gate=False):
    d = L.WgradDesc()
    d.N, d.H, d.W, d.taps, d.n_x, d.n_dy = n, h, w, taps, len(xs), len(dys)
    d.flags = (L.GEMM_BF16 if "bf16" in flags else 0) | (L.GEMM_DIRECT if "direct" in flags else 0)
    for i, c in enumerate(xs):
        _view(d.x[i], c, c_len=x_len, hs=h, ws=w, fold=fold)
    for i, c in enumerate(dys):
        if deconv:   # the four pixel phases of a 2x2 stride-2 transposed convolution
            _view(d.dy[i], c, hs=2 * h, ws=2 * w, sy=2, sx=2, oy=i // 2, ox=i % 2)
        else:
            _view(d.dy[i], c, hs=h, ws=w)
        if dy_gate:
            d.dy[i].gate = 0x300000
    return d


# (id, _desc arguments, n_split at target_blocks 256 / 3 / 4096, pairs_per_workgroup, planes, label)
PARENT = [
    ("first-layer-cin1", dict(n=32, h=256, w=256, taps=9, xs=[1], dys=[32]), (1024, 1024, 1024), 1, 9, "small_cin_wgrad_kernel"),
    ("first-layer-cin3-bf16", dict(n=8, h=512, w=512, taps=9, xs=[3], dys=[64], flags="bf16"), (512, 512, 512), 1, 9,
     "small_cin_wgrad_kernel"),
    ("1x1-cin4", dict(n=2, h=32, w=32, taps=1, xs=[4], dys=[32]), (8, 8, 8), 1, 1, "wgrad_dma_kernel<1>"),
    ("1x1-cin4-large", dict(n=32, h=256, w=256, taps=1, xs=[4], dys=[32]), (1024, 1024, 1024), 1, 1, "wgrad_dma_kernel<1>"),
    ("3x3-C8-slice-of-4", dict(n=32, h=256, w=256, taps=9, xs=[8], dys=[32], x_len=4), (256, 3, 4096), 1, 9, "wgrad_dma_kernel<9>"),
    ("wino-32-32", dict(n=32, h=256, w=256, taps=9, xs=[32], dys=[32]), (256, 3, 4096), 1, 16, "wgrad_wino_kernel"),
    ("wino-fold", dict(n=32, h=256, w=256, taps=9, xs=[32], dys=[32], fold=True), (256, 3, 4096), 1, 16, "wgrad_wino_kernel"),
    ("wino-32+32+32-32", dict(n=32, h=256, w=256, taps=9, xs=[32, 32, 32], dys=[32]), (85, 1, 1365), 1, 16, "wgrad_wino_kernel"),
    ("direct-32-32", dict(n=32, h=256, w=256, taps=9, xs=[32], dys=[32], flags="direct"), (256, 3, 4096), 1, 9, "wgrad_dma_kernel<9>"),
    ("fold-direct-32-32", dict(n=32, h=256, w=256, taps=9, xs=[32], dys=[32], flags="direct", fold=True), (256, 3, 4096), 1, 9,
     "wgrad_fast_kernel<9>"),
    ("dy-relu-gate", dict(n=32, h=256, w=256, taps=9, xs=[32], dys=[32], dy_gate=True), (256, 3, 4096), 1, 9, "wgrad_kernel<9>"),
    ("unaligned-30-32", dict(n=32, h=256, w=256, taps=9, xs=[30], dys=[32]), (256, 3, 4096), 1, 9, "wgrad_kernel<9>"),
    ("16-wide-256-256", dict(n=32, h=16, w=16, taps=9, xs=[256], dys=[256]), (4, 1, 32), 1, 9, "wgrad_dma_kernel<9>"),
    ("16x16-512-512", dict(n=32, h=16, w=16, taps=9, xs=[512], dys=[512]), (1, 1, 16), 1, 9, "wgrad_dma_kernel<9>"),
    ("deconv-pw-64-4x32", dict(n=32, h=128, w=128, taps=1, xs=[64], dys=[32] * 4, deconv=True), (256, 3, 2048), 8, 1, "wgrad_pw_kernel"),
    ("deconv-pw-512-4x256", dict(n=32, h=16, w=16, taps=1, xs=[512], dys=[256] * 4, deconv=True), (4, 1, 32), 8, 1, "wgrad_pw_kernel"),
    ("deconv-64-4x16", dict(n=1, h=8, w=8, taps=1, xs=[64], dys=[16] * 4, deconv=True), (1, 1, 1), 1, 1, "wgrad_dma_kernel<1>"),
    ("1x1-64-32", dict(n=2, h=64, w=64, taps=1, xs=[64], dys=[32]), (32, 1, 32), 1, 1, "wgrad_dma_kernel<1>"),
    ("bf16-pair-32-32", dict(n=8, h=512, w=512, taps=9, xs=[32], dys=[32], flags="bf16"), (512, 3, 4096), 1, 9, "wgrad_bf16_kernel<9>"),
    ("bf16-quad-64-64", dict(n=8, h=256, w=256, taps=9, xs=[64], dys=[64], flags="bf16"), (256, 3, 2048), 4, 9,
     "wgrad_bf16_quad_kernel<9>"),
    ("bf16-quad-128+64-64", dict(n=8, h=256, w=256, taps=9, xs=[128, 64], dys=[64], flags="bf16"), (85, 1, 1365), 4, 9,
     "wgrad_bf16_quad_kernel<9>"),
    ("bf16-96+64-64", dict(n=8, h=256, w=256, taps=9, xs=[96, 64], dys=[64], flags="bf16"), (51, 1, 409), 1, 9, "wgrad_bf16_kernel<9>"),
    ("bf16-deconv-128-4x64", dict(n=8, h=128, w=128, taps=1, xs=[128], dys=[64] * 4, flags="bf16", deconv=True), (32, 1, 512), 4, 1,
     "wgrad_bf16_quad_kernel<1>"),
    ("tiny-1x8x8", dict(n=1, h=8, w=8, taps=9, xs=[8], dys=[8]), (1, 1, 1), 1, 9, "wgrad_dma_kernel<9>"),
]


def _plan(L, d, target):
    out = L.WgradSizes()
    assert L.lib().unetpp_wgrad_plan(ctypes.byref(d), target, ctypes.byref(out)) == 0
    return out


@pytest.mark.parametrize("case,args,splits,pairs_per_workgroup,planes,label", PARENT, ids=[c[0] for c in PARENT])
def test_plan_matches_the_decisions_before_it(L, case, args, splits, pairs_per_workgroup, planes, label):
    """n_split, pairs_per_workgroup and planes are RECORDED from the library of commit 83ca35a, the last one that
    decided them in four places: its ops.wgrad formula was evaluated on the CPU (no device: 0 / 0 CUs, so without the
    CU scaling, which tests/test_gpu_persistent.py covers) through its unetpp_wgrad_pairs_per_workgroup,
    unetpp_wgrad_max_split and unetpp_wgrad_slab_planes for these descriptors at target_blocks 256, 3 and 4096.  The
    labels could not be recorded without launching; they are what that commit's cascade of launchers gives when read
    by hand, and the GPU tests see each of them running."""
    d = _desc(L, **args)
    k = sum(d.x[i].c_len for i in range(d.n_x))
    ncols = sum(d.dy[i].c_len for i in range(d.n_dy))
    default = _plan(L, d, 0)
    for target, split in zip((256, 3, 4096), splits):
        p = _plan(L, d, target)
        assert (p.n_split, p.pairs_per_workgroup, p.planes) == (split, pairs_per_workgroup, planes), (case, target)
        assert p.kernel.decode() == label, (case, target)
        assert p.slab_floats == split * (planes * k + 1) * ncols
    assert (default.n_split, default.kernel) == (splits[0], label.encode())   # target_blocks <= 0: 256


def test_plain_image_of_2gib_is_planned_as_the_direct_sum_that_runs(L):
    """The one intended difference from commit 83ca35a.  There unetpp_wgrad_slab_planes answered 16 (Winograd) for
    1 x 4096 x 4096, 32 -> 32, plain views, while the Winograd launcher handed such a launch (an image of 2 GiB, beyond
    its per-image buffer resources) to a direct-sum kernel that writes 9-plane slabs.  The plan and the launch now share
    one selection: 9 planes, a direct-sum label, the same n_split as before (256 / 3 / 4096, recorded as above)."""
    d = _desc(L, n=1, h=4096, w=4096, taps=9, xs=[32], dys=[32])
    for target, split in zip((256, 3, 4096), (256, 3, 4096)):
        p = _plan(L, d, target)
        assert (p.n_split, p.pairs_per_workgroup, p.planes) == (split, 1, 9)
        assert p.kernel == b"wgrad_dma_kernel<9>"
    d = _desc(L, n=1, h=4096, w=4096, taps=9, xs=[32], dys=[32], fold=True)   # folded views: still the Winograd kernel
    assert (_plan(L, d, 256).planes, _plan(L, d, 256).kernel) == (16, b"wgrad_wino_kernel")


def test_small_wgrad_blocks_is_a_switch_of_the_library(L):
    """UNETPP_SMALL_WGRAD_BLOCKS was read by the Python layer; it is a row of the library's switch table now."""
    first = _desc(L, n=32, h=256, w=256, taps=9, xs=[1], dys=[32])
    other = _desc(L, n=32, h=256, w=256, taps=9, xs=[32], dys=[32])
    with L.debug_switch("SMALL_WGRAD_BLOCKS", 2048):
        assert _plan(L, first, 256).n_split == 2048
        assert _plan(L, other, 256).n_split == 256
    assert _plan(L, first, 256).n_split == 1024
    text = open(L.INCLUDE + "/unetpp_hip.h").read()
    assert "SMALL_WGRAD_BLOCKS" in text[text.index("Dispatcher switches"):text.index("int unetpp_debug_set")]


def test_plan_refuses_what_the_launch_refuses(L):
    lib = L.lib()
    out = L.WgradSizes()
    good = _desc(L, n=2, h=32, w=32, taps=9, xs=[32], dys=[32])
    assert lib.unetpp_wgrad_plan(None, 256, ctypes.byref(out)) == -1
    assert lib.unetpp_wgrad_plan(ctypes.byref(good), 256, None) == -1
    assert lib.unetpp_wgrad_plan(ctypes.byref(good), 256, ctypes.byref(out)) == 0
    for change in (lambda d: setattr(d, "taps", 4), lambda d: setattr(d, "n_x", 0), lambda d: setattr(d, "N", 0),
                   lambda d: setattr(d.x[0], "ptr", None), lambda d: setattr(d.dy[0], "Hs", 16),
                   lambda d: setattr(d.x[0], "c_len", 64)):
        d = _desc(L, n=2, h=32, w=32, taps=9, xs=[32], dys=[32])
        change(d)
        assert lib.unetpp_wgrad_plan(ctypes.byref(d), 256, ctypes.byref(out)) == -1
        d.n_split, d.slabs = 1, 0x400000
        assert lib.unetpp_wgrad(ctypes.byref(d), None) == -1
    bf = _desc(L, n=2, h=32, w=32, taps=9, xs=[36], dys=[32], flags="bf16")   # bf16 views are 8-channel aligned
    assert lib.unetpp_wgrad_plan(ctypes.byref(bf), 256, ctypes.byref(out)) == -1
    good.n_split, good.slabs = out.n_split, None                              # the launch itself needs slabs and a split
    assert lib.unetpp_wgrad(ctypes.byref(good), None) == -1
    good.n_split, good.slabs = 0, 0x400000
    assert lib.unetpp_wgrad(ctypes.byref(good), None) == -1
    good.n_split = 9                                                          # 2 x 32 x 32: 8 pixel tiles
    assert lib.unetpp_wgrad(ctypes.byref(good), None) == -1
