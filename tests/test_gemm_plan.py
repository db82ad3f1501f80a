"""CPU-only: unetpp_gemm_plan makes the decisions the forward / input-gradient GEMM made in four places before it
(which kernel and form, grid, workgroup size, weight-image size, rows of an attached BatchNorm finalize).  Planning
touches no device memory, so descriptors with made-up pointers do.

The expected values in tests/golden/gemm_plan_parent.json are RECORDED from the library of commit d52c49d, the last
one whose launchers decided for themselves: every row of CASES was launched once on an MI355X (256 usable CUs, and 8
through unetpp_set_reserved_cus(248)) at its real shape with real device memory, alone and under every switch of
SWITCHES; the label is that library's unetpp_last_kernel_name() after the launch, workgroups / threads are the grid and
workgroup size of the launch in a rocprofv3 kernel trace of that run, image_floats is its
unetpp_gemm_weight_image_floats(), and stats_rows counts the rows of a poisoned stats_partial buffer the launch wrote
(what the attached finalize has to read).  A row that differs from the record means the selection is wrong."""
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_parent.json")

# (switch, value) pairs every row is also planned under
SWITCHES = [("BF16_NO_DMA", 1), ("BF16_DMA_FORM", 0), ("BF16_DMA_FORM", 4), ("BF16_DMA_FORM", 8), ("BF16_DMA_SMALL", 0),
            ("BF16_DMA_STATS", 0), ("BF16_DMA_POINTWISE", 0), ("PW_DIRECT", 0), ("WINO_NO_LEAN", 1)]


def V(c, c_len=None, c_off=0, up=1, oy=0, ox=0, fold=False, gate=False, relu=False, accumulate=False):
    """a view: channels [c_off, c_off + c_len) of a tensor with c channels and up x the launch's rows and columns"""
    return dict(c=c, c_len=c if c_len is None else c_len, c_off=c_off, up=up, oy=oy, ox=ox, fold=fold, gate=gate,
                relu=relu, accumulate=accumulate)


def phases(c, **kw):
    """the four pixel phases of a 2x2 stride-2 transposed convolution"""
    return [V(c, up=2, oy=i // 2, ox=i % 2, **kw) for i in range(4)]


# id -> arguments of desc()
CASES = {
    # fp32 with a weight image
    "wino-32-32": dict(n=2, h=16, w=16, taps=9, ins=[V(32)], outs=[V(32)]),
    "wino-32-32-w32": dict(n=2, h=32, w=32, taps=9, ins=[V(32)], outs=[V(32)]),
    "wino-fold": dict(n=2, h=16, w=16, taps=9, ins=[V(32, fold=True)], outs=[V(32)]),
    "wino-strided": dict(n=2, h=16, w=16, taps=9, ins=[V(64, c_len=32, c_off=32, up=2, oy=1)], outs=[V(32)]),
    "wino-narrow": dict(n=2, h=16, w=16, taps=9, ins=[V(32)], outs=[V(16)]),
    "wino-64+32-64": dict(n=2, h=8, w=8, taps=9, ins=[V(64), V(32)], outs=[V(64)]),
    "wino-stats-bn": dict(n=16, h=64, w=256, taps=9, ins=[V(32)], outs=[V(32)], stats=True, bn=True),
    "wino-strided-stats-bn": dict(n=2, h=16, w=16, taps=9, ins=[V(32, up=2)], outs=[V(32)], stats=True, bn=True),
    "wino-cin4-image": dict(n=2, h=16, w=16, taps=9, ins=[V(4)], outs=[V(32)]),
    "direct-32-32": dict(n=2, h=16, w=16, taps=9, ins=[V(32)], outs=[V(32)], flags="direct"),
    "direct-stats": dict(n=2, h=32, w=32, taps=9, ins=[V(32)], outs=[V(64)], flags="direct", stats=True),
    "pw-64-32": dict(n=2, h=16, w=16, taps=1, ins=[V(64)], outs=[V(32)]),
    "pw-deconv-64-4x32": dict(n=2, h=16, w=16, taps=1, ins=[V(64)], outs=phases(32)),
    "pw-dgrad-4x32-64": dict(n=2, h=16, w=16, taps=1, ins=phases(32), outs=[V(64, gate=True, accumulate=True)]),
    "pw-deconv-64-4x64-two-per-cu": dict(n=2, h=16, w=16, taps=1, ins=[V(64)], outs=phases(64)),
    "pw-deconv-128-4x64-one-per-cu": dict(n=2, h=16, w=16, taps=1, ins=[V(128)], outs=phases(64)),
    "1x1-w24": dict(n=2, h=8, w=24, taps=1, ins=[V(64)], outs=[V(32)]),
    "1x1-w24-deconv-even-tiles": dict(n=2, h=8, w=24, taps=1, ins=[V(64)], outs=phases(32)),
    "1x1-w24-odd-tiles": dict(n=2, h=8, w=24, taps=1, ins=[V(64)], outs=[V(96)]),
    "1x1-weights-beyond-lds": dict(n=2, h=16, w=16, taps=1, ins=[V(256)], outs=[V(256)]),
    # fp32 without one
    "generic-unaligned-30-32": dict(n=2, h=16, w=16, taps=9, ins=[V(30)], outs=[V(32)], image=False),
    "generic-gate-on-load": dict(n=2, h=16, w=16, taps=9, ins=[V(32, gate=True)], outs=[V(32)], image=False),
    "generic-1x1-aligned": dict(n=2, h=16, w=16, taps=1, ins=[V(64)], outs=[V(32)], image=False),
    "first-layer-cin1": dict(n=2, h=16, w=16, taps=9, ins=[V(1)], outs=[V(32)], image=False),
    "first-layer-cin3": dict(n=2, h=16, w=16, taps=9, ins=[V(3)], outs=[V(32)], image=False),
    "first-layer-cin4": dict(n=2, h=16, w=16, taps=9, ins=[V(4)], outs=[V(32)], image=False),
    "first-layer-cin1-stats-bn": dict(n=32, h=64, w=256, taps=9, ins=[V(1)], outs=[V(32)], image=False, stats=True, bn=True),
    # bf16 storage
    "bf16-first-layer-cin1": dict(n=2, h=16, w=16, taps=9, ins=[V(1)], outs=[V(32)], flags="bf16", image=False),
    "bf16-first-layer-cin3": dict(n=2, h=16, w=16, taps=9, ins=[V(3)], outs=[V(32)], flags="bf16", image=False),
    "bf16-first-layer-cin4": dict(n=2, h=16, w=16, taps=9, ins=[V(4)], outs=[V(32)], flags="bf16", image=False),
    "bf16-32-64-512-units": dict(n=16, h=64, w=256, taps=9, ins=[V(32)], outs=[V(64)], flags="bf16"),
    "bf16-32-64-16-units": dict(n=2, h=64, w=64, taps=9, ins=[V(32)], outs=[V(64)], flags="bf16"),
    "bf16-32-64-small": dict(n=2, h=32, w=32, taps=9, ins=[V(32)], outs=[V(64)], flags="bf16"),
    "bf16-32-32-one-chunk-one-tile": dict(n=2, h=16, w=16, taps=9, ins=[V(32)], outs=[V(32)], flags="bf16"),
    "bf16-64-32-one-tile": dict(n=2, h=32, w=32, taps=9, ins=[V(64)], outs=[V(32)], flags="bf16"),
    "bf16-stats": dict(n=2, h=32, w=32, taps=9, ins=[V(32)], outs=[V(32)], flags="bf16", stats=True),
    "bf16-stats-bn": dict(n=2, h=32, w=32, taps=9, ins=[V(32)], outs=[V(64)], flags="bf16", stats=True, bn=True),
    "bf16-fold": dict(n=2, h=32, w=32, taps=9, ins=[V(32, fold=True)], outs=[V(64)], flags="bf16"),
    "bf16-24-channel-slice": dict(n=2, h=32, w=32, taps=9, ins=[V(32, c_len=24)], outs=[V(64)], flags="bf16"),
    "bf16-pointwise-w24-plain": dict(n=2, h=8, w=24, taps=1, ins=[V(64)], outs=phases(32), flags="bf16"),
    "bf16-pointwise-w24-gated": dict(n=2, h=8, w=24, taps=1, ins=phases(32), outs=[V(64, gate=True, accumulate=True)],
                                     flags="bf16"),
    "bf16-pointwise-w24-odd-tiles": dict(n=2, h=8, w=24, taps=1, ins=[V(64)], outs=[V(96)], flags="bf16"),
    "bf16-pw-64-4x32": dict(n=2, h=16, w=16, taps=1, ins=[V(64)], outs=phases(32), flags="bf16"),
    "bf16-pw-128-4x64-two-per-cu": dict(n=2, h=16, w=16, taps=1, ins=[V(128)], outs=phases(64), flags="bf16"),
    "bf16-pw-dgrad-4x32-64": dict(n=2, h=16, w=16, taps=1, ins=phases(32), outs=[V(64, gate=True, accumulate=True)],
                                  flags="bf16"),
}
# planned for 8 CUs as well: the rows whose form depends on the CU count, and one persistent grid of each family
CUS8 = ["bf16-32-64-512-units", "bf16-32-64-16-units", "bf16-32-64-small", "wino-stats-bn", "first-layer-cin1-stats-bn",
        "pw-64-32", "bf16-pw-64-4x32", "direct-stats", "bf16-fold", "bf16-pointwise-w24-plain"]


def desc(L, mem, n, h, w, taps, ins, outs, flags="", image=True, stats=False, bn=False, image_floats=16):
    """mem(floats) -> a 16-byte aligned address that many floats can be read and written at (or look as if)"""
    d = L.GemmDesc()
    d.N, d.H, d.W, d.taps, d.n_in, d.n_out = n, h, w, taps, len(ins), len(outs)
    d.flags = (L.GEMM_BF16 if "bf16" in flags else 0) | (L.GEMM_DIRECT if "direct" in flags else 0)
    for views, specs in ((d.inp, ins), (d.out, outs)):
        for v, s in zip(views, specs):
            hs, ws = h * s["up"], w * s["up"]
            floats = n * hs * ws * s["c"]
            v.ptr = mem(floats)
            v.C, v.c_off, v.c_len = s["c"], s["c_off"], s["c_len"]
            v.Hs, v.Ws, v.sy, v.sx, v.oy, v.ox = hs, ws, s["up"], s["up"], s["oy"], s["ox"]
            if s["fold"]:
                v.scale, v.shift, v.relu = mem(s["c_len"]), mem(s["c_len"]), 1
            if s["gate"]:
                v.gate = mem(floats)
            v.relu = 1 if (s["relu"] or s["fold"]) else 0
            v.accumulate = 1 if s["accumulate"] else 0
    k = sum(s["c_len"] for s in ins)
    nc = sum(s["c_len"] for s in outs)
    d.weight = mem(taps * k * nc)
    d.weight_image = mem(image_floats) if image else None
    if stats:
        rows = L.lib().unetpp_gemm_stats_rows(n, h, w) if bn else L.lib().unetpp_gemm_pixel_blocks(n, h, w)
        d.stats_partial = mem(rows * nc * 2)
    if bn:
        d.bn.gamma, d.bn.beta, d.bn.mean, d.bn.invstd = (mem(nc) for _ in range(4))
        d.bn.scale, d.bn.shift = mem(nc), mem(nc)
        d.bn.count, d.bn.eps, d.bn.momentum = n * h * w, 1e-5, 0.1
    return d


def fake_mem(floats):
    return 0x100000   # never dereferenced; 16-byte aligned


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN) as f:
        return json.load(f)


def _plan(L, d, cus):
    out = L.GemmSizes()
    assert L.lib().unetpp_gemm_plan(ctypes.byref(d), cus, ctypes.byref(out)) == 0
    return out


def _check(L, case, d, cus, want, what):
    p = _plan(L, d, cus)
    got = dict(label=p.kernel.decode(), workgroups=p.workgroups, threads=p.threads)
    assert got == {k: want[k] for k in got}, (case, what, got, want)
    if "stats_rows" in want:   # what the attached finalize reads = the rows the parent's launch wrote
        blocks = L.lib().unetpp_gemm_pixel_blocks(d.N, d.H, d.W)
        assert (p.bn_rows if p.bn_rows > 0 else blocks) == want["stats_rows"], (case, what, p.bn_rows)
        assert p.bn_rows == 0 or d.bn.scale, (case, what)
    return p


@pytest.mark.parametrize("case", list(CASES))
def test_plan_matches_the_launchers_before_it(L, parent, case):
    rec = parent["rows"][case]
    d = desc(L, fake_mem, **CASES[case])
    p = _check(L, case, d, 256, rec["base"], "cus 256")
    assert p.image_floats == rec["image_floats"] == L.lib().unetpp_gemm_weight_image_floats(ctypes.byref(d))
    for name, value in SWITCHES:
        key = "%s=%d" % (name, value)
        with L.debug_switch(name, value):
            # the record keeps a switch only where it moved the launch
            q = _check(L, case, d, 256, rec["switches"].get(key, rec["base"]), key)
            assert q.image_floats == rec["image_floats"]
    _check(L, case, d, 256, rec["base"], "switches back")
    if case in CUS8:
        _check(L, case, d, 8, rec["cus8"], "cus 8")


def test_record_reaches_every_kernel_and_form(parent):
    seen = set()
    for rec in parent["rows"].values():
        for r in [rec["base"], rec.get("cus8", rec["base"])] + list(rec["switches"].values()):
            seen.add((r["label"], r["threads"]))
    labels = {s[0] for s in seen}
    assert labels == {"small_cin_fwd_kernel", "gemm_pw_bf16_kernel", "gemm_bf16_dma_kernel<9>", "gemm_bf16_dma_kernel<1>",
                      "gemm_bf16_kernel<9>", "gemm_bf16_kernel<1>", "gemm_pw_kernel", "gemm_wino_kernel",
                      "gemm_fast_kernel<9>", "gemm_fast_kernel<1>", "gemm_pix_kernel<9>", "gemm_pix_kernel<1>"}
    assert ("gemm_bf16_dma_kernel<9>", 512) in seen and ("gemm_bf16_dma_kernel<9>", 256) in seen   # 8- and 4-wave forms
    assert set(parent["rows"]) == set(CASES)


def test_weight_image_is_an_input_of_the_selection(L):
    """Only whether d->weight_image is NULL counts, and it decides between the kernels that read the packed operand
    and the image kernels; image_floats does not depend on it."""
    args = CASES["wino-cin4-image"]
    with_image = _plan(L, desc(L, fake_mem, **args), 256)
    elsewhere = _plan(L, desc(L, lambda floats: 0x7f0000000040, **args), 256)
    without = _plan(L, desc(L, fake_mem, **dict(args, image=False)), 256)
    assert with_image.kernel == elsewhere.kernel == b"gemm_wino_kernel" and without.kernel == b"small_cin_fwd_kernel"
    assert with_image.image_floats == elsewhere.image_floats == without.image_floats > 0
    unaligned = desc(L, fake_mem, **CASES["generic-unaligned-30-32"])
    assert _plan(L, unaligned, 256).image_floats == 0
    unaligned.weight_image = 0x100000    # an image no image kernel can read
    out = L.GemmSizes()
    assert L.lib().unetpp_gemm_plan(ctypes.byref(unaligned), 256, ctypes.byref(out)) == -1
    assert L.lib().unetpp_gemm_fwd(ctypes.byref(unaligned), None) == -1


def test_plan_refuses_what_the_launch_refuses(L):
    lib = L.lib()
    out = L.GemmSizes()
    good = dict(n=2, h=32, w=32, taps=9, ins=[V(32)], outs=[V(32)])
    d = desc(L, fake_mem, **good)
    assert lib.unetpp_gemm_plan(None, 256, ctypes.byref(out)) == -1
    assert lib.unetpp_gemm_plan(ctypes.byref(d), 256, None) == -1
    assert lib.unetpp_gemm_fwd(None, None) == -1
    assert lib.unetpp_gemm_plan(ctypes.byref(d), 256, ctypes.byref(out)) == 0

    def two_outputs_with_statistics(d):
        d.n_out = 2
        d.out[1] = d.out[0]
        d.stats_partial = 0x100000

    def no_weights_at_all(d):
        d.weight = d.weight_image = None

    def finalize_without_statistics(d):
        d.bn.scale = d.bn.shift = d.bn.gamma = d.bn.beta = d.bn.mean = d.bn.invstd = 0x100000
        d.bn.count = 2048

    for image in (True, False):
        for flags in ("", "bf16"):
            for change in (lambda d: setattr(d, "taps", 4), lambda d: setattr(d, "n_in", 0), lambda d: setattr(d, "N", 0),
                           lambda d: setattr(d, "n_out", 9), lambda d: setattr(d.out[0], "Hs", 16),
                           lambda d: setattr(d.inp[0], "Ws", 31), two_outputs_with_statistics, no_weights_at_all,
                           finalize_without_statistics):
                d = desc(L, fake_mem, **dict(good, image=image, flags=flags))
                change(d)
                assert lib.unetpp_gemm_plan(ctypes.byref(d), 256, ctypes.byref(out)) == -1, (image, flags)
                assert lib.unetpp_gemm_fwd(ctypes.byref(d), None) == -1, (image, flags)
    # bf16 storage has no generic kernel: without an image only the first layer runs
    bf = desc(L, fake_mem, **dict(good, flags="bf16", image=False))
    assert lib.unetpp_gemm_plan(ctypes.byref(bf), 256, ctypes.byref(out)) == -1
    assert lib.unetpp_gemm_fwd(ctypes.byref(bf), None) == -1
    assert lib.unetpp_gemm_weight_image_floats(ctypes.byref(bf)) > 0   # (its image can still be sized)
    bf = desc(L, fake_mem, **dict(good, flags="bf16", ins=[V(36)]))   # bf16 views are 8-channel aligned
    assert lib.unetpp_gemm_plan(ctypes.byref(bf), 256, ctypes.byref(out)) == -1
    assert lib.unetpp_gemm_fwd(ctypes.byref(bf), None) == -1


def test_plan_for_the_current_device_needs_one(L):
    """cus <= 0 asks the device; on a machine without one the plan says so instead of guessing."""
    d = desc(L, fake_mem, **CASES["wino-32-32"])
    out = L.GemmSizes()
    rc = L.lib().unetpp_gemm_plan(ctypes.byref(d), 0, ctypes.byref(out))
    usable = L.lib().unetpp_usable_cus(None)
    assert rc == (0 if usable > 0 else -2)
    if usable > 0:
        assert (out.kernel, out.workgroups) == (b"gemm_wino_kernel", _plan(L, d, usable).workgroups)
