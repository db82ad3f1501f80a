"""Ignore masks on the GPU, bit for bit against tests/mask_oracle.py:
  (1) unetpp_mask_pack: widths about the word and the wave, one and several rows and planes, uint8 / bool / float with
      NaN and -0.0, a guard behind the output;
  (2) unetpp_mask_polygons: the planted rings of mask_oracle.polygon_case (level edges, vertices on pixel centres, a
      ring of more vertices than the LDS edge chunk, holes and islands, several planes, padding, rings outside and far
      beyond the frame), G = 0, 1, 40, a small grid, permuted rings, two runs, the partition property;
  (3) unetpp_target_ignore_mask: ignore_oracle.MARK_SHAPES with every window kind, the eight flips and turns with
      shifts and overhang, rotation and scale, `outside`, an index outside [0, M), P = 0, a second class group, a
      small grid; agreement with unetpp_target_ignore on whole-number rectangles; refusals;
  (4) SceneCrops, train_step and evaluate end to end."""
import numpy as np
import pytest
import torch

from tests import crops_oracle as co
from tests import ignore_oracle as io
from tests import mask_oracle as mo

pytestmark = pytest.mark.gpu
F32, U32, I32 = np.float32, np.uint32, np.int32
GUARD = 64
PATTERN = np.array([0x3F2A5A5B], dtype=U32).view(F32)[0]        # what the untouched elements of a target hold
GUARD_BITS = 0x7FC0BEEF                                          # a NaN behind the target
WORD_GUARD = 0x5A5AC3C3                                          # behind (and, before the launch, in) a bit plane


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # (a copy: the oracle's cases are read-only)


def _lib_ops():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    from unet_nested4tiny_objects_keypoints_amd.ops import _ptr, _stream, check
    return _lib, _ptr, _stream, check


# (1) -----------------------------------------------------------------------------------------------------------------
def _pack(dev, mask):
    """unetpp_mask_pack through the C ABI into a buffer pre-filled with WORD_GUARD, a guard behind it -> bits as numpy"""
    _lib, _ptr, _stream, check = _lib_ops()
    w = mask.shape[-1]
    rows, wd = mask.size // w, (w + 31) // 32
    buf = torch.full((rows * wd + GUARD,), WORD_GUARD, dtype=torch.int32, device=dev)
    src = _t(mask.view(np.uint8) if mask.dtype == bool else mask, dev)
    kind = _lib.MASK_F32 if mask.dtype == F32 else _lib.MASK_U8
    check(_lib.lib().unetpp_mask_pack(_ptr(src), kind, rows, w, _ptr(buf), _stream()), "unetpp_mask_pack")
    torch.cuda.synchronize()
    assert _lib.lib().unetpp_last_kernel_name() == b"mask_pack"
    assert bool((buf[rows * wd:] == WORD_GUARD).all()), "the guard behind the bits was written"
    return buf[:rows * wd].cpu().numpy().reshape(mask.shape[:-1] + (wd,))


@pytest.mark.parametrize("W", [1, 31, 32, 33, 64, 65, 130])
def test_pack_against_the_oracle(dev, W):
    from unet_nested4tiny_objects_keypoints_amd import IgnoreMask
    rng = np.random.default_rng(700 + W)
    for H in (1, 17):
        for P in (1, 3):
            on = rng.random((2, P, H, W)) < 0.4
            on[0, 0, 0, -1] = True                                    # the last pixel of a row
            f = np.where(on, rng.standard_normal(on.shape), 0.0).astype(F32)
            f[on & (rng.random(on.shape) < 0.2)] = np.nan             # non-zero
            f[~on & (rng.random(on.shape) < 0.3)] = -0.0              # zero
            u8 = np.where(on, rng.integers(1, 256, on.shape), 0).astype(np.uint8)
            want = mo.pack(on)
            for mask in (u8, on, f):
                got = _pack(dev, mask)
                assert np.array_equal(got, want), (W, H, P, mask.dtype)
                assert mo.tails(got, W) == 0
            m = IgnoreMask.from_raster(_t(f, dev), plane_class=list(range(-1, P - 1)))
            assert m.bits.is_cuda and np.array_equal(m.bits.cpu().numpy(), want) and m.size == (H, W)
            assert np.array_equal(m.to_raster().cpu().numpy(), on)
            assert np.array_equal(IgnoreMask.from_raster(_t(on[:, 0], dev)).bits.cpu().numpy(), want[:, :1])   # [S, H, W]
            assert np.array_equal(IgnoreMask.from_raster(_t(f.astype(np.float64), dev)).bits.cpu().numpy(), want)


# (2) -----------------------------------------------------------------------------------------------------------------
def _polygons(dev, case):
    """unetpp_mask_polygons through the C ABI into a buffer pre-filled with WORD_GUARD -> raster bool [S, P, H, W]"""
    _lib, _ptr, _stream, check = _lib_ops()
    (H, W), P = case["size"], case["planes"]
    S, G, V = case["vertices"].shape[:3]
    wd = (W + 31) // 32
    n = S * P * H * wd
    buf = torch.full((n + GUARD,), WORD_GUARD, dtype=torch.int32, device=dev)
    v, c, p, k = (_t(case[key], dev) if G else None for key in ("vertices", "counts", "poly_plane", "poly_clear"))
    check(_lib.lib().unetpp_mask_polygons(_ptr(v), _ptr(c), _ptr(p), _ptr(k), S, G, V, P, H, W, _ptr(buf), _stream()),
          "unetpp_mask_polygons")
    torch.cuda.synchronize()
    assert _lib.lib().unetpp_last_kernel_name() == b"mask_polygons"
    assert bool((buf[n:] == WORD_GUARD).all()), "the guard behind the bits was written"
    bits = buf[:n].cpu().numpy().reshape(S, P, H, wd)
    assert mo.tails(bits, W) == 0
    return mo.unpack(bits, W)


def _diff(got, want):
    return int((got != want).sum()), np.argwhere(got != want)[:5].tolist()


@pytest.mark.parametrize("G", mo.POLY_G)
@pytest.mark.parametrize("size", mo.POLY_FRAMES, ids=lambda s: "%dx%d" % s)
def test_polygons_against_the_oracle(dev, size, G):
    from tests.helpers import usable_cus
    H, W = size
    case = mo.polygon_case(H, W, G)
    want = mo.polygon_expected(H, W, G)
    got = _polygons(dev, case)
    assert np.array_equal(got, want), _diff(got, want)
    assert want.any() == (G > 0)
    assert np.array_equal(_polygons(dev, case), got)                  # a second run
    with usable_cus(8):                                               # 64 workgroups: some take a second unit
        assert np.array_equal(_polygons(dev, case), got)
    if G > 1:
        perm = mo.permuted_sets(case)
        assert not np.array_equal(perm["counts"], case["counts"])
        assert np.array_equal(_polygons(dev, perm), got)


def test_from_polygons_and_the_partition_property(dev):
    from unet_nested4tiny_objects_keypoints_amd import IgnoreMask
    size = mo.PARTITION_SIZE
    for seed in range(4):
        c = mo.partition_case(seed)
        case = mo.rings_as_case([c["whole"], c["left"], c["right"]], size)
        got = _polygons(dev, case)[0]
        assert not (got[1] & got[2]).any() and np.array_equal(got[1] | got[2], got[0])
        for p, k in enumerate(("whole", "left", "right")):
            assert np.array_equal(got[p], mo.ring_inside_int(c[k + "_q"], size)), (seed, k)
    # the class method: defaults (plane 0, no clearing ring), [G] lists broadcast over the frames, plane classes
    H, W = mo.POLY_FRAMES[0]
    case = mo.polygon_case(H, W, 40)
    want = mo.polygon_expected(H, W, 40)
    m = IgnoreMask.from_polygons(_t(case["vertices"], dev), _t(case["counts"], dev), (H, W), _t(case["poly_plane"], dev),
                                 _t(case["poly_clear"], dev).bool(), plane_class=[-1, 0, 1])
    assert np.array_equal(m.to_raster().cpu().numpy(), want) and m.plane_class.tolist() == [-1, 0, 1] and len(m) == 2
    flat = mo.polygons(case["vertices"], case["counts"], (H, W), None, None, 1)
    m0 = IgnoreMask.from_polygons(_t(case["vertices"], dev), _t(case["counts"], dev), (H, W))
    assert m0.planes == 1 and np.array_equal(m0.to_raster().cpu().numpy(), flat)
    shared = IgnoreMask.from_polygons(_t(case["vertices"], dev), _t(case["counts"], dev), (H, W),
                                      poly_plane=case["poly_plane"][0].tolist(), poly_clear=case["poly_clear"][0].tolist())
    assert shared.planes == 6                                         # max(poly_plane) + 1: ring 11 names plane 5
    assert np.array_equal(shared.to_raster().cpu().numpy()[:, :3],
                          mo.polygons(case["vertices"], case["counts"], (H, W), case["poly_plane"][0], case["poly_clear"][0], 3))
    cov = m.coverage().cpu().numpy()
    assert np.allclose(cov, want.mean(axis=(2, 3)), rtol=0, atol=1e-15)
    assert np.array_equal(m.union(m).bits.cpu().numpy(), m.bits.cpu().numpy())
    host = m.to("cpu")
    assert host.device.type == "cpu" and np.array_equal(host.to_raster().numpy(), want)


# (3) -----------------------------------------------------------------------------------------------------------------
def _mark(dev, case, C_, size, outside, prefill=None, n_frames=None):
    """unetpp_target_ignore_mask through the C ABI on a target pre-filled with PATTERN (or `prefill`) and a guard
    behind it -> the target as numpy"""
    _lib, _ptr, _stream, check = _lib_ops()
    N, (Ho, Wo), (Hs, Ws) = len(case["index"]), size, case["src_size"]
    n = N * C_ * Ho * Wo
    buf = torch.empty(n + GUARD, dtype=torch.float32, device=dev)
    buf[:n] = float(PATTERN) if prefill is None else _t(prefill, dev).reshape(-1)
    buf[n:].view(torch.int32).fill_(GUARD_BITS)
    raster = case["raster"]
    M, P = raster.shape[:2]
    M = M if n_frames is None else n_frames
    if P and "bits" not in case:
        case["bits"] = mo.pack(raster)                               # packed once per case
    bits, cls = (_t(case["bits"], dev), _t(np.asarray(case["plane_class"], I32), dev)) if P else (None, None)
    index, rows = _t(case["index"], dev), _t(case["rows"], dev)
    check(_lib.lib().unetpp_target_ignore_mask(_ptr(bits), _ptr(cls), M, P, Hs, Ws, _ptr(index), N, _ptr(rows), C_, Ho, Wo,
                                               1 if outside else 0, _ptr(buf), _stream()), "unetpp_target_ignore_mask")
    torch.cuda.synchronize()
    assert bool((buf[n:].view(torch.int32) == GUARD_BITS).all()), "the guard behind the target was written"
    return buf[:n].view(N, C_, Ho, Wo).cpu().numpy()


def _want(case, C_, size, outside, prefill=None, n_frames=None):
    N = len(case["index"])
    base = np.full((N, C_) + tuple(size), PATTERN, dtype=F32) if prefill is None else prefill
    mask = mo.mark_mask_bits(case["raster"], case["plane_class"], case["index"], case["rows"], C_, size, outside,
                             n_frames=n_frames)
    return io.apply_mark(base, mask), mask


def _same(got, want):
    return np.array_equal(got.view(I32), want.view(I32))


@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("shape", io.MARK_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_mark_against_the_oracle(dev, shape, P):
    _lib = _lib_ops()[0]
    N, C_, Ho, Wo = shape
    rng = np.random.default_rng(31)
    prefill = rng.random((N, C_, Ho, Wo)).astype(F32)                    # every unmarked element keeps its bits
    for kind0 in range(4):                                               # every sample slot sees every window kind
        case = mo.mark_case(N, C_, Ho, Wo, P, first_kind=kind0)
        for outside in (False, True):
            got = _mark(dev, case, C_, (Ho, Wo), outside, prefill=prefill)
            assert _lib.lib().unetpp_last_kernel_name() == b"target_ignore_mask"
            want, mask = _want(case, C_, (Ho, Wo), outside, prefill=prefill)
            assert _same(got, want), (shape, P, outside, case["kinds"], int((got.view(I32) != want.view(I32)).sum()))
            assert mask.any() and not mask[0].all()
            if N >= 3:                                                   # an index outside [0, M)
                assert (got[1] == -1).all() if outside else _same(got[1], prefill[1])
    assert _same(_mark(dev, case, C_, (Ho, Wo), True), _want(case, C_, (Ho, Wo), True)[0])    # on the constant pattern


def test_mark_the_eight_flips_and_turns_overhang_rotation_and_scale(dev):
    from unet_nested4tiny_objects_keypoints_amd.loader import affine_params
    for Ho, Wo in ((40, 48), (33, 70)):
        case = mo.dihedral_case(Ho, Wo)
        for outside in (True, False):
            got = _mark(dev, case, case["C"], (Ho, Wo), outside)
            want, mask = _want(case, case["C"], (Ho, Wo), outside)
            assert _same(got, want), (Ho, Wo, outside, int((got.view(I32) != want.view(I32)).sum()))
            assert mask[10].all() == outside and mask[10].any() == outside    # index = -1
    # opt-in rotation and scale: rows from affine_params, positions between the pixels
    N, C_, Ho, Wo = io.MARK_SHAPES[1]
    base = mo.mark_case(N, C_, Ho, Wo, 4)
    fwd = mo.affine_rows(Ho, Wo, (co.X0 + Wo / 2.0, co.Y0 + Ho / 2.0), n=4)
    case = dict(raster=base["raster"], plane_class=base["plane_class"], src_size=base["src_size"],
                rows=affine_params(fwd).numpy(), index=np.asarray([0, 1, 1, 0], np.int64))
    for outside in (True, False):
        got = _mark(dev, case, C_, (Ho, Wo), outside)
        want, mask = _want(case, C_, (Ho, Wo), outside)
        assert _same(got, want) and 0.02 < mask.mean() < 0.98
    xs, _ = io.source_positions(case["rows"][0], Ho, Wo)
    assert (xs != np.round(xs)).any()


def test_mark_without_planes_a_second_class_group_and_a_small_grid(dev):
    from tests.helpers import usable_cus
    # P = 0: the `outside` rule alone, the rectangle kernel's with R = 0
    oc = io.outside_case()
    case = dict(oc, raster=np.zeros((2, 0) + oc["src_size"], bool), plane_class=np.zeros(0, I32))
    for outside in (True, False):
        got = _mark(dev, case, oc["C"], oc["out_size"], outside, n_frames=2)
        want = io.apply_mark(np.full(got.shape, PATTERN, F32),
                             io.mark_mask(oc["rects"][:, :0], oc["rect_class"][:, :0], oc["index"], oc["rows"], oc["C"],
                                          oc["out_size"], oc["src_size"], outside))
        assert _same(got, want) and (got == -1).any() == outside
        assert _same(got, _want(case, oc["C"], oc["out_size"], outside, n_frames=2)[0])
    # C = 40: planes of classes 35 and 32 take a second class group
    N, C_, Ho, Wo = 1, 40, 33, 70
    base = mo.mark_case(N, 4, Ho, Wo, 4)
    case = dict(plane_class=np.asarray([-1, 35, 32, 40], I32), index=base["index"], rows=base["rows"], src_size=base["src_size"])
    case["raster"] = base["raster"] & (np.random.default_rng(3).random(base["raster"].shape[-2:]) < 0.5)   # sparser
    got = _mark(dev, case, C_, (Ho, Wo), True)
    want, mask = _want(case, C_, (Ho, Wo), True)
    assert _same(got, want)
    assert (mask[0, 35] & ~mask[0, 34]).any() and (mask[0, 32] & ~mask[0, 33]).any() and not mask[0, 39].all()
    # 90 units of (sample, tile) on 64 workgroups: some take a second unit
    big = mo.mark_case(2, 3, 129, 257, 4, first_kind=3)
    full = _mark(dev, big, 3, (129, 257), True)
    with usable_cus(8):
        small = _mark(dev, big, 3, (129, 257), True)
    assert _same(full, small) and _same(full, _want(big, 3, (129, 257), True)[0])


def test_mark_agrees_with_the_rectangle_path(dev):
    """whole-number rectangles rasterised by the oracle, windows of the exact family (whole-number source positions):
    unetpp_target_ignore_mask writes the bits unetpp_target_ignore writes"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    for (N, C_, Ho, Wo), codes in (((3, 4, 40, 48), (0, 2, 4, 6)), ((2, 2, 33, 70), (6, 4, 2, 0)),
                                  ((4, 3, 40, 40), (1, 3, 5, 7)), ((4, 3, 40, 40), (0, 7, 2, 5))):
        rc = io.mark_case(N, C_, Ho, Wo, 300)
        rects = np.round(rc["rects"])                                 # (a NaN stays one; half-way edges become whole)
        rows = np.stack([mo.window_row8(codes[n % 4], (co.X0 + 3 * n, co.Y0 - 2 * n), (Ho, Wo)) for n in range(N)]).astype(F32)
        xs, ys = io.source_positions(rows[N - 1], Ho, Wo)
        assert (xs == np.round(xs)).all() and (ys == np.round(ys)).all()
        raster, classes = mo.rects_raster(rects, rc["rect_class"], C_, rc["src_size"])
        case = dict(raster=raster, plane_class=classes, index=rc["index"], rows=rows, src_size=rc["src_size"])
        for outside in (False, True):
            got = _mark(dev, case, C_, (Ho, Wo), outside)
            target = torch.full((N, C_, Ho, Wo), float(PATTERN), device=dev)
            ops.target_ignore(target, _t(rects.astype(F32), dev), _t(rc["rect_class"], dev), _t(rc["index"], dev), _t(rows, dev),
                              rc["src_size"], outside=outside)
            assert _same(got, target.cpu().numpy()), (N, C_, Ho, Wo, outside)
            assert (got == -1).any() and not (got == -1).all()


def test_refusals(dev):
    from unet_nested4tiny_objects_keypoints_amd import IgnoreMask, ops
    _lib = _lib_ops()[0]
    lib = _lib.lib()
    N, C_, Ho, Wo = 2, 2, 33, 70
    Hs, Ws = 50, 30
    raster = np.random.default_rng(1).random((2, 2, Hs, Ws)) < 0.5
    bits, cls = _t(mo.pack(raster), dev), _t(np.asarray([-1, 0], I32), dev)
    idx = _t(np.asarray([0, 1], np.int64), dev)
    rows = _t(np.stack([io.window_row("identity", (-9, 4), (Ho, Wo))] * 2).astype(F32), dev)
    tgt = torch.full((N, C_, Ho, Wo), float(PATTERN), device=dev)
    good = dict(bits=bits.data_ptr(), plane_class=cls.data_ptr(), M=2, P=2, Hs=Hs, Ws=Ws, index=idx.data_ptr(), N=2,
                params=rows.data_ptr(), C=2, Ho=Ho, Wo=Wo, outside=1, target=tgt.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.unetpp_target_ignore_mask(a["bits"], a["plane_class"], a["M"], a["P"], a["Hs"], a["Ws"], a["index"], a["N"],
                                             a["params"], a["C"], a["Ho"], a["Wo"], a["outside"], a["target"], None)

    for bad in (dict(bits=None), dict(plane_class=None), dict(index=None), dict(params=None), dict(target=None), dict(M=0),
                dict(P=-1), dict(N=0), dict(C=0), dict(C=65536), dict(Ho=0), dict(Wo=-1), dict(Hs=0), dict(Ws=0),
                dict(Ho=(1 << 24) + 1), dict(Ws=(1 << 24) + 1)):
        assert call(**bad) == -1, bad
    assert call(P=0, outside=0, bits=None, plane_class=None) == 0
    src = torch.zeros(4, 40, dtype=torch.uint8, device=dev)
    out = torch.full((4, 2), WORD_GUARD, dtype=torch.int32, device=dev)
    for args in ((None, 0, 4, 40, out.data_ptr()), (src.data_ptr(), 0, 4, 40, None), (src.data_ptr(), 2, 4, 40, out.data_ptr()),
                 (src.data_ptr(), 0, 0, 40, out.data_ptr()), (src.data_ptr(), 0, 4, 0, out.data_ptr()),
                 (src.data_ptr(), 0, 1 << 20, 1 << 12, out.data_ptr())):
        assert lib.unetpp_mask_pack(*args, None) == -1, args
    v = torch.zeros(1, 1, 3, 2, device=dev)
    c = torch.full((1, 1), 3, dtype=torch.int32, device=dev)
    ok = dict(v=v.data_ptr(), c=c.data_ptr(), p=c.data_ptr(), k=c.data_ptr(), S=1, G=1, V=3, P=1, H=4, W=40, bits=out.data_ptr())
    for bad in (dict(v=None), dict(c=None), dict(p=None), dict(k=None), dict(bits=None), dict(S=0), dict(G=-1), dict(V=-1),
                dict(P=0), dict(H=0), dict(W=0), dict(W=(1 << 24) + 1)):
        a = dict(ok, **bad)
        assert lib.unetpp_mask_polygons(a["v"], a["c"], a["p"], a["k"], a["S"], a["G"], a["V"], a["P"], a["H"], a["W"],
                                        a["bits"], None) == -1, bad
    torch.cuda.synchronize()
    assert bool((tgt == float(PATTERN)).all()) and bool((out == WORD_GUARD).all())      # nothing was touched
    # through ops: dtypes, devices, geometry, C
    cpu = torch.device("cpu")
    with pytest.raises(TypeError):
        ops.target_ignore_mask(tgt, bits.to(torch.int64), cls, idx, rows, (Hs, Ws))
    with pytest.raises(TypeError):
        ops.target_ignore_mask(tgt, bits, cls.to(torch.int64), idx, rows, (Hs, Ws))
    with pytest.raises(TypeError):
        ops.target_ignore_mask(tgt.double(), bits, cls, idx, rows, (Hs, Ws))
    with pytest.raises(RuntimeError):
        ops.target_ignore_mask(tgt, bits.to(cpu), cls, idx, rows, (Hs, Ws))
    with pytest.raises(ValueError):
        ops.target_ignore_mask(tgt, bits, cls, idx, rows, (Hs, Ws + 40))              # the planes are of another size
    with pytest.raises(ValueError):
        ops.target_ignore_mask(tgt, bits, cls[:1], idx, rows, (Hs, Ws))
    with pytest.raises(ValueError):
        ops.target_ignore_mask(tgt, bits, cls, idx[:1], rows, (Hs, Ws))
    with pytest.raises(ValueError):
        ops.target_ignore_mask(tgt, None, None, idx, rows, (Hs, Ws))                  # no planes and no n_frames
    with pytest.raises(ValueError):
        ops.target_ignore_mask(torch.zeros(1, 65536, 1, 1, device=dev), None, None, idx[:1], rows[:1], (Hs, Ws), True, n_frames=1)
    with pytest.raises(TypeError):
        ops.mask_polygons(v.double(), c, c, c, 1, (4, 40))
    with pytest.raises(TypeError):
        ops.mask_polygons(v, c.long(), c, c, 1, (4, 40))
    with pytest.raises(ValueError):
        ops.mask_polygons(v, c, c, c.view(1, 1, 1), 1, (4, 40))
    with pytest.raises(ValueError):
        ops.mask_polygons(v, c, c, c, 0, (4, 40))
    with pytest.raises(ValueError):
        IgnoreMask.from_polygons(v, torch.zeros(1, 2, dtype=torch.int32), (4, 40))
    torch.cuda.synchronize()
    assert bool((tgt == float(PATTERN)).all())


# (4) -----------------------------------------------------------------------------------------------------------------
def _scene():
    S, H, W, per = 2, 80, 96, 9
    rng = np.random.default_rng(18)
    frames = rng.integers(0, 255, size=(S, H, W, 1), dtype=np.uint8)
    labels = np.zeros((S, per, 2), dtype=F32)
    classes = np.zeros((S, per), dtype=I32)
    for s in range(S):
        flat = rng.choice(H * W, per, replace=False)
        labels[s, :, 0], labels[s, :, 1] = flat % W, flat // W
        classes[s] = rng.integers(0, 2, per)
    labels[0, 0], classes[0, 0] = (30, 20), 0                      # a label inside the masked area of frame 0
    labels[0, 1], classes[0, 1] = (88, 56), 1                      # a label of class 1 under the class-0 plane: stays
    raster = np.zeros((S, 2, H, W), bool)                          # plane 0: every class; plane 1: class 0
    ys, xs = np.mgrid[0:H, 0:W]
    raster[0, 0] = (xs - 32) ** 2 + (ys - 21) ** 2 <= 81           # a disc
    raster[0, 1, 50:, 60:] = True
    raster[1, 0] = (xs + ys) % 11 == 0                             # stripes
    raster[1, 1, :30, :20] = True
    rects = np.asarray([[[60, 50, 95, 79], [5, 5, 4, 4]], [[50.5, 10.5, 70.5, 30.5], [10, 60, 30, 70]]], dtype=F32)
    rcls = np.asarray([[1, -1], [-1, 7]], dtype=I32)
    return frames, labels, classes, raster, rects, rcls


def test_scene_crops_mark_their_targets(dev):
    """two 96 x 80 frames under 88 x 88 windows (a centred pad in y, flips and quarter turns): the target is the oracle's
    mark over the target of the same seed without ignore"""
    from unet_nested4tiny_objects_keypoints_amd import (IgnoreMask, IgnoreRegions, IgnoreUnion, ObjectPaste, SceneCrops,
                                                        _lib)
    from unet_nested4tiny_objects_keypoints_amd.crops import paste_source_table
    frames, labels, classes, raster, rects, rcls = _scene()
    size, src = (88, 88), (80, 96)
    planes = [-1, 0]

    def make(**kw):
        return SceneCrops(_t(frames, dev), _t(labels, dev), _t(classes, dev), n_classes=2, crop=size, p_object=0.6,
                          jitter=(20, 20), radius=3.0, seed=5, **kw)

    base = [v.cpu().numpy() for v in make().batch(4)]
    mask = IgnoreMask.from_raster(_t(raster, dev), planes)
    regions = IgnoreRegions(rects, rcls)
    for kw, with_rects in ((dict(ignore=mask), False), (dict(ignore=mask.to("cpu"), ignore_outside=True), False),
                           (dict(ignore=IgnoreUnion(regions, mask)), True),
                           (dict(ignore=IgnoreUnion(mask, regions), ignore_outside=True), True)):
        crops = make(**kw)
        got = [v.cpu().numpy() for v in crops.batch(4)]
        rows, index, origin = (v.cpu().numpy() for v in crops.last)
        for a, b in ((got[0], base[0]), (got[2], base[2]), (got[3], base[3])):      # inputs, points, inside: untouched
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        outside = kw.get("ignore_outside", False)
        want = mo.mark_mask_bits(raster, planes, index, rows, 2, size, outside)
        if with_rects:
            want = want | io.mark_mask(rects, rcls, index, rows, 2, size, src, outside)
        assert np.array_equal(got[1].view(I32), io.apply_mark(base[1], want).view(I32)), kw
        assert 0.01 < want.mean() < 0.9 and (got[1][~want] >= 0).all()
    assert _lib.lib().unetpp_last_kernel_name() in (b"target_ignore", b"target_ignore_mask")
    # geometry and types
    with pytest.raises(ValueError):
        make(ignore=IgnoreMask.from_raster(_t(raster[:1], dev)))                     # one frame for two
    with pytest.raises(ValueError):
        make(ignore=IgnoreMask.from_raster(_t(raster[:, :, :, :90], dev)))           # another frame size
    with pytest.raises(ValueError):
        make(ignore=IgnoreUnion(regions, IgnoreMask.from_raster(_t(raster[:, :, :70], dev))))
    with pytest.raises(TypeError, match="IgnoreMask"):
        make(ignore=raster)
    # a paste source inside a masked area is excluded; for an IgnoreRegions the table is what it was
    args = (_t(labels, dev), _t(classes, dev), 2, src, 2)
    f0, xy0, c0 = paste_source_table(*args)
    f1, xy1, c1 = paste_source_table(*args, ignore=mask)
    rows0 = {(int(f), float(x), float(y)) for f, (x, y) in zip(f0.tolist(), xy0.tolist())}
    rows1 = {(int(f), float(x), float(y)) for f, (x, y) in zip(f1.tolist(), xy1.tolist())}
    assert (0, 30.0, 20.0) in rows0 and (0, 30.0, 20.0) not in rows1 and rows1 < rows0
    assert (0, 88.0, 56.0) in rows1                                                   # class 1 under the class-0 plane
    keep = ~mo.contains(raster, planes, np.arange(2).reshape(2, 1), classes, labels)
    assert rows1 == {r for r in rows0 if keep[r[0]][(labels[r[0]] == np.asarray(r[1:], F32)).all(axis=1)].all()}
    f2, xy2, _ = paste_source_table(*args, ignore=IgnoreUnion(mask, regions))
    both = keep & ~io.contains(rects, rcls, np.arange(2).reshape(2, 1), classes, labels)
    assert len(f2) == sum(1 for r in rows0 if both[r[0]][(labels[r[0]] == np.asarray(r[1:], F32)).all(axis=1)].all())
    crops = make(ignore=mask, paste=ObjectPaste(max_pastes=2, p=1.0, patch_radius=2, core=1.5))
    assert torch.equal(crops.paste.src_frame, f1) and torch.equal(crops.paste.src_xy, xy1)
    assert all(torch.isfinite(v.float()).all() for v in crops.batch(2))


def test_one_train_step_on_a_masked_batch(dev):
    from unet_nested4tiny_objects_keypoints_amd import (IgnoreMask, PenaltyReducedFocalLoss, SceneCrops, UNet_Nested,
                                                        train_step)
    frames, labels, classes, raster, _, _ = _scene()
    crops = SceneCrops(_t(frames, dev), _t(labels, dev), _t(classes, dev), n_classes=2, crop=(32, 32), p_object=0.6,
                       jitter=(8, 8), radius=3.0, seed=6, ignore=IgnoreMask.from_raster(_t(raster, dev), [-1, 0]),
                       ignore_outside=True)
    x, target, _, _ = crops.batch(2)
    assert bool((target < 0).any()) and bool((target >= 0).any())
    torch.manual_seed(81)
    model = UNet_Nested(in_channels=1, n_classes=2, feature_scale=8, depth=3).to(dev).train()
    model.drop_out.p = 0.0
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    outs, loss = train_step(model, opt, PenaltyReducedFocalLoss(ignore_negative=True), x, target)
    assert np.isfinite(float(loss)) and float(loss) > 0
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


def test_evaluate_drops_what_lies_in_the_mask(dev):
    """the blobs of tests/test_gpu_ignore.py with its rectangles rasterised: the same counts"""
    from unet_nested4tiny_objects_keypoints_amd import (IgnoreMask, IgnoreRegions, IgnoreUnion, PeakDetector, evaluate,
                                                        false_positive_centres)
    H = W = 64
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)

    def blob(cx, cy):
        return np.exp(-0.5 * np.sqrt((xs - cx) ** 2 + (ys - cy) ** 2) / 3.0)

    maps = np.zeros((1, 2, H, W), dtype=F32)
    maps[0, 0] = np.maximum.reduce([blob(10, 12), blob(40, 44), blob(50, 10)]).astype(F32)     # (50, 10): in the mask
    maps[0, 1] = np.maximum.reduce([blob(20, 50), blob(8, 30)]).astype(F32)                     # (8, 30): a false positive
    labels = np.asarray([[[10, 12], [40, 44], [20, 50], [55, 15], [-1, -1]]], dtype=F32)      # (55, 15): in the mask
    classes = np.asarray([[0, 0, 1, 0, -1]], dtype=I32)
    raster = np.zeros((1, 2, H, W), bool)
    raster[0, 0, 4:21, 44:61] = True
    raster[0, 1, 24:37, 0:17] = True
    dets = PeakDetector(threshold=0.5, radius=2)(_t(maps, dev))
    plain = evaluate(dets, _t(labels, dev), _t(classes, dev), 3.0)
    assert (int(plain.tp_total), int(plain.fp_total), int(plain.fn_total)) == (3, 2, 1)
    mask = IgnoreMask.from_raster(_t(raster, dev), [0, 0])                                      # both planes: class 0 only
    score = evaluate(dets, _t(labels, dev), _t(classes, dev), 3.0, ignore=mask)
    assert (int(score.tp_total), int(score.fp_total), int(score.fn_total)) == (3, 1, 0)
    assert score.tp.tolist() == [[2, 1]] and score.fp.tolist() == [[0, 1]] and score.fn.tolist() == [[0, 0]]
    assert int(score.served.sum()) == int(plain.served.sum()) - 1 and int(score.label_pred[0, 3]) == -1
    f, p = false_positive_centres(dets, score)
    assert f.tolist() == [0] and p.cpu().round().tolist() == [[8.0, 30.0]]                     # nothing from the mask
    rect = IgnoreRegions(np.asarray([[[44, 4, 60, 20], [0, 24, 16, 36]]], dtype=F32), [0, 0])
    same = evaluate(dets, _t(labels, dev), _t(classes, dev), 3.0, ignore=rect)
    assert torch.equal(same.served, score.served) and torch.equal(same.label_pred, score.label_pred)
    # with the class-1 false positive masked as well, by a union of a CPU mask and a rectangle: AP = 1
    union = IgnoreUnion(IgnoreMask.from_raster(torch.from_numpy(raster[:, :1]), [0]),
                        IgnoreRegions(np.asarray([[[0, 24, 16, 36]]], dtype=F32), [-1]))
    clean = evaluate(dets, _t(labels, dev), _t(classes, dev), 3.0, ignore=union)
    assert (int(clean.tp_total), int(clean.fp_total), int(clean.fn_total)) == (3, 0, 0)
    assert float(clean.average_precision) == 1.0 and len(false_positive_centres(dets, clean)[0]) == 0
