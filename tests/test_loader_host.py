"""CPU checks of the device input pipeline's conventions (loader.py, csrc/loader.hip) and of the float64 restatement the
GPU tests hold the kernels against (tests/loader_oracle.py):
  (1) the restatement is F.grid_sample(bilinear, zeros, align_corners=True) in float64;
  (2) the eight dihedral maps are torch.flip / rot90 plus a shift, exactly;
  (3) an fp32 evaluation in the kernel's operation order stays inside the derived bound;
  (4) affine_params: forward composed with inverse is the identity;
  (5) argument checks of the entry points (status codes, no device touched) and no CPU fallback.

The bound of (3), derived and not measured (u = 2^-24): the source position carries dx = 4u (|m0| xo + |m1| yo + |m2|)
(three roundings of terms of that size), dy likewise; the fill-padded bilinear surface is continuous with slopes at most
Dx, Dy (the largest neighbour differences of the padded image), so a position error moves the value by at most
dx Dx + dy Dy whichever cell the floor lands in; weights, products and the three additions add less than 8u Vmax."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loader_oracle as lo


def test_restatement_is_grid_sample():
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    worst = 0.0
    for (Hs, Ws), (Ho, Wo) in (((48, 80), (64, 64)), ((24, 40), (32, 52)), ((9, 7), (5, 11))):
        img = rng.uniform(-1, 1, (3, Hs, Ws))
        rows = lo.random_rows(rng, 4, (Hs, Ws), (Ho, Wo))
        for r in rows:
            got = lo.warp_plane(img, r[:6], (Ho, Wo), 0.0)
            xo, yo = np.meshgrid(np.arange(Wo, dtype=np.float64), np.arange(Ho, dtype=np.float64))
            xs, ys = r[0] * xo + r[1] * yo + r[2], r[3] * xo + r[4] * yo + r[5]
            grid = torch.from_numpy(np.stack([2 * xs / (Ws - 1) - 1, 2 * ys / (Hs - 1) - 1], axis=-1))[None]
            want = F.grid_sample(torch.from_numpy(img)[None], grid, mode="bilinear", padding_mode="zeros",
                                 align_corners=True)[0].numpy()
            worst = max(worst, float(np.abs(got - want).max()))
    assert worst <= 1e-9, worst


@pytest.mark.parametrize("out_size", ["turned", (16, 20), (32, 52)], ids=["same", "crop", "pad"])
@pytest.mark.parametrize("shift", [(0, 0), (3, -5), (-30, 2)], ids=["t0", "t3-5", "t-30+2"])
def test_dihedral_maps_are_flips_and_turns(shift, out_size):
    Hs, Ws, fill = 24, 40, 7.0
    img = np.random.default_rng(5).integers(0, 256, (2, Hs, Ws)).astype(np.float64)
    for flip_x, q in lo.DIHEDRAL:
        size = ((Ws, Hs) if q % 2 else (Hs, Ws)) if out_size == "turned" else out_size
        row = lo.dihedral_rows([(flip_x, q, shift)], (Hs, Ws), size)[0]
        assert np.array_equal(row, np.round(row)), (flip_x, q, row)             # whole numbers: a pixel permutation
        for dt in (np.float64, np.float32):
            got = lo.warp_plane(img, row[:6], size, fill, dtype=dt)
            want = lo.dihedral_torch(torch.from_numpy(img), flip_x, q, shift, size, fill).numpy()
            assert np.array_equal(got, want), (flip_x, q, shift, size, dt)
    # the quarter turn of the parameter row is the clockwise one
    row = lo.dihedral_rows([(False, 1, (0, 0))], (Hs, Ws), (Ws, Hs))[0]
    assert np.array_equal(lo.warp_plane(img, row[:6], (Ws, Hs), fill), np.rot90(img, -1, axes=(1, 2)))


def test_fp32_evaluation_stays_inside_the_bound():
    rng = np.random.default_rng(11)
    fill, worst = 7.0, 0.0
    for i in range(300):
        Hs, Ws = int(rng.integers(48, 65)), int(rng.integers(64, 81))
        size = (64, 64) if i % 2 else (32, 52)
        img = rng.integers(0, 256, (1, Hs, Ws)).astype(np.float64)
        row = lo.random_rows(rng, 1, (Hs, Ws), size)[0].astype(np.float32)
        want = lo.warp_plane(img, row[:6].astype(np.float64), size, fill)
        got = lo.warp_plane(img, row[:6], size, fill, dtype=np.float32)
        assert got.dtype == np.float32
        ratio = float((np.abs(got.astype(np.float64) - want) / lo.plane_bound(img, row[:6], size, fill)).max())
        worst = max(worst, ratio)
    print("fp32 emulation: worst err/bound", worst)
    assert worst <= 1.0, worst


def test_affine_params_forward_and_inverse_compose_to_identity():
    from unet_nested4tiny_objects_keypoints_amd import affine_params
    rng = np.random.default_rng(2)
    want = lo.random_rows(rng, 32, (48, 80), (64, 64))
    rows = affine_params(want[:, 6:12].reshape(-1, 2, 3), gain=torch.from_numpy(want[:, 12]), bias=0.25)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (32, 16)
    assert bool((rows[:, 14:] == 0).all()) and bool((rows[:, 13] == 0.25).all())
    assert np.allclose(rows[:, 12].numpy(), want[:, 12], rtol=1e-7)
    assert np.allclose(rows.numpy()[:, :12], want[:, :12], rtol=1e-6, atol=1e-5)   # the oracle's closed-form inverse
    r = rows.double().numpy()
    for n in range(32):
        inv = np.vstack([r[n, :6].reshape(2, 3), [0, 0, 1]])
        fwd = np.vstack([r[n, 6:12].reshape(2, 3), [0, 0, 1]])
        pts = np.array([[0, 0, 1], [63, 0, 1], [0, 63, 1], [63, 63, 1]], dtype=np.float64).T
        back = fwd @ (inv @ pts)
        assert float(np.abs(back - pts).max()) <= 1e-6 * 64, n
    one = affine_params([[1, 0, 2], [0, 1, -3]])
    assert one.tolist() == [[1, 0, -2, 0, 1, 3, 1, 0, 2, 0, 1, -3, 1, 0, 0, 0]]
    with pytest.raises(ValueError):
        affine_params([[1, 2, 0], [2, 4, 0]])


def test_argument_checks_touch_no_device():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host

    def warp(store=p, kind=_lib.STORE_U8, M=4, Hs=8, Ws=8, C=1, index=p, N=2, params=p, mul=p, add=p, out=p, Ho=8,
             Wo=8, labels=None, S=0, labels_out=None, inside=None):
        return lib.unetpp_warp_batch(store, kind, M, Hs, Ws, C, index, N, params, mul, add, 0.0, out, Ho, Wo, labels, S,
                                     labels_out, inside, None)

    for name in ("store", "index", "params", "mul", "add", "out"):
        assert warp(**{name: None}) == -1, name
    for name in ("M", "Hs", "Ws", "C", "N", "Ho", "Wo"):
        assert warp(**{name: 0}) == -1, name
        assert warp(**{name: -3}) == -1, name
    assert warp(C=9) == -1
    assert warp(kind=2) == -1
    assert warp(Ws=(1 << 24) + 1) == -1
    assert warp(labels=p, S=3, labels_out=p, inside=None) == -1
    assert warp(labels=p, S=3, labels_out=None, inside=p) == -1
    assert warp(labels=p, S=0, labels_out=p, inside=p) == -1
    assert warp(labels=None, S=3) == -1
    aug = _lib.AugmentDesc(0.5, 0.5, 1, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0)
    assert lib.unetpp_augment_draw(None, 4, 1, 8, 8, 8, 8, ctypes.byref(aug), None) == -1
    assert lib.unetpp_augment_draw(p, 4, 1, 8, 8, 8, 8, None, None) == -1
    assert lib.unetpp_augment_draw(p, 0, 1, 8, 8, 8, 8, ctypes.byref(aug), None) == -1
    assert lib.unetpp_augment_draw(p, 4, 1, 8, 0, 8, 8, ctypes.byref(aug), None) == -1
    aug.scale_lo = 0.0
    assert lib.unetpp_augment_draw(p, 4, 1, 8, 8, 8, 8, ctypes.byref(aug), None) == -1
    assert ctypes.sizeof(_lib.AugmentDesc) == 48


def test_no_cpu_fallback_and_argument_errors():
    from unet_nested4tiny_objects_keypoints_amd import Augment, DeviceLoader, affine_params, ops, warp_batch
    store = torch.zeros(2, 8, 8, 1, dtype=torch.uint8)
    rows = affine_params([[1, 0, 0], [0, 1, 0]]).expand(2, 16).contiguous()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp_batch(store, torch.tensor([0, 1]), rows, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.warp_batch(store, torch.tensor([0, 1]), rows, (8, 8), torch.ones(1), torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceLoader(store, None, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Augment().draw(2, 0, (8, 8), (8, 8), "cpu")
    with pytest.raises(ValueError):
        Augment(scale=(0.0, 1.0))
    with pytest.raises(ValueError):
        Augment(flip_h=1.5)
    d = Augment(translate=(5, 4), contrast=(0.5, 1.5), brightness=0.1).desc()
    assert (d.max_tx, d.max_ty, d.gain_lo, d.gain_hi, d.rot90) == (5.0, 4.0, 0.5, 1.5, 1)


def test_draw_restatement_default_family_is_whole_numbers():
    got = lo.draw_ref(64, 12345, (24, 40), (24, 40), translate=(5, 5))
    rows = got["rows"]
    assert np.array_equal(rows[:, :12], np.round(rows[:, :12]))   # even sizes: the centre terms are whole, turned or not
    assert set(np.unique(got["q"])) == {0, 1, 2, 3} and got["flip_x"].any() and not got["flip_x"].all()
    assert np.abs(got["tx"]).max() <= 5 and np.abs(got["tx"]).max() >= 4
    u = lo.uniforms(12345, np.arange(64), 0)
    assert np.array_equal(u, np.float32(u).astype(np.float64)) and (u >= 0).all() and (u < 1).all()
