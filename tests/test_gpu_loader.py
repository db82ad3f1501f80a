"""The device input pipeline (loader.py, csrc/loader.hip) on the GPU, against the float64 restatement of
tests/loader_oracle.py:
  (1) identity rows copy bit for bit;  (2) the dihedral maps with shifts, crops and pads equal torch's flip / rot90 /
  roll bit for bit;  (3) row tails and a misaligned output inside guard words;  (4) general maps inside the derived
  bound, uint8 and float32 stores;  (5) labels;  (6) image and labels move together under drawn rows;  (7) the draw
  kernel against its restatement;  (8) an out-of-range index;  (9) offsets past 2^31;  (10) DeviceLoader.

The bound of (3) and (4) is derived, not measured (tests/test_loader_host.py states it and checks an fp32 emulation
against it): in source units dx Dx + dy Dy + 8u Vmax with dx = 4u (|m0| xo + |m1| yo + |m2|), u = 2^-24, and for the
output |gain mul[c]| bound_v + 4u (|out| + |gain add[c]| + |bias|)."""
import numpy as np
import pytest
import torch

from tests import loader_oracle as lo
from tests.helpers import bound_ratio, report_ratio

pytestmark = pytest.mark.gpu

GUARD = 4
GUARD_BITS = 0x7FC0BEEF       # a NaN payload no arithmetic here produces
FILL = 7.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), torch.as_tensor(b).contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.float().view(torch.int32))


def _rows(rows64, dev):
    """float64 rows -> (the fp32 rows the kernel gets on the device, the same values as float64 for the restatement)"""
    r32 = torch.from_numpy(np.asarray(rows64)).float()
    return r32.to(dev), r32.double().numpy()


def _nchw(store):
    s = store.cpu()
    return (s.permute(0, 3, 1, 2) if s.dtype == torch.uint8 else s).numpy()


# (1) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
def test_identity_copies_bit_for_bit(dev, C):
    from unet_nested4tiny_objects_keypoints_amd import _lib, affine_params, warp_batch
    g = torch.Generator().manual_seed(C)
    store = torch.randint(0, 256, (3, 8, 12, C), dtype=torch.uint8, generator=g).to(dev)
    index = torch.tensor([2, 0, 2], device=dev)
    rows = affine_params([[1, 0, 0], [0, 1, 0]]).expand(3, 16).contiguous().to(dev)
    got = warp_batch(store, index, rows, (8, 12), mul=1, add=0)
    assert _lib.lib().unetpp_last_kernel_name() == b"warp_u8"
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (3, C, 8, 12)
    assert torch.equal(got, store[index].permute(0, 3, 1, 2).float())
    f32 = store.permute(0, 3, 1, 2).float().contiguous()       # the same through the float32 store layout
    got = warp_batch(f32, index, rows, (8, 12))
    assert _lib.lib().unetpp_last_kernel_name() == b"warp_f32"
    assert torch.equal(got, f32[index])


# (2) -----------------------------------------------------------------------------------------------------------------
SHIFTS = [(0, 0), (3, -5), (-30, 2)]   # the last is mostly out of frame


@pytest.mark.parametrize("out_size", ["turned", (16, 20), (32, 52)], ids=["same", "crop", "pad"])
def test_dihedral_maps_are_bitwise_permutations(dev, out_size):
    from unet_nested4tiny_objects_keypoints_amd import warp_batch
    Hs, Ws, C = 24, 40, 2
    store = torch.randint(0, 256, (2, Hs, Ws, C), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    imgs = store.permute(0, 3, 1, 2).float()
    for odd in (0, 1):   # a quarter turn of a 24x40 frame fills 40x24: one launch per output size
        size = ((Ws, Hs) if odd else (Hs, Ws)) if out_size == "turned" else out_size
        cases = [(fx, q, t) for fx, q in lo.DIHEDRAL if q % 2 == odd for t in SHIFTS]
        index = [i % 2 for i in range(len(cases))]
        rows, _ = _rows(lo.dihedral_rows(cases, (Hs, Ws), size), dev)
        got = warp_batch(store.to(dev), torch.tensor(index, device=dev), rows, size, fill=FILL).cpu()
        for n, (fx, q, t) in enumerate(cases):
            want = lo.dihedral_torch(imgs[index[n]], fx, q, t, size, FILL)
            assert _bits_equal(got[n], want), (fx, q, t, size)
        assert float((got == FILL).float().mean()) < 0.9 and bool((got != FILL).any())   # something was in frame


# (3) -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def general(dev):
    """64 general maps on a uint8 [4, 48, 80, 3] store, shared by (3), (4) and (5): per-channel mul / add that differ,
    gain 0.5 to 1.5, bias +-0.2, fill 7."""
    rng = np.random.default_rng(17)
    store = torch.from_numpy(rng.integers(0, 256, (4, 48, 80, 3), dtype=np.uint8))
    index = rng.integers(0, 4, 64)
    mul, add = [1 / 255.0, 1 / 128.0, 1 / 64.0], [-0.5, 0.25, 0.0]
    return dict(store=store, index=index, mul=mul, add=add,
                mul32=np.float32(mul).astype(np.float64), add32=np.float32(add).astype(np.float64))


@pytest.mark.parametrize("Wo", [13, 20])
def test_row_tails_and_a_misaligned_output(dev, general, Wo):
    from unet_nested4tiny_objects_keypoints_amd import ops
    N, C, Ho = 5, 3, 9
    rows, rows64 = _rows(lo.random_rows(np.random.default_rng(Wo), N, (48, 80), (Ho, Wo)), dev)
    store, index = general["store"].to(dev), torch.tensor(general["index"][:N], device=dev)
    mul = torch.tensor(general["mul"], device=dev)
    add = torch.tensor(general["add"], device=dev)
    numel = N * C * Ho * Wo
    buf = torch.empty(GUARD + 1 + numel + GUARD, dtype=torch.float32, device=dev)
    buf.view(torch.int32).fill_(GUARD_BITS)
    out = buf[GUARD + 1:GUARD + 1 + numel].view(N, C, Ho, Wo)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4
    got = ops.warp_batch(store, index, rows, (Ho, Wo), mul, add, FILL, out=out)
    assert got.data_ptr() == out.data_ptr()
    bits = buf.view(torch.int32).cpu()
    assert bool((bits[:GUARD + 1] == GUARD_BITS).all()) and bool((bits[GUARD + 1 + numel:] == GUARD_BITS).all())
    aligned = ops.warp_batch(store, index, rows, (Ho, Wo), mul, add, FILL)      # 16-byte stores where the rows allow
    assert aligned.data_ptr() % 16 == 0
    assert _bits_equal(got, aligned.cpu())
    want, bound = lo.warp_batch_ref(_nchw(store), general["index"][:N], rows64, (Ho, Wo), general["mul32"],
                                    general["add32"], FILL)
    ratio = bound_ratio(got, want, bound)
    report_ratio("tails Wo=%d" % Wo, "warp", ratio)
    assert ratio <= 1.0


# (4) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size", [(64, 64), (32, 52)], ids=["64x64", "32x52"])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_general_maps_stay_inside_the_bound(dev, general, kind, out_size):
    from unet_nested4tiny_objects_keypoints_amd import warp_batch
    rng = np.random.default_rng(23 + out_size[1])
    rows, rows64 = _rows(lo.random_rows(rng, 64, (48, 80), out_size), dev)
    if kind == "u8":
        store = general["store"]
    else:
        store = torch.randn(4, 3, 48, 80, generator=torch.Generator().manual_seed(4))
    index = general["index"]
    got = warp_batch(store.to(dev), torch.from_numpy(index).to(dev), rows, out_size, mul=general["mul"],
                     add=general["add"], fill=FILL)
    assert tuple(got.shape) == (64, 3) + out_size
    want, bound = lo.warp_batch_ref(_nchw(store), index, rows64, out_size, general["mul32"], general["add32"], FILL)
    ratio = bound_ratio(got, want, bound)
    report_ratio("general %s %dx%d" % ((kind,) + out_size), "warp", ratio)
    assert ratio <= 1.0
    # the maps resample: a kernel that copies, or ignores the rows, is nowhere near
    assert float(np.abs(want[1:] - want[:-1]).max()) > 0.1


# (5) -----------------------------------------------------------------------------------------------------------------
def test_labels_follow_the_forward_map(dev, general):
    from unet_nested4tiny_objects_keypoints_amd import warp_batch
    rng = np.random.default_rng(31)
    M, S, N, size = 4, 9, 64, (32, 52)
    labels = np.stack([rng.uniform(0, 79, (M, S)), rng.uniform(0, 47, (M, S))], axis=-1).astype(np.float32)
    labels[0, 2] = labels[3, 0] = (-1.0, -1.0)       # the "none" sentinel
    labels[1, 4] = (-1.0, 5.0)                         # one negative coordinate is a sentinel too
    labels[2, 1] = (0.0, 0.0)                          # the frame corner is a label, not a sentinel
    rows, rows64 = _rows(lo.random_rows(rng, N, (48, 80), size, shift=6.0), dev)
    index = general["index"]
    want, inside, bound, margin = lo.labels_ref(labels, index, rows64, size)
    assert float(margin.min()) >= 1e-3, float(margin.min())     # a condition on these inputs, not a tolerance
    assert inside.any() and not inside.all()
    _, got, got_inside = warp_batch(general["store"].to(dev), torch.from_numpy(index).to(dev), rows, size,
                                    labels=torch.from_numpy(labels).to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, S, 2)
    assert got_inside.dtype == torch.uint8 and tuple(got_inside.shape) == (N, S)
    got = got.cpu().double().numpy()
    is_none = (labels[index][..., 0] < 0) | (labels[index][..., 1] < 0)
    assert np.array_equal(got[is_none], np.full((int(is_none.sum()), 2), -1.0))
    assert not got_inside.cpu().numpy()[is_none].any()
    ratio = float((np.abs(got - want)[~is_none] / bound[~is_none]).max())
    report_ratio("labels", "forward map", ratio)
    assert ratio <= 1.0
    assert np.array_equal(got_inside.cpu().numpy().astype(bool), inside)


# (6) -----------------------------------------------------------------------------------------------------------------
def test_image_and_labels_move_together(dev):
    from unet_nested4tiny_objects_keypoints_amd import Augment, warp_batch
    rng = np.random.default_rng(41)
    M, S, N, side = 4, 6, 32, 40
    labels = np.full((M, S, 2), -1.0, dtype=np.float32)
    store = torch.zeros(M, side, side, 1, dtype=torch.uint8)
    for m in range(M):
        spots = rng.permutation(side * side)[:S - 1]          # distinct pixels; the last label stays "none"
        spots[0] = 2 * side + 1 + m                            # one near the edge: a shift of up to 5 can push it out
        for s, p in enumerate(spots):
            labels[m, s] = (p % side, p // side)
            store[m, p // side, p % side, 0] = 255
    aug = Augment(translate=(5, 5))
    rows = aug.draw(N, 2024, (side, side), (side, side), dev)
    index = torch.arange(N, device=dev) % M
    out, pts, inside = warp_batch(store.to(dev), index, rows, (side, side), labels=torch.from_numpy(labels).to(dev))
    out, pts, inside = out.cpu(), pts.cpu(), inside.cpu().bool()
    assert bool(((out == 0) | (out == 255)).all())
    assert torch.equal((out == 255).sum(dim=(1, 2, 3)), inside.sum(dim=1))
    assert not bool(inside[:, S - 1].any()) and bool((pts[:, S - 1] == -1).all())
    assert 0 < int(inside.sum()) and int((~inside[:, :S - 1]).sum()) > 0     # both kinds occur in this draw
    for n in range(N):
        for s in range(S - 1):
            x, y = pts[n, s].tolist()
            assert x == int(x) and y == int(y)
            if inside[n, s]:
                assert out[n, 0, int(y), int(x)] == 255, (n, s)
            else:
                assert not (0 <= x <= side - 1 and 0 <= y <= side - 1), (n, s)


# (7) -----------------------------------------------------------------------------------------------------------------
def _ulps(got, want64):
    want = np.float32(want64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def test_draw_kernel_against_its_restatement(dev):
    from unet_nested4tiny_objects_keypoints_amd import Augment, _lib
    N, src, size = 257, (24, 40), (32, 52)      # more than one workgroup
    exact = dict(flip_h=0.5, flip_v=0.3, rot90=True, translate=(5, 7), contrast=(0.5, 1.5), brightness=0.2)
    got = Augment(**exact).draw(N, 77, src, size, dev)
    assert _lib.lib().unetpp_last_kernel_name() == b"augment_draw"
    got = got.cpu().numpy()
    ref = lo.draw_ref(N, 77, src, size, **exact)
    want = ref["rows"]
    # no rotation, unit scale, even sizes: whole numbers, so flips, quarter turns and shifts are the restatement's exactly
    assert np.array_equal(got[:, :12], want[:, :12]) and np.array_equal(got[:, :12], np.round(got[:, :12]))
    assert len(set(zip(ref["flip_x"], ref["flip_y"], ref["q"]))) == 16 and np.abs(ref["ty"]).max() == 7
    assert float(_ulps(got[:, 12], want[:, 12]).max()) <= 2 and float(_ulps(got[:, 13], want[:, 13]).max()) <= 2
    assert np.array_equal(got[:, 14:], np.zeros((N, 2)))
    again = Augment(**exact).draw(N, 77, src, size, dev).cpu().numpy()
    assert np.array_equal(got.view(np.int32), again.view(np.int32))
    other = Augment(**exact).draw(N, 78, src, size, dev).cpu().numpy()
    assert not np.array_equal(got, other)

    general = dict(exact, rotate=30.0, scale=(0.5, 2.0))
    got = Augment(**general).draw(N, 5, src, size, dev).cpu().numpy()
    want = lo.draw_ref(N, 5, src, size, **general)["rows"]
    tol = 2 * 2.0 ** -23 * np.maximum(1.0, np.abs(want[:, :12]))
    err = np.abs(got[:, :12].astype(np.float64) - want[:, :12])
    report_ratio("draw", "matrix entries", float((err / tol).max()))
    assert bool((err <= tol).all())
    assert float(_ulps(got[:, 12], want[:, 12]).max()) <= 2 and float(_ulps(got[:, 13], want[:, 13]).max()) <= 2
    det = want[:, 0] * want[:, 4] - want[:, 1] * want[:, 3]       # 1 / s^2 up to the flips' sign
    assert 0.25 <= float(np.abs(det).min()) < 0.5 and 2.0 < float(np.abs(det).max()) <= 4.0   # scales 0.5 .. 2 were drawn


# (8) -----------------------------------------------------------------------------------------------------------------
def test_out_of_range_index_is_an_all_fill_sample(dev):
    from unet_nested4tiny_objects_keypoints_amd import affine_params, warp_batch
    M, S = 3, 4
    store = torch.randint(1, 256, (M, 8, 12, 2), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    labels = torch.rand(M, S, 2).mul(7).to(dev)
    rows = affine_params([[1, 0, 0], [0, 1, 0]], gain=1.5, bias=0.25).expand(3, 16).contiguous().to(dev)
    index = torch.tensor([-1, M, 1], device=dev)
    out, pts, inside = warp_batch(store, index, rows, (8, 12), mul=[0.5, 0.25], add=[1.0, -1.0], fill=FILL, labels=labels)
    want = torch.tensor([1.5 * (FILL * 0.5 + 1.0) + 0.25, 1.5 * (FILL * 0.25 - 1.0) + 0.25])
    assert torch.equal(out[:2].cpu(), want.view(1, 2, 1, 1).expand(2, 2, 8, 12))
    assert bool((pts[:2] == -1).all()) and not bool(inside[:2].any())
    assert torch.equal(out[2].cpu(), 1.5 * (store[1].permute(2, 0, 1).float().cpu() * want.new_tensor([0.5, 0.25]).view(2, 1, 1)
                                            + want.new_tensor([1.0, -1.0]).view(2, 1, 1)) + 0.25)
    assert torch.equal(pts[2], labels[1]) and bool(inside[2].all())


# (9) -----------------------------------------------------------------------------------------------------------------
def test_store_offsets_are_64_bit(dev):
    from unet_nested4tiny_objects_keypoints_amd import affine_params, warp_batch
    M = 524_800                                   # x 64 x 64 bytes = 2.15 GB: the last sample starts past 2^31
    store = torch.empty((M, 64, 64, 1), dtype=torch.uint8, device=dev)     # not filled
    assert (M - 1) * 64 * 64 > 2 ** 31
    g = torch.Generator().manual_seed(6)
    first = torch.randint(0, 256, (64, 64, 1), dtype=torch.uint8, generator=g)
    last = torch.randint(0, 256, (64, 64, 1), dtype=torch.uint8, generator=g)
    store[0], store[M - 1] = first.to(dev), last.to(dev)
    rows = affine_params([[1, 0, 0], [0, 1, 0]]).expand(2, 16).contiguous().to(dev)
    got = warp_batch(store, torch.tensor([M - 1, 0], device=dev), rows, (64, 64), mul=1).cpu()
    assert torch.equal(got[0, 0], last[..., 0].float()) and torch.equal(got[1, 0], first[..., 0].float())
    del store


# (10) ----------------------------------------------------------------------------------------------------------------
def _numbered(dev, M=10, side=8):
    store = torch.arange(M, dtype=torch.uint8).view(M, 1, 1, 1).expand(M, side, side, 1).contiguous().to(dev)
    labels = torch.rand(M, 3, 2, generator=torch.Generator().manual_seed(3)).mul(side - 1).to(dev)
    return store, labels


def test_device_loader_epochs(dev):
    from unet_nested4tiny_objects_keypoints_amd import Augment, DeviceLoader
    store, labels = _numbered(dev)

    def epochs(seed):
        ld = DeviceLoader(store, labels, (8, 8), mul=1.0, augment=Augment(), seed=seed)
        assert len(ld) == 10
        return [[tuple(t.cpu() for t in b) for b in ld.epoch(4, shuffle=True, drop_last=False)] for _ in range(2)]

    a, b, c = epochs(5), epochs(5), epochs(6)
    for ep in a:
        assert [int(x.shape[0]) for x, _, _ in ep] == [4, 4, 2]
        seen = torch.cat([x[:, 0, 0, 0] for x, _, _ in ep])
        assert all(bool((x == x[:, :1, :1, :1]).all()) for x, _, _ in ep)     # a permutation of a constant image
        assert sorted(seen.tolist()) == list(range(10))                       # every sample once
    for ea, eb in zip(a, b):                                                   # one seed: identical epochs
        for ta, tb in zip(ea, eb):
            assert all(torch.equal(x, y) for x, y in zip(ta, tb))
    order = lambda eps: [torch.cat([x[:, 0, 0, 0] for x, _, _ in ep]).tolist() for ep in eps]   # noqa: E731
    assert order(a)[0] != order(a)[1] or order(a) != order(c)                 # the order is drawn, per epoch and seed
    plain = DeviceLoader(store, labels, (8, 8), mul=1.0)                      # no augmentation: one launch, identity
    x, pts, inside = next(iter(plain.epoch(5, shuffle=False)))
    assert torch.equal(x[:, 0, 0, 0].cpu(), torch.arange(5.0)) and torch.equal(pts, labels[:5]) and bool(inside.all())
    assert len(list(plain.epoch(4))) == 2
    x, none, none2 = DeviceLoader(store, None, (12, 6), mul=1.0, fill=99).batch([9, 3])   # a centred pad / crop
    assert none is None and none2 is None and tuple(x.shape) == (2, 1, 12, 6)
    assert bool((x[0, 0, 2:10] == 9).all()) and bool((x[:, 0, :2] == 99).all()) and bool((x[:, 0, 10:] == 99).all())


def test_device_loader_feeds_a_training_step(dev):
    from unet_nested4tiny_objects_keypoints_amd import (AdamW, Augment, DeviceLoader, FocalLoss_BCE_2d, Heatmap,
                                                        UNet_Nested, train_step)
    torch.manual_seed(12)
    M, S = 8, 3
    images = torch.randint(0, 256, (M, 40, 40, 1), dtype=torch.uint8).to(dev)
    labels = torch.rand(M, S, 2).mul(24).add(8).to(dev)
    loader = DeviceLoader(images, labels, (32, 32), augment=Augment(translate=(3, 3), contrast=(0.8, 1.2)), seed=1)
    model = UNet_Nested(in_channels=1, n_classes=2, feature_scale=8).to(dev).train()
    opt = AdamW(model.parameters(), lr=1e-2, weight_decay=1e-4)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    hm = Heatmap([[0, 1], [2]], 32, 32)
    before = [p.detach().clone() for p in model.parameters()]
    inputs, pts, inside = next(iter(loader.epoch(4)))
    assert tuple(inputs.shape) == (4, 1, 32, 32) and float(inputs.min()) >= 0.0 and float(inputs.max()) <= 1.2001
    target = hm.create_heatmap(pts)
    assert tuple(target.shape) == (4, 2, 32, 32) and float(target.max()) > 0
    _, loss = train_step(model, opt, crit, inputs, target)
    assert bool(torch.isfinite(loss))
    assert any(not torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
