"""Copy-paste of tiny objects (crops.py: ObjectPaste, csrc/paste.hip) on the GPU, against tests/paste_oracle.py:
  (1) the draw against its restatement: all five outputs bit for bit, the same bits twice;
  (2) the pixels against their float32 restatement, bit for bit over the whole tensor (so nothing outside the accepted
      patches moves); with weight 1 everywhere a pasted patch is the warp of the source pixels, bit for bit;
  (3) the target merge: within 1 float32 ulp of the union brute force where that is non-zero and exactly 0 where it is 0
      (one exp and one sqrt in float64 on both sides, rounded to float32 once: the bound of tests/test_gpu_crops.py),
      untouched where a frame label is strictly nearer, negatives preserved, an all-void window untouched;
  (4) rows of any content are safe: unusable source rows come out void, and given to the pixel kernel change nothing;
  (5) end to end through SceneCrops;  (6) which launches a batch issues."""
import numpy as np
import pytest
import torch

from tests import paste_oracle as po
from tests.test_gpu_crops import _hold

pytestmark = pytest.mark.gpu

RADIUS = po.RADIUS
_SETS = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def sets(name):
    """an input set with the restatement's rows and pixels: computed once, shared, never modified"""
    if name not in _SETS:
        cs = po.case(name)
        rows = po.draw_of(cs)
        _SETS[name] = (cs, rows, po.apply_of(cs, rows))
    return _SETS[name]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _store(cs, dev):
    """the device store in the layout of its type: uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws]"""
    return _t(cs["store"].transpose(0, 2, 3, 1) if cs["u8"] else cs["store"], dev)


def _bits(a):
    return np.asarray(a).view(np.int32)


def _gpu_draw(cs, dev, **over):
    from unet_nested4tiny_objects_keypoints_amd import ops
    a = dict(cs, **over)
    got = ops.paste_draw(a["K"], a["seed"], _t(a["src_frame"], dev), _t(a["src_xy"], dev), _t(a["src_class"], dev),
                         _t(a["labels"], dev), _t(a["label_class"], dev), _t(a["index"], dev), _t(a["rows"], dev), a["C"],
                         (po.HS, po.WS), (a["Ho"], a["Wo"]), a["p"], a["R"], a["clearance"])
    return dict(zip(("src", "dst", "code", "xy", "cls"), (v.cpu().numpy() for v in got)))


def _gpu_apply(cs, rows, dev, alpha=None):
    from unet_nested4tiny_objects_keypoints_amd import ops
    x = _t(cs["inputs"], dev)
    out = ops.paste_apply(x, _t(rows["src"], dev), _t(rows["dst"], dev), _t(rows["code"], dev), _t(cs["src_frame"], dev),
                          _t(cs["src_xy"], dev), _t(cs["src_class"], dev), _store(cs, dev),
                          _t(cs["rows"], dev), _t(cs["mul"], dev), _t(cs["add"], dev),
                          _t(cs["alpha"] if alpha is None else alpha, dev), cs["C"])
    assert out is x
    return out.cpu().numpy()


# (1) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(po.CASES))
def test_draw_against_its_restatement(dev, name):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    cs, want, _ = sets(name)
    got = _gpu_draw(cs, dev)
    assert _lib.lib().unetpp_last_kernel_name() == b"paste_draw"
    for k in ("src", "dst", "code", "xy", "cls"):
        assert got[k].dtype == want[k].dtype and np.array_equal(_bits(got[k]), _bits(want[k])), (name, k)
    again = _gpu_draw(cs, dev)
    assert all(np.array_equal(_bits(got[k]), _bits(again[k])) for k in got)
    acc = want["src"] >= 0
    if cs["K"] == 4:                                          # the fixtures' condition: some accepted, some void
        assert acc.sum() >= 1 and (~acc).sum() >= 1
    if cs["N"] == 3:
        assert not (got["src"][1] >= 0).any() and (got["cls"][1] == -1).all()      # index -1
    off = _gpu_draw(cs, dev, p=0.0)
    assert (off["src"] == -1).all() and (off["cls"] == -1).all() and np.array_equal(off["dst"], want["dst"])
    other = _gpu_draw(cs, dev, seed=cs["seed"] + 1)
    assert not np.array_equal(other["dst"], want["dst"])


def test_every_code_is_accepted_somewhere():
    codes = set()
    for name in po.CASES:
        _, rows, _ = sets(name)
        codes |= set(rows["code"][rows["src"] >= 0].tolist())
    assert codes == set(range(8))


# (2) -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(po.CASES))
def test_pixels_against_their_restatement(dev, name):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    cs, rows, want = sets(name)
    got = _gpu_apply(cs, rows, dev)
    assert _lib.lib().unetpp_last_kernel_name() == (b"paste_apply_u8" if cs["u8"] else b"paste_apply_f32")
    assert np.array_equal(_bits(got), _bits(want)), name
    assert (got != cs["inputs"]).any() == (rows["src"] >= 0).any()
    assert np.array_equal(_bits(got), _bits(_gpu_apply(cs, rows, dev)))


@pytest.mark.parametrize("name", ["3x40x48-c1-u8-r4-k4-l7", "2x33x70-c3-f32-r4-k4-l300", "3x40x48-c3-u8-r1-k9-l1"])
def test_weight_one_is_the_warp_of_the_source_pixels(dev, name):
    """alpha == 1 everywhere, the identity code: the pasted patch equals ops.warp_batch of the source frame under the
    exact translation that carries the source centre to the destination centre, with the window's gain and bias"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    from unet_nested4tiny_objects_keypoints_amd.crops import paste_alpha
    cs, rows, _ = sets(name)
    R, (Ho, Wo) = cs["R"], (cs["Ho"], cs["Wo"])
    ones = np.ones((2 * R + 1, 2 * R + 1), dtype=np.float32)
    if R == 1:
        ones = paste_alpha(1, 1.49).numpy()                   # core just under R + 0.5: the table itself is all ones
        assert (ones == 1.0).all()
    plain = dict(rows, code=np.zeros_like(rows["code"]))
    got = _gpu_apply(cs, plain, dev, alpha=ones)
    seen = 0
    for n, k in zip(*np.nonzero(rows["src"] >= 0)):
        t = rows["src"][n, k]
        px, py = rows["dst"][n, k]
        cx, cy = np.floor(cs["src_xy"][t].astype(np.float64) + 0.5)
        row = np.zeros((1, 16), dtype=np.float32)
        row[0, [0, 4, 6, 10]] = 1.0
        row[0, 2], row[0, 5], row[0, 8], row[0, 11] = cx - px, cy - py, px - cx, py - cy
        row[0, 12:14] = cs["rows"][n, 12:14]
        warped = ops.warp_batch(_store(cs, dev), _t(np.array([cs["src_frame"][t]], dtype=np.int64), dev), _t(row, dev),
                                (Ho, Wo), _t(cs["mul"], dev), _t(cs["add"], dev), 0.0).cpu().numpy()
        box = (slice(None), slice(py - R, py + R + 1), slice(px - R, px + R + 1))
        assert np.array_equal(_bits(got[n][box]), _bits(warped[0][box])), (name, n, k)
        seen += 1
    assert seen >= 1


# (3) -----------------------------------------------------------------------------------------------------------------
def _frame_target(cs, dev, prefill=None):
    """the frame's own target of an input set (ops.points_target), or a tensor of that shape filled with `prefill`"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    if prefill is not None:
        return torch.full((cs["N"], cs["C"], cs["Ho"], cs["Wo"]), prefill, dtype=torch.float32, device=dev)
    return ops.points_target(_t(cs["labels"], dev), _t(cs["label_class"], dev), _t(cs["index"], dev), _t(cs["rows"], dev),
                             cs["C"], (cs["Ho"], cs["Wo"]), RADIUS)


@pytest.mark.parametrize("name", list(po.CASES))
def test_target_merge_against_the_union_brute_force(dev, name):
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    cs, rows, _ = sets(name)
    xy, cls = _t(rows["xy"], dev), _t(rows["cls"], dev)
    size = (cs["Ho"], cs["Wo"])
    want, m_frame, m_paste = po.union_target_ref(cs["labels"], cs["label_class"], cs["index"], cs["rows"], cs["C"], size,
                                                 RADIUS, rows["xy"], rows["cls"])
    target = _frame_target(cs, dev)
    before = target.cpu().numpy()
    assert ops.paste_target(target, xy, cls, RADIUS) is target
    assert _lib.lib().unetpp_last_kernel_name() == b"paste_target"
    got = target.cpu().numpy()
    _hold(got, want, (name, "union"))
    nearer = m_frame < m_paste                                # a frame label is strictly nearer: not an element moves
    assert nearer.any() or cs["L"] == 1
    assert np.array_equal(_bits(got[nearer]), _bits(before[nearer]))
    assert (got != before).any() == (rows["src"] >= 0).any()
    again = _frame_target(cs, dev)
    ops.paste_target(again, xy, cls, RADIUS)
    assert np.array_equal(_bits(got), _bits(again.cpu().numpy()))

    # negatives preserved on a target the ignore launch marked
    rects, rect_class, mask = po.ignore_rects(cs)
    marked = _frame_target(cs, dev)
    ops.target_ignore(marked, _t(rects, dev), _t(rect_class, dev), _t(cs["index"], dev), _t(cs["rows"], dev), (po.HS, po.WS))
    assert np.array_equal(marked.cpu().numpy() == -1.0, mask) and mask.any()
    ops.paste_target(marked, xy, cls, RADIUS)
    kept = marked.cpu().numpy()
    assert (kept[mask] == -1.0).all()
    assert np.array_equal(_bits(kept[~mask]), _bits(got[~mask]))

    # a window whose slots are all void is untouched, not even read: NaNs stay
    nans = _frame_target(cs, dev, prefill=float("nan"))
    pattern = _bits(nans.cpu().numpy()).copy()
    ops.paste_target(nans, xy, cls, RADIUS)
    after = nans.cpu().numpy()
    void = ~(rows["src"] >= 0).any(axis=1)
    if cs["N"] == 3:
        assert void[1]
    assert np.array_equal(_bits(after[void]), pattern[void])
    zeros = torch.zeros_like(nans)                            # and on a zero target every live class map is written
    ops.paste_target(zeros, xy, cls, RADIUS)
    z = zeros.cpu().numpy()
    for n in range(cs["N"]):
        for c in range(cs["C"]):
            assert (z[n, c] > 0).any() == bool((rows["cls"][n] == c).any())


def test_more_units_than_workgroups(dev):
    """72 windows (an input set 24 times over) on 8 usable CUs: 64 workgroups for 72 draws, 648 patches and 216 tiles, so
    workgroups take further units -- the same bits as on the full grid, and the draw is still the restatement's"""
    from tests.helpers import usable_cus
    from unet_nested4tiny_objects_keypoints_amd import ops
    cs, _, _ = sets("3x40x48-c3-f32-r4-k9-l300")
    big = dict(cs, N=72, index=np.tile(cs["index"], 24), rows=np.tile(cs["rows"], (24, 1)),
               inputs=np.tile(cs["inputs"], (24, 1, 1, 1)))
    want = po.draw_of(big)
    assert (want["src"] >= 0).sum() > 24

    def run():
        rows = _gpu_draw(big, dev)
        target = ops.paste_target(_frame_target(big, dev), _t(rows["xy"], dev), _t(rows["cls"], dev), RADIUS)
        return rows, _gpu_apply(big, rows, dev), target.cpu().numpy()

    full = run()
    with usable_cus(8):
        small = run()
    assert all(np.array_equal(_bits(full[0][k]), _bits(want[k])) for k in want)
    assert all(np.array_equal(_bits(full[0][k]), _bits(small[0][k])) for k in want)
    assert np.array_equal(_bits(full[1]), _bits(small[1])) and np.array_equal(_bits(full[2]), _bits(small[2]))
    assert (full[1] != big["inputs"]).any()


# (4) -----------------------------------------------------------------------------------------------------------------
def test_unusable_rows_are_void_and_change_nothing(dev):
    """rows 8..11 of the source table: a frame out of range, a patch off the frame, a class >= C, a NaN.  Every one is
    handled by a guard of the kernels; none relies on an access out of range."""
    cs, _, _ = sets("3x40x48-c3-f32-r4-k9-l300")
    bad = dict(cs, src_frame=cs["src_frame"][8:], src_xy=cs["src_xy"][8:], src_class=cs["src_class"][8:])
    got = _gpu_draw(bad, dev)
    want = po.draw_of(bad)
    assert (got["src"] == -1).all() and (got["cls"] == -1).all() and (got["xy"] == -1).all()
    assert all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in got)
    N, K, R = cs["N"], cs["K"], cs["R"]
    rows = dict(src=np.zeros((N, K), dtype=np.int32), dst=np.full((N, K, 2), 12, dtype=np.int32),
                code=np.zeros((N, K), dtype=np.int32))
    rows["src"][:] = np.arange(N * K).reshape(N, K) % 4 + 8                       # the four unusable rows
    assert np.array_equal(_bits(_gpu_apply(cs, rows, dev)), _bits(cs["inputs"]))
    rows["src"][:] = np.array([-1, 12, 2 ** 31 - 1, -2 ** 31])[np.arange(N * K).reshape(N, K) % 4]   # no row of the table
    assert np.array_equal(_bits(_gpu_apply(cs, rows, dev)), _bits(cs["inputs"]))
    rows["src"][:] = 0                                                            # a good row, but ...
    rows["code"][:] = np.array([8, -1, 2 ** 31 - 1])[np.arange(N * K).reshape(N, K) % 3]            # ... no such code
    assert np.array_equal(_bits(_gpu_apply(cs, rows, dev)), _bits(cs["inputs"]))
    rows["code"][:] = 0
    edge = [(R - 1, 12), (12, R - 1), (cs["Wo"] - R, 12), (12, cs["Ho"] - R), (-5, -5), (2 ** 31 - 1, 12), (12, -2 ** 31)]
    rows["dst"][:] = np.array(edge)[np.arange(N * K).reshape(N, K) % len(edge)]   # ... a patch that leaves the window
    assert np.array_equal(_bits(_gpu_apply(cs, rows, dev)), _bits(cs["inputs"]))
    assert np.array_equal(_bits(po.apply_of(cs, rows)), _bits(cs["inputs"]))
    rows["dst"][:] = (R, cs["Ho"] - 1 - R)                                        # the last place that fits: it pastes
    one = dict(src=rows["src"][:, :1], dst=rows["dst"][:, :1], code=rows["code"][:, :1])
    got = _gpu_apply(cs, one, dev)
    assert np.array_equal(_bits(got), _bits(po.apply_of(cs, one))) and (got != cs["inputs"]).any()


# (5), (6) ------------------------------------------------------------------------------------------------------------
def _scene():
    rng = np.random.default_rng(21)
    S, per = 2, 12
    frames = rng.integers(0, 256, (S, po.HS, po.WS, 1), dtype=np.uint8)
    gx, gy = np.meshgrid(np.arange(4) * 30 + 15, np.arange(3) * 28 + 16)          # twelve objects, far apart
    labels = np.stack([gx.ravel(), gy.ravel()], axis=1)[None].repeat(S, 0).astype(np.float32)
    labels += rng.uniform(-0.45, 0.45, labels.shape).astype(np.float32)           # off the pixel grid
    classes = rng.integers(0, 2, (S, per)).astype(np.int32)
    return frames, labels, classes


def test_end_to_end(dev):
    from unet_nested4tiny_objects_keypoints_amd import (AdamW, Augment, FocalLoss_BCE_2d, IgnoreRegions, ObjectPaste,
                                                        SceneCrops, UNet_Nested, _lib, train_step)
    frames, labels, classes = _scene()
    size, n, C, R, K = (40, 48), 6, 2, 2, 4
    name = lambda: _lib.lib().unetpp_last_kernel_name()   # noqa: E731

    def make(paste=None, **kw):
        return SceneCrops(_t(frames, dev), _t(labels, dev), _t(classes, dev), n_classes=C, crop=size, p_object=0.75,
                          jitter=(6, 6), radius=RADIUS, seed=13, paste=paste,
                          augment=Augment(rot90=False, contrast=(0.5, 1.5), brightness=0.2), **kw)

    def pasting(p):
        return ObjectPaste(max_pastes=K, p=p, patch_radius=R, core=1.0, clearance=5.0)

    plain, off, on = make(), make(pasting(0.0)), make(pasting(1.0))
    assert plain.last_paste is None and plain.paste is None
    ps = on.paste
    table = po.source_table_ref(labels, classes, C, (po.HS, po.WS), R)
    assert len(table[0]) == 24
    for got, want in zip((ps.src_frame, ps.src_xy, ps.src_class), table):
        assert np.array_equal(got.cpu().numpy(), want)
    taken = void = 0
    for step in range(3):
        b_plain = plain.batch(n)
        assert name() == b"points_target"                     # (6) never a paste launch without paste
        b_off = off.batch(n)
        assert name() == b"paste_target"                      # (6) the last launch of a pasting batch
        b_on = on.batch(n)
        assert name() == b"paste_target"
        for a, b in zip(b_plain, b_off):                      # p = 0: the bits of an object without paste
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), step
        assert all(torch.equal(a, b) for a, b in zip(plain.last, off.last))
        assert (off.last_paste.src == -1).all()
        rows, index, origin = (v.cpu().numpy() for v in on.last)
        assert np.array_equal(_bits(rows), _bits(plain.last[0].cpu().numpy()))    # the same windows
        pr = {k: v.cpu().numpy() for k, v in on.last_paste._asdict().items()}
        taken += int((pr["src"] >= 0).sum())
        void += int((pr["src"] < 0).sum())
        # the pixels: the restatement applied to the p = 0 inputs of the same seed
        store = frames.transpose(0, 3, 1, 2)
        pix = po.paste_apply_ref(b_plain[0].cpu().numpy(), pr["src"], pr["dst"], pr["code"], table[0], table[1], table[2],
                                 store, rows, on.mul.cpu().numpy(), on.add.cpu().numpy(), ps.alpha.cpu().numpy(), C)
        assert np.array_equal(_bits(b_on[0].cpu().numpy()), _bits(pix)), step
        assert torch.equal(b_on[2], b_plain[2]) and torch.equal(b_on[3], b_plain[3])   # points, inside: the frame's labels
        union, _, _ = po.union_target_ref(labels, classes, index, rows, C, size, RADIUS, pr["xy"], pr["cls"])
        _hold(b_on[1].cpu().numpy(), union, ("end to end", step))
        # the rows are the restatement's for the paste's seed: the batch's seed xor the constant
        seeds = torch.Generator().manual_seed(13)
        for _ in range(step + 1):
            seed = int(torch.randint(0, 2 ** 62, (1,), generator=seeds, dtype=torch.int64))
        from unet_nested4tiny_objects_keypoints_amd.crops import _PASTE_SEED
        want = po.paste_draw_ref(n, K, seed ^ _PASTE_SEED, table[0], table[1], table[2], labels, classes, index, rows, C,
                                 (po.HS, po.WS), size, 1.0, R, 5.0)
        assert all(np.array_equal(_bits(pr[k]), _bits(want[k])) for k in want), step

    assert taken >= 1 and void >= 1
    inputs, target = b_on[0], b_on[1]
    net = UNet_Nested(in_channels=1, n_classes=C, feature_scale=8, depth=2).to(dev).train()
    opt = AdamW(net.parameters(), lr=1e-3)
    _, loss = train_step(net, opt, FocalLoss_BCE_2d(gamma=3, size_average=False), inputs, target)
    assert np.isfinite(float(loss.detach()))

    a, b = make(pasting(1.0)), make(pasting(1.0))             # two objects with one seed: the same bits
    for step in range(2):
        for va, vb in zip(a.batch(n), b.batch(n)):
            assert torch.equal(va.view(torch.uint8), vb.view(torch.uint8)), step
        assert all(torch.equal(x, y) for x, y in zip(a.last_paste, b.last_paste))

    # ignore regions: the left 70 columns of every frame; sources come from outside them, patches land anywhere
    ign = IgnoreRegions(torch.tensor([[[0.0, 0.0, 69.0, po.HS - 1.0]]] * 2))
    with_ign, without = make(pasting(1.0), ignore=ign), make(None, ignore=ign)
    assert int(with_ign.paste.src_frame.numel()) == 12 and float(with_ign.paste.src_xy[:, 0].min()) > 69.0
    hit = 0
    for step in range(3):
        t_on = with_ign.batch(n)[1].cpu().numpy()
        assert name() == b"target_ignore"
        t_off = without.batch(n)[1].cpu().numpy()
        assert np.array_equal(t_on == -1.0, t_off == -1.0)     # ignoring wins over a pasted label as over any other
        pr = {k: v.cpu().numpy() for k, v in with_ign.last_paste._asdict().items()}
        for i, k in zip(*np.nonzero(pr["src"] >= 0)):
            px, py = pr["dst"][i, k]
            patch = t_on[i, :, py - R:py + R + 1, px - R:px + R + 1]
            if (t_off[i, :, py, px] == -1.0).all():
                assert (patch[:, R, R] == -1.0).all()
                hit += 1
    assert hit >= 1                                           # a patch did land inside a rectangle

    with pytest.raises(ValueError):
        on.paste.set_sources([0, 2], [[20.0, 20.0], [30.0, 30.0]], [0, 1])        # frame 2 of 2
    with pytest.raises(ValueError):
        on.paste.set_sources([0], [[20.0, 20.0]], [C])
    with pytest.raises(ValueError):
        on.paste.set_sources([], torch.zeros(0, 2), [])
    on.paste.set_sources([1], [[20.25, 30.5]], [1])
    on.batch(n)
    pr = on.last_paste
    assert set(pr.src.cpu().unique().tolist()) <= {-1, 0} and set(pr.cls.cpu().unique().tolist()) == {-1, 1}
    with pytest.raises(ValueError):                           # the window is smaller than the patch
        SceneCrops(_t(frames, dev), _t(labels, dev), _t(classes, dev), n_classes=C, crop=(8, 48), paste=ObjectPaste())
    with pytest.raises(ValueError):                           # no label can be pasted: every one has a close neighbour
        SceneCrops(_t(frames, dev), _t(np.float32([[[20, 20], [22, 21]]] * 2), dev), _t(np.int32([[0, 1]] * 2), dev),
                   n_classes=C, crop=size, paste=ObjectPaste(patch_radius=2, core=1.0))

