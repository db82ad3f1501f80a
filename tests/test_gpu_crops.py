"""Training on scenes (crops.py, csrc/crops.hip) on the GPU, against the restatement of tests/crops_oracle.py:
  (1) the target kernel against brute force over all labels: at most 1 float32 ulp per element down to the denormals
      (the bound tests/test_gpu_loss_targets.py holds single-point channels to: one exp and one sqrt in float64 on both
      sides, rounded to float32 once), exactly 0 where the restatement is 0, the same bits twice, every element written;
  (2) 300 coincident labels: the candidate list is filled past its size and emptied in rounds;
  (3) the draw kernel against its restatement, bit for bit;
  (4) end to end: image and target of a batch went through the same transform, a train step takes the batch, two
      objects with one seed give the same bits."""
import numpy as np
import pytest
import torch

from tests import crops_oracle as co
from tests.loss_oracle import ulps

pytestmark = pytest.mark.gpu

RADIUS = 3.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _target(case, C, size, radius, dev, prefill=None):
    from unet_nested4tiny_objects_keypoints_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    out = None
    if prefill is not None:
        out = torch.full((len(case["index"]), C, size[0], size[1]), prefill, dtype=torch.float32, device=dev)
    got = ops.points_target(t(case["labels"]), t(case["label_class"]), t(case["index"]), t(case["rows"]), C, size,
                            radius, out=out)
    return got.cpu().numpy()


def _hold(got, want, what):
    """exactly 0 where the restatement is 0, at most 1 ulp elsewhere; -> the worst ulp"""
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.isfinite(got).all(), what
    zero = want == 0
    assert np.array_equal(got[zero], want[zero]), (what, "not exactly 0 where the restatement is 0")
    worst = float(ulps(got[~zero], want[~zero]).max(initial=0.0))
    print("target ulps:", what, worst, "denormal elements:", int(((want > 0) & (want < 2.0 ** -126)).sum()))
    assert worst <= 1.0, (what, worst)
    return worst


# (1) -----------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 4, 40, 48), (2, 2, 33, 70), (1, 3, 129, 257)]


@pytest.mark.parametrize("L", [1, 7, 300])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_targets_against_brute_force(dev, shape, L):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    N, C, Ho, Wo = shape
    first = SHAPES.index(shape) + [1, 7, 300].index(L)       # over the nine cases every sample slot sees every transform
    case = co.target_case(N, C, Ho, Wo, L, first_kind=first)
    want = co.points_target_ref(case["labels"], case["label_class"], case["index"], case["rows"], C, (Ho, Wo), RADIUS)
    got = _target(case, C, (Ho, Wo), RADIUS, dev, prefill=float("nan"))   # a NaN left behind = an element not written
    assert _lib.lib().unetpp_last_kernel_name() == b"points_target"
    _hold(got, want, (shape, L, case["kinds"]))
    again = _target(case, C, (Ho, Wo), RADIUS, dev)
    assert np.array_equal(got.view(np.int32), again.view(np.int32))
    # what the label sets plant is there to be seen
    if N >= 3:
        assert not got[1].any()                               # an index outside [0, M): all-zero maps
    if C == 4:
        assert not got[:, 3].any()                            # a class without labels
    live = [n for n in range(N) if 0 <= case["index"][n] < N]
    plain = [n for n in live if case["kinds"][n] != "general"]     # unit scale: the planted distances are as planted
    if L >= 6:                                                # the lone far label: denormals and zeros, nothing else
        far = min(2, C - 1)
        assert all(want[n, far].max() < 2.0 ** -126 for n in live)
        assert all((want[n, far] > 0).any() for n in plain)
    for n in [n for n in plain if case["kinds"][n] == "identity"]:
        ax, ay = Wo // 3 + n, Ho // 2 - n
        if L >= 2:                                            # two labels two pixels apart: the pixel between is a tie
            assert got[n, 0, ay, ax] == 1.0 and got[n, 0, ay, ax + 2] == 1.0
        if L >= 2:
            assert want[n, 0, ay, ax + 1] == np.float32(np.exp(-0.5 / RADIUS))
        if L >= 5:                                            # the label landing at exactly (-1, -1) shines into the corner
            low = 1 if C >= 3 else 0
            assert got[n, low, 0, 0] >= np.float32(np.exp(-0.5 * np.sqrt(2.0) / RADIUS)) * (1 - 2.0 ** -23)


def test_a_second_class_group_and_a_small_grid(dev):
    """C = 6 takes two class groups per tile, classes 4 and 5 served by the second; with 8 usable CUs the grid is 64
    workgroups for the 90 (class group, tile) units, so workgroups take a second unit: the same bits as on the full grid"""
    from tests.helpers import usable_cus
    case = co.target_case(1, 2, 129, 257, 300, first_kind=3)
    cls = case["label_class"]
    case["label_class"] = np.where(cls == 1, 5, np.where(cls == 0, 4, cls)).astype(np.int32)   # 2 stays: now a live class
    want = co.points_target_ref(case["labels"], case["label_class"], case["index"], case["rows"], 6, (129, 257), RADIUS)
    got = _target(case, 6, (129, 257), RADIUS, dev, prefill=float("nan"))
    _hold(got, want, "C = 6")
    assert got[:, 4].any() and got[:, 2].any() and not got[:, [0, 1, 3]].any()
    with usable_cus(8):
        small = _target(case, 6, (129, 257), RADIUS, dev, prefill=float("nan"))
    assert np.array_equal(got.view(np.int32), small.view(np.int32))


# (2) -----------------------------------------------------------------------------------------------------------------
def test_coincident_labels_take_rounds(dev):
    N, C, Ho, Wo, L = 2, 2, 33, 70, 300
    labels = np.zeros((1, L, 2), dtype=np.float32)
    labels[0, :, 0], labels[0, :, 1] = co.X0 + 17.25, co.Y0 - 3.5
    labels[0, 299] = (co.X0 + 60.0, co.Y0 + 30.0)                 # one more, in the second chunk of 256 labels
    classes = np.zeros((1, L), dtype=np.int32)
    classes[0, 100:120] = 1
    rows = np.stack([co.window_row(k, (Ho, Wo)) for k in ("identity", "general")]).astype(np.float32)
    case = dict(labels=labels, label_class=classes, index=np.zeros(N, dtype=np.int64), rows=rows)
    want = co.points_target_ref(labels, classes, case["index"], rows, C, (Ho, Wo), RADIUS)
    got = _target(case, C, (Ho, Wo), RADIUS, dev, prefill=float("nan"))
    _hold(got, want, "coincident")
    assert got[0, 0, 30, 60] == 1.0


# (3) -----------------------------------------------------------------------------------------------------------------
def _draw(n, seed, M, src, size, frames, xy, p_object, jitter, aug, dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    f = torch.as_tensor(np.asarray(frames, dtype=np.int32)).to(dev) if len(frames) else None
    p = torch.as_tensor(np.asarray(xy, dtype=np.float32).reshape(-1, 2)).to(dev) if len(frames) else None
    rows, index, origin = ops.crops_draw(n, seed, M, src, size, f, p, p_object, jitter, aug.desc(), dev)
    return rows.cpu().numpy(), index.cpu().numpy(), origin.cpu().numpy()


CENTRES = ([0, 1, 2, 2, 0, 1, 2, 0, 1, 2, 1],
           [[0, 0], [89, 69], [40.4, 30.6], [12, 66], [45, 35], [3, 33], [88, 2], [20, 20], [60.5, 10.5], [30, 50],
            [75, 60]])


@pytest.mark.parametrize("src,size,table", [((70, 90), (32, 32), True), ((24, 40), (32, 32), True),
                                            ((70, 90), (32, 32), False)], ids=["clamp", "pad", "no-table"])
def test_draw_kernel_against_its_restatement(dev, src, size, table):
    from unet_nested4tiny_objects_keypoints_amd import Augment, _lib
    N, M, p_object, jitter = 257, 3, 0.6, (5, 7)              # more than one workgroup
    frames, xy = CENTRES if table else ([], [])
    exact = dict(flip_h=0.5, flip_v=0.3, rot90=size[0] == size[1], contrast=(0.5, 1.5), brightness=0.2)
    rows, index, origin = _draw(N, 77, M, src, size, frames, xy, p_object, jitter, Augment(**exact), dev)
    assert _lib.lib().unetpp_last_kernel_name() == b"crops_draw"
    ref = co.crops_draw_ref(N, 77, M, src, size, frames, xy, p_object, jitter, **exact)
    assert index.dtype == np.int64 and origin.dtype == np.int32
    assert np.array_equal(index, ref["index"]) and np.array_equal(origin, ref["origin"])
    want = ref["rows"]
    assert np.array_equal(rows[:, :12], want[:, :12]) and np.array_equal(rows[:, :12], np.round(rows[:, :12]))
    assert float(ulps(rows[:, 12], want[:, 12].astype(np.float32)).max()) <= 2
    assert float(ulps(rows[:, 13], want[:, 13].astype(np.float32)).max()) <= 2
    assert np.array_equal(rows[:, 14:], np.zeros((N, 2)))
    # the share of object windows is the restatement's count: the draw is deterministic
    share = int(ref["object"].sum())
    if table:
        assert 0.5 * N < share < 0.7 * N
        if src == (70, 90):
            assert (origin[:, 0] == 0).any() and (origin[:, 0] == 58).any() and (origin[:, 1] == 38).any()   # the clamp acted
            inside = (origin[:, 0] >= 0) & (origin[:, 0] <= 58) & (origin[:, 1] >= 0) & (origin[:, 1] <= 38)
            assert inside.all()
        else:
            assert (origin[:, 1] == -4).all()                 # a frame below the window: a centred pad
            assert (origin[:, 0] >= 0).all() and (origin[:, 0] <= 8).all() and (origin[:, 0] == 8).any()
    else:
        assert share == 0
    again = _draw(N, 77, M, src, size, frames, xy, p_object, jitter, Augment(**exact), dev)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip((rows, index, origin), again))
    other = _draw(N, 78, M, src, size, frames, xy, p_object, jitter, Augment(**exact), dev)
    assert not np.array_equal(rows, other[0])


def test_draw_object_share_and_table_frames(dev):
    """every object window reads a row of the table: its frame, and a centre within the jitter of it (before the clamp)"""
    from unet_nested4tiny_objects_keypoints_amd import Augment
    frames, xy = [1, 9], [[45.0, 35.0], [10.0, 10.0]]          # the second row names a frame that does not exist
    rows, index, origin = _draw(257, 3, 3, (70, 90), (32, 32), frames, xy, 0.6, (5, 7), Augment(), dev)
    ref = co.crops_draw_ref(257, 3, 3, (70, 90), (32, 32), frames, xy, 0.6, (5, 7))
    assert np.array_equal(index, ref["index"]) and np.array_equal(origin, ref["origin"])
    obj = ref["object"]
    assert int((index[obj] == -1).sum()) > 0 and set(np.unique(index[obj])) == {-1, 1}
    at = index == 1
    hit = obj & at
    assert (np.abs(origin[hit, 0] + 16 - 45) <= 5).all() and (np.abs(origin[hit, 1] + 16 - 35) <= 7).all()


# (4) -----------------------------------------------------------------------------------------------------------------
def _scene(dev):
    S, H, W, per = 2, 96, 112, 9
    rng = np.random.default_rng(8)
    frames = np.zeros((S, H, W, 1), dtype=np.uint8)
    labels = np.zeros((S, per, 2), dtype=np.float32)
    classes = np.zeros((S, per), dtype=np.int32)
    for s in range(S):
        flat = rng.choice(H * W, per, replace=False)
        labels[s, :, 0], labels[s, :, 1] = flat % W, flat // W
        labels[s, 0] = (0, 0) if s == 0 else (W - 1, H - 1)      # a corner: the clamp acts
        classes[s] = rng.integers(0, 2, per)
        frames[s, labels[s, :, 1].astype(int), labels[s, :, 0].astype(int), 0] = 255
    return frames, labels, classes


def _compose(frames, index, origin, row, size):
    """the window by torch ops: slice a zero-padded frame at the origin, turn, flip"""
    Ho, Wo = size
    a = np.round(row[6:12]).reshape(2, 3)[:, :2]
    for fx in (False, True):
        for fy in (False, True):
            for q in range(4):
                qc, qs = (1, 0, -1, 0)[q], (0, 1, 0, -1)[q]
                dx, dy = (-1 if fx else 1), (-1 if fy else 1)
                if np.array_equal(a, np.array([[dx * qc, -dx * qs], [dy * qs, dy * qc]])):
                    pad = max(Ho, Wo)
                    canvas = torch.nn.functional.pad(torch.from_numpy(frames[index, :, :, 0]).float(), (pad, pad, pad, pad))
                    w = canvas[origin[1] + pad:origin[1] + pad + Ho, origin[0] + pad:origin[0] + pad + Wo]
                    w = torch.rot90(w, -q, dims=(0, 1))
                    w = torch.flip(w, dims=(1,)) if fx else w
                    return torch.flip(w, dims=(0,)) if fy else w
    raise AssertionError("not a dihedral map: %r" % (a,))


def test_image_and_target_move_together_and_train(dev):
    from unet_nested4tiny_objects_keypoints_amd import AdamW, FocalLoss_BCE_2d, SceneCrops, UNet_Nested, train_step
    frames, labels, classes = _scene(dev)
    size, n = (32, 32), 24
    t = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731

    def make():
        return SceneCrops(t(frames), t(labels), t(classes), n_classes=2, crop=size, p_object=0.75, jitter=(6, 6),
                          radius=RADIUS, mul=1.0, seed=11)

    crops = make()
    assert crops.centre_frame.numel() == 18
    inputs, target, points, inside = crops.batch(n)
    rows, index, origin = (v.cpu().numpy() for v in crops.last)
    assert tuple(inputs.shape) == (n, 1, 32, 32) and tuple(target.shape) == (n, 2, 32, 32)
    assert tuple(points.shape) == (n, 9, 2) and tuple(inside.shape) == (n, 9) and inside.dtype == torch.uint8
    got_in, got_t = inputs.cpu(), target.cpu().numpy()
    pts, ins = points.cpu().numpy(), inside.cpu().numpy().astype(bool)
    assert set(np.unique(index)) <= {0, 1} and ins.any()
    for i in range(n):
        want = _compose(frames, int(index[i]), origin[i], rows[i], size)
        assert torch.equal(got_in[i, 0], want), i
    want_t = co.points_target_ref(labels, classes, index, rows, 2, size, RADIUS)
    _hold(got_t, want_t, "end to end")
    seen = 0
    for i in range(n):
        for l in np.flatnonzero(ins[i]):
            x, y = pts[i, l]
            assert x == round(x) and y == round(y)
            assert got_in[i, 0, int(y), int(x)] == 255.0 and got_t[i, classes[index[i], l], int(y), int(x)] == 1.0
            seen += 1
    assert seen >= n // 2

    net = UNet_Nested(in_channels=1, n_classes=2, feature_scale=8, depth=2).to(dev).train()
    opt = AdamW(net.parameters(), lr=1e-3)
    _, loss = train_step(net, opt, FocalLoss_BCE_2d(gamma=3, size_average=False), inputs, target)
    assert np.isfinite(float(loss.detach()))

    a, b = make(), make()
    for step, (ba, bb) in enumerate(zip(a.batches(8, 3), b.batches(8, 3))):
        for va, vb in zip(ba, bb):
            assert torch.equal(va.view(torch.uint8 if va.dtype == torch.uint8 else torch.int32),
                               vb.view(torch.uint8 if vb.dtype == torch.uint8 else torch.int32)), step
    first = make().batch(8)[0]
    assert not torch.equal(first, a.batch(8)[0])              # the fourth batch of `a` is another draw

    with pytest.raises(ValueError):
        crops.set_centres([0, 2], [[1.0, 1.0], [2.0, 2.0]])    # frame 2 of 2
    crops.set_centres([], torch.zeros(0, 2))
    crops.batch(4)
    assert int(crops.centre_frame.numel()) == 0
    crops.add_centres([1], [[50.0, 40.0]], repeat=3)
    assert crops.centre_frame.tolist() == [1, 1, 1]
