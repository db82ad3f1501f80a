"""The validation step on the device (validate.py, Heatmap.match_points / match_distmin, csrc/validate.hip).

The matcher is pinned against a NumPy restatement of its rule (float32 differences, float64 squares, greedy global
minimum over (d, label position, prediction index)) and of the landmark loss in the kernel's summation order; the whole
step against synthetic heads with a known answer and against the composition of the existing per-head calls."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PATTERN = [[0], [1, 2, 3], [4], [5, 6]]
THREADS = 256   # partial sums of a head: csrc/validate.hip kMatchThreads


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------- NumPy restatement
def np_match(points, found, labels, pattern, heads):
    """points [heads*N*C, K, 2] f32, found [heads*N*C], labels [N, S, 2] f32 -> matched, mask, loss [heads] f32, count"""
    points, labels = np.asarray(points, np.float32), np.asarray(labels, np.float32)
    n_img, s = labels.shape[:2]
    c, k = len(pattern), points.shape[1]
    matched = np.full((heads, n_img, s, 2), -1.0, np.float32)
    mask = np.zeros((heads, n_img, s), bool)
    loss, count = np.zeros(heads, np.float32), np.zeros(heads, np.int32)
    for h in range(heads):
        part = np.zeros(THREADS, np.float64)
        for m in range(n_img * c):
            n, ci = divmod(m, c)
            g = h * n_img * c + m
            p = min(max(int(found[g]), 0), k)
            labs = pattern[ci]
            if p == 0 or not labs:
                continue
            t = labels[n, labs]                                   # [L, 2]
            dx = (points[g, None, :p, 0] - t[:, None, 0]).astype(np.float32)
            dy = (points[g, None, :p, 1] - t[:, None, 1]).astype(np.float32)
            d = dx.astype(np.float64) * dx.astype(np.float64) + dy.astype(np.float64) * dy.astype(np.float64)  # [L, P]
            free = d.copy()
            for _ in range(min(len(labs), p)):
                i, j = np.unravel_index(int(np.argmin(free)), free.shape)   # first minimum in (i, j) order
                matched[h, n, labs[i]] = points[g, j]
                mask[h, n, labs[i]] = True
                part[m % THREADS] += d[i, j]
                count[h] += 1
                free[i, :] = np.inf
                free[:, j] = np.inf
        step = THREADS // 2
        while step:
            part[:step] += part[step:2 * step]
            step //= 2
        with np.errstate(invalid="ignore", divide="ignore"):
            loss[h] = np.float32(part[0] / (2.0 * float(count[h])))
    return matched, mask, loss, count


def same_bits(a, b):
    """float32 arrays equal bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a.view(np.int32)[~nan] == b.view(np.int32)[~nan]).all())


def _random_case(rng):
    heads = int(rng.integers(1, 4))
    n = int(rng.choice([1, 2, 3, 7, 16, 64]))
    c = int(rng.integers(1, 5))
    lens = [int(rng.integers(1, 9)) for _ in range(c)]
    s = sum(lens) + int(rng.integers(0, 5))                   # labels that no map holds
    order = rng.permutation(s)
    pattern, at = [], 0
    for ln in lens:
        pattern.append([int(v) for v in order[at:at + ln]])
        at += ln
    k = int(rng.integers(1, 11))                              # up to 10 predictions: more than the labels of a map
    ties = rng.random() < 0.5
    if ties:   # integer predictions, half-pixel labels in a small window: exact distance ties
        points = rng.integers(0, 6, (heads * n * c, k, 2)).astype(np.float32)
        labels = (rng.integers(0, 6, (n, s, 2)) + 0.5).astype(np.float32)
    else:
        points = rng.uniform(0, 64, (heads * n * c, k, 2)).astype(np.float32)
        labels = rng.uniform(0, 64, (n, s, 2)).astype(np.float32)
    found = rng.integers(0, k + 1, heads * n * c).astype(np.int32)   # 0, fewer and more than the labels
    found[rng.random(found.shape) < 0.1] = 0
    return heads, pattern, points, found, labels


def _run(dev, heads, pattern, points, found, labels):
    from unet_nested4tiny_objects_keypoints_amd import ops
    got = ops.match_points(torch.from_numpy(points).to(dev), torch.from_numpy(found).to(dev),
                           torch.from_numpy(labels).to(dev), pattern, heads=heads)
    return [t.cpu().numpy() for t in got]


def test_matcher_equals_numpy_restatement(dev):
    rng = np.random.default_rng(2026)
    ties = empty = 0
    for _ in range(300):
        case = _random_case(rng)
        matched, mask, loss, count = _run(dev, *case)
        want = np_match(case[2], case[3], case[4], case[1], case[0])
        np.testing.assert_array_equal(matched, want[0])
        np.testing.assert_array_equal(mask, want[1])
        np.testing.assert_array_equal(count, want[3])
        assert same_bits(loss, want[2]), (loss, want[2])
        assert (np.isnan(loss) == (count == 0)).all()
        empty += int((count == 0).sum())
        ties += int(float(case[4][0, 0, 0]) % 1 == 0.5)
    assert empty > 0 and ties > 50


def test_greedy_differs_from_each_label_taking_its_nearest(dev):
    # both labels are nearest to prediction 0; the closer pair (label 1, d = 1) takes it, label 0 gets prediction 1
    labels = np.array([[[0, 0], [3, 0]]], np.float32)
    points = np.array([[[2, 0], [10, 0]]], np.float32)
    matched, mask, loss, count = _run(dev, 1, [[0, 1]], points, np.array([2], np.int32), labels)
    assert matched[0, 0].tolist() == [[10, 0], [2, 0]] and mask.all() and count[0] == 2
    assert loss[0] == np.float32((1 + 100) / 4)


def test_three_way_tie_goes_by_label_position_then_prediction_index(dev):
    # map [2, 0]: label 2 at position 0, label 0 at position 1; label 1 is in no map.  Pairs at d = 1: (pos 0, p0),
    # (pos 0, p1), (pos 1, p0).  Label position first: label 2 (not the lower label index 0); prediction index next: p0.
    labels = np.array([[[2, 0], [10, 10], [0, 0]]], np.float32)
    points = np.array([[[1, 0], [0, 1]]], np.float32)
    matched, mask, loss, count = _run(dev, 1, [[2, 0]], points, np.array([2], np.int32), labels)
    assert matched[0, 0].tolist() == [[0, 1], [-1, -1], [1, 0]]
    assert mask[0, 0].tolist() == [True, False, True] and count[0] == 2
    assert loss[0] == np.float32((1 + 5) / 4)
    # no prediction at all: nothing matched, loss NaN
    matched, mask, loss, count = _run(dev, 1, [[2, 0]], points, np.array([0], np.int32), labels)
    assert (matched == -1).all() and not mask.any() and count[0] == 0 and np.isnan(loss[0])


def test_match_distmin_is_one_row_of_match_points(dev):
    from unet_nested4tiny_objects_keypoints_amd import Heatmap
    rng = np.random.default_rng(5)
    hm = Heatmap(PATTERN, 64, 64)
    points = torch.from_numpy(rng.integers(0, 64, (3, 4, 3, 2)).astype(np.float32)).to(dev)
    found = torch.from_numpy(rng.integers(0, 4, (3, 4)).astype(np.int32)).to(dev)
    targets = torch.from_numpy(rng.uniform(0, 64, (3, 8, 2)).astype(np.float32)).to(dev)
    matched, mask = hm.match_points(points, found, targets)
    assert matched.shape == (3, 8, 2) and mask.dtype == torch.bool and not mask[:, 7].any()
    for n in range(3):
        for c, idx in enumerate(PATTERN):
            preds = points[n, c, :int(found[n, c])].cpu().tolist()
            got = hm.match_distmin(preds, targets[n].cpu().tolist(), idx)
            assert got == matched[n, idx].cpu().tolist()
    assert hm.match_distmin([], [[1.0, 2.0]], [0]) == [[-1.0, -1.0]]


# ------------------------------------------------------------------------------------------- the whole step
def _spread_labels(rng, n, s, size):
    """integer labels on a 24-px grid (>= 20 px apart after a +-2 jitter), >= 14 px from the frame"""
    cells = [(x, y) for x in range(16, size - 15, 24) for y in range(16, size - 15, 24)]
    out = np.zeros((n, s, 2), np.float32)
    for b in range(n):
        pick = rng.choice(len(cells), s, replace=False)
        out[b] = np.array([cells[i] for i in pick], np.float32) + rng.integers(-2, 3, (s, 2))
    return out


def test_synthetic_heads_with_a_known_answer(dev):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, Heatmap, validate_outputs
    rng = np.random.default_rng(7)
    size = 128
    hm = Heatmap(PATTERN, size, size)
    labels = _spread_labels(rng, 2, 7, size)
    shifts = [(0, 0), (1, -2), (-3, 1), (2, 2)]
    heads = [hm.create_heatmap(labels + np.array(sh, np.float32)) for sh in shifts]
    lx, ly = (labels[1, 2] + np.array(shifts[3], np.float32)).astype(int)   # image 1, label 2 (map 1) of the last head
    heads[3][1, 1, max(ly - 12, 0):ly + 13, max(lx - 12, 0):lx + 13] = 0
    lab = torch.from_numpy(labels).to(dev)
    res = validate_outputs(tuple(heads), FocalLoss_BCE_2d(gamma=3, size_average=False), hm, lab)
    for h, (sx, sy) in enumerate(shifts):
        want = labels + np.array([sx, sy], np.float32)
        mask = res.mask[h].cpu().numpy()
        if h < 3:
            assert mask.all() and int(res.matched_count[h]) == 14
        else:
            assert not mask[1, 2] and mask.sum() == 13 and int(res.matched_count[h]) == 13
            want[1, 2] = -1
        np.testing.assert_array_equal(res.points[h].cpu().numpy(), want)
        assert float(res.landmark_losses[h]) == (sx * sx + sy * sy) / 2
    assert res.heatmap_losses.shape == (4,) and float(res.heatmap_losses[0]) < float(res.heatmap_losses[1])


def _net(dev, depth, bf16, plain=False):
    from unet_nested4tiny_objects_keypoints_amd import UNet, UNet_Nested
    torch.manual_seed(depth)
    if plain:
        return UNet(n_classes=4, n_channels=3, widths=(8, 16, 32, 64, 64)).to(dev).eval()
    m = UNet_Nested(in_channels=3, n_classes=4, feature_scale=4, depth=depth).to(dev).eval()
    if bf16:
        m.set_activation_dtype(torch.bfloat16)
    return m


def _batch(dev, n=3):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 3, 64, 64, generator=g).to(dev)
    labels = (torch.rand(n, 8, 2, generator=g) * 48 + 8).to(dev)     # label 7 is in no map
    return x, labels


@pytest.mark.parametrize("depth,bf16,plain", [(4, False, False), (3, False, False), (4, True, False), (3, True, False),
                                              (4, False, True)])
def test_validate_step_is_the_composition_of_existing_calls(dev, depth, bf16, plain):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, Heatmap, validate_step
    m = _net(dev, depth, bf16, plain)
    hm = Heatmap(PATTERN, 64, 64)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    x, labels = _batch(dev)
    buffers = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref_outs = m(x)
    ref_outs = ref_outs if isinstance(ref_outs, tuple) else (ref_outs,)
    thr = 0.5
    res = validate_step(m, crit, hm, x, labels, threshold=thr)
    outs = res.outputs if isinstance(res.outputs, tuple) else (res.outputs,)
    assert len(outs) == len(ref_outs) == res.heatmap_losses.shape[0]
    target = hm.create_heatmap(labels)
    pts, fnd = [], []
    for h, (o, r) in enumerate(zip(outs, ref_outs)):
        assert o.dtype == torch.float32 and torch.equal(o, r)
        assert torch.equal(res.heatmap_losses[h], crit(r, target).reshape(()))
        points, found = hm.transfer_points(r, threshold=thr)
        matched, mask = hm.match_points(points, found, labels)
        assert torch.equal(res.points[h], matched) and torch.equal(res.mask[h], mask)
        pts.append(points.cpu().numpy().reshape(-1, points.shape[2], 2))
        fnd.append(found.cpu().numpy().reshape(-1))
    want = np_match(np.concatenate(pts), np.concatenate(fnd), labels.cpu().numpy(), PATTERN, len(outs))
    assert same_bits(res.landmark_losses.cpu().numpy(), want[2])
    np.testing.assert_array_equal(res.matched_count.cpu().numpy(), want[3])
    assert int(res.matched_count.sum()) > 0
    for k, v in m.state_dict().items():   # eval: BatchNorm running statistics untouched
        assert torch.equal(v, buffers[k]), k
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        validate_step(m, crit, hm, x, labels)


def test_one_extraction_over_stacked_heads_is_per_head_extraction(dev, monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, Heatmap, ops, validate_step
    m = _net(dev, 4, False)
    hm = Heatmap(PATTERN, 64, 64)
    x, labels = _batch(dev)
    with torch.no_grad():
        outs = m(x)
    stacked = torch.stack(outs).view(-1, 64, 64)
    all_pts, all_cnt = ops.keypoints_extract(stacked, 3, 0.5)
    for h, o in enumerate(outs):
        pts, cnt = ops.keypoints_extract(o.reshape(-1, 64, 64), 3, 0.5)
        sl = slice(h * pts.shape[0], (h + 1) * pts.shape[0])
        assert torch.equal(all_pts[sl], pts) and torch.equal(all_cnt[sl], cnt)
    calls = []
    real = ops.keypoints_extract

    def counted(*a, **k):
        calls.append(a[0].shape)
        return real(*a, **k)
    monkeypatch.setattr(ops, "keypoints_extract", counted)
    validate_step(m, FocalLoss_BCE_2d(), hm, x, labels)
    assert calls == [torch.Size([len(outs) * 3 * 4, 64, 64])]


def test_validate_step_is_deterministic(dev):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, Heatmap, validate_step
    m = _net(dev, 4, False)
    hm = Heatmap(PATTERN, 64, 64)
    x, labels = _batch(dev, n=8)
    a = validate_step(m, FocalLoss_BCE_2d(), hm, x, labels)
    b = validate_step(m, FocalLoss_BCE_2d(), hm, x, labels)
    for fa, fb in zip(a, b):
        for ta, tb in zip(fa if isinstance(fa, tuple) else (fa,), fb if isinstance(fb, tuple) else (fb,)):
            assert torch.equal(ta, tb) or same_bits(ta.cpu().numpy(), tb.cpu().numpy())


def test_validate_step_with_GraphedForward_equals_eager(dev):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, GraphedForward, Heatmap, validate_step
    m = _net(dev, 4, False)
    hm = Heatmap(PATTERN, 64, 64)
    crit = FocalLoss_BCE_2d()
    x, labels = _batch(dev, n=1)
    eager = validate_step(m, crit, hm, x, labels)
    graphed = validate_step(m, crit, hm, x, labels, forward=GraphedForward(m, x))
    for fe, fg in zip(eager, graphed):
        for te, tg in zip(fe if isinstance(fe, tuple) else (fe,), fg if isinstance(fg, tuple) else (fg,)):
            assert torch.equal(te, tg) or same_bits(te.cpu().numpy(), tg.cpu().numpy())
