"""Cascaded scene inference on the GPU (scene.py CascadeSceneInference, csrc/scene.hip unetpp_scene_screen).

(a) unetpp_scene_screen alone, bit for bit against the numpy restatement (tests/cascade_oracle.py): active as ints, score
    through view(int32).  Maps [2, 3, 70, 90] (rows of 90 floats: the 16-byte boundaries sit elsewhere in every second
    row); the plan's rectangles with margin 0 and 10, 1x1 / one-row / one-column rectangles, one starting at x = 2 mod 4
    with a ragged width, the whole frame, padding rows; planted: a maximum equal to the threshold, one a step below it, a
    NaN, all NaN, +inf, and -0.0 against a threshold of 0.0.  With everything outside the rectangles of a second call
    turned into NaN the results do not move (nothing outside a rectangle is read); a third call returns the same bits.
(b) 64-bit offsets: a frame map of 47000 x 47000 (2.2e9 elements, never filled), four rectangles in its bottom-right corner.
(c) CascadeSceneInference end to end on the depth-3 network and the 2 x 96 x 112 frames of tests/test_gpu_scene.py:
    out == where(A, D, M1) bit for bit with the threshold ON a tile's score; -inf / +inf; margin 0, flips, the ensemble;
    graphed against eager; detect and audit.
"""
import numpy as np
import pytest
import torch

from tests.cascade_oracle import owner_mask, screen_ref, screen_rects
from tests.test_scene_host import oracle64, rect_rows

pytestmark = pytest.mark.gpu

MUL = 1.0 / 255.0
PAD = (-1, 0, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def run_screen(maps, rects, threshold):
    from unet_nested4tiny_objects_keypoints_amd import ops
    table = ops.scene_rects(rects)
    active, score = ops.scene_screen(maps, table, table.to(maps.device), threshold)
    assert active.dtype == torch.int32 and score.dtype == torch.float32 and active.shape == score.shape == (len(rects),)
    return active.cpu().numpy(), score.cpu().numpy()


def assert_equals_ref(got, maps, rects, threshold):
    want_active, want_score = screen_ref(maps.cpu().numpy(), rects, threshold)
    assert got[0].tolist() == want_active.tolist()
    assert got[1].view(np.int32).tolist() == want_score.view(np.int32).tolist()


# ------------------------------------------------------------------------------------------------ (a)
THR = 0.75
# planted rectangles of frame 1, six rows apart: (y_lo, y_hi, x_lo, x_hi) = (8 i, 8 i + 6, 1, 12)
EQUAL, BELOW, ONE_NAN, ALL_NAN, PLUS_INF, MINUS_ZERO = range(6)


def planted_rect(i):
    return (1, 0, 0, 8 * i, 8 * i + 6, 1, 12)


def screen_case(dev):
    S, C, H, W = 2, 3, 70, 90
    g = torch.Generator().manual_seed(77)
    m = torch.randn(S, C, H, W, generator=g)
    thr = torch.tensor(THR, dtype=torch.float32)
    below = torch.nextafter(thr, torch.tensor(float("-inf")))
    for i in (EQUAL, BELOW, ONE_NAN, PLUS_INF):
        _, _, _, y0, y1, x0, x1 = planted_rect(i)
        m[1, :, y0:y1, x0:x1] = m[1, :, y0:y1, x0:x1].clamp_max(THR - 0.5)
    m[1, 2, 3, 7] = thr
    m[1, 0, 8 + 5, 11] = below
    m[1, 1, 16 + 2, 1] = float("nan")
    m[1, :, 24:30, 1:12] = float("nan")
    m[1, 2, 32, 4] = float("inf")
    m[1, :, 40:46, 1:12] = -m[1, :, 40:46, 1:12].abs() - 0.125
    m[1, 0, 41, 6] = -0.0
    plan0 = screen_rects(H, W, 32, 10, 2, 0, S)
    plan10 = screen_rects(H, W, 32, 10, 2, 10, S)
    assert len(plan0) == 2 * 5 * 6 and any(r[5] % 4 == 2 for r in plan0) and plan10 != plan0
    special = [(0, 0, 0, 5, 6, 7, 8),            # 1 x 1
               (1, 0, 0, 13, 14, 3, 88),         # one row
               (0, 0, 0, 2, 69, 41, 42),         # one column
               (1, 0, 0, 47, 66, 6, 19),         # starts at x = 2 mod 4, 13 wide
               (0, 0, 0, 0, H, 0, W),            # the whole frame
               PAD, PAD]
    planted = [planted_rect(i) for i in range(6)]
    return m.to(dev), plan0, plan10, special, planted


def test_screen_equals_the_numpy_restatement(dev):
    m, plan0, plan10, special, planted = screen_case(dev)
    rects = plan0 + plan10 + special + planted
    got = run_screen(m, rects, THR)
    assert_equals_ref(got, m, rects, THR)
    active, score = got[0][-6:], got[1][-6:]
    thr = np.float32(THR)
    assert active.tolist() == [1, 0, 1, 1, 1, 0]
    assert score[EQUAL] == thr and score[BELOW] == np.nextafter(thr, np.float32(-np.inf)) and score[BELOW] < thr
    assert np.isfinite(score[ONE_NAN]) and score[ONE_NAN] < thr and not np.isnan(got[1]).any()
    assert score[ALL_NAN] == -np.inf and score[PLUS_INF] == np.inf
    pads = slice(len(rects) - 8, len(rects) - 6)
    assert got[0][pads].tolist() == [0, 0] and (got[1][pads] == -np.inf).all()
    # -0.0 against a threshold of 0.0: !(-0.0 < 0.0), so the tile is active; its maximum is the -0.0 itself
    zero = run_screen(m, rects, 0.0)
    assert_equals_ref(zero, m, rects, 0.0)
    assert zero[0][-6:].tolist() == [1, 1, 1, 1, 1, 1]
    assert zero[1][-1] == 0.0 and np.signbit(zero[1][-1]) and np.signbit(got[1][-1])
    # a third run of the first call: the same bits
    again = run_screen(m, rects, THR)
    assert again[0].tolist() == got[0].tolist() and again[1].view(np.int32).tolist() == got[1].view(np.int32).tolist()
    # nothing but padding rows: nothing is launched, and the answer is still "inactive, -inf"
    none = run_screen(m, [PAD, PAD, PAD], THR)
    assert none[0].tolist() == [0, 0, 0] and (none[1] == -np.inf).all()
    from unet_nested4tiny_objects_keypoints_amd import ops
    for bad in ([(0, 0, 0, 0, 71, 0, 90)], [(2, 0, 0, 0, 8, 0, 8)], [(0, 0, 0, 8, 8, 0, 8)]):
        with pytest.raises(RuntimeError, match="invalid argument"):
            run_screen(m, bad, THR)
    with pytest.raises(ValueError, match="NaN"):
        run_screen(m, plan0, float("nan"))
    with pytest.raises(ValueError):
        ops.scene_screen(m[0], ops.scene_rects(plan0), ops.scene_rects(plan0).to(dev), THR)


def test_screen_reads_nothing_outside_its_rectangles(dev):
    m, plan0, plan10, special, planted = screen_case(dev)
    first = plan0 + plan10 + special + planted
    got = run_screen(m, first, THR)
    keep = list(range(0, len(plan0), 2)) + [2 * len(plan0) + i for i in range(4)] + \
        [len(first) - 6 + i for i in range(6)]                    # every second owned rectangle, the small ones, the planted
    rects = [first[i] for i in keep]
    inside = torch.zeros(m.shape[0], 1, m.shape[2], m.shape[3], dtype=torch.bool, device=dev)
    for (s, _, _, y0, y1, x0, x1) in rects:
        inside[s, :, y0:y1, x0:x1] = True
    assert 0.3 < float(inside.float().mean()) < 0.8
    poisoned = torch.where(inside, m, torch.full_like(m, float("nan")))
    second = run_screen(poisoned, rects, THR)
    assert second[0].tolist() == got[0][keep].tolist()
    assert second[1].view(np.int32).tolist() == got[1][keep].view(np.int32).tolist()
    assert_equals_ref(second, poisoned, rects, THR)


# ------------------------------------------------------------------------------------------------ (b)
def test_screen_offsets_beyond_2_31_elements(dev):
    side, tile, halo, align = 47000, 64, 8, 2
    maps = torch.empty(1, 1, side, side, device=dev)                   # 8.8 GB, never filled
    assert maps.numel() > 2 ** 31
    from unet_nested4tiny_objects_keypoints_amd.scene import plan_tiles
    rows, cols = plan_tiles(side, side, tile, halo, align)
    corner = [(0, oy, ox, max(y0 - halo, oy), min(y1 + halo, oy + tile), max(x0 - halo, ox), min(x1 + halo, ox + tile))
              for (oy, y0, y1) in rows[-2:] for (ox, x0, x1) in cols[-2:]]            # margin = halo, clipped to the tile
    assert len(corner) == 4 and max(r[4] for r in corner) == side and max(r[6] for r in corner) == side
    y_min, x_min = min(r[3] for r in corner), min(r[5] for r in corner)
    assert (y_min * side + x_min) > 2 ** 31
    g = torch.Generator(device=dev).manual_seed(9)
    for r in corner:
        maps[0, :, r[3]:r[4], r[5]:r[6]] = torch.randn(1, r[4] - r[3], r[6] - r[5], generator=g, device=dev)
    small = maps[:, :, y_min:, x_min:].contiguous()
    shifted = [(s, 0, 0, y0 - y_min, y1 - y_min, x0 - x_min, x1 - x_min) for (s, _, _, y0, y1, x0, x1) in corner]
    thr = float(np.sort(screen_ref(small.cpu().numpy(), shifted, 0.0)[1])[2])     # a tile's own score: equality is live
    got = run_screen(maps, corner, thr)
    assert_equals_ref(got, small, shifted, thr)
    assert 1 <= got[0].sum() <= 4
    del maps
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ (c)
H0, W0, TILE0, HEAD0, S0, CHUNK0, HALO0, ALIGN0 = 96, 112, 64, 2, 2, 5, 24, 4
KW = dict(tile=TILE0, chunk=CHUNK0, mul=MUL)


@pytest.fixture(scope="module")
def case(dev):
    """the model and frames of tests/test_gpu_scene.py, the shallow map M1 and the deep maps D of plain SceneInference
    objects -- computed once and left unchanged"""
    from unet_nested4tiny_objects_keypoints_amd import SceneInference, UNet_Nested
    _, ctor, state = oracle64(3, 8)
    model = UNet_Nested(**ctor)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(41)
    u8 = torch.randint(0, 256, (S0, H0, W0, 1), generator=g, dtype=torch.uint8).to(dev)
    M1 = SceneInference(model, head=1, **KW)(u8)
    deep = {"plain": SceneInference(model, head=HEAD0, **KW)(u8),
            "flips": SceneInference(model, head=HEAD0, tta="flips", **KW)(u8),
            "ensemble": SceneInference(model, head=HEAD0, ensemble=True, **KW)(u8)}
    owned = rect_rows(H0, W0, TILE0, HALO0, ALIGN0, S0)
    return dict(model=model, u8=u8, M1=M1, M1_np=M1.cpu().numpy(), deep=deep, owned=owned)


def reference(case, margin, threshold=None):
    """(threshold, active, score) of the numpy restatement on M1; threshold None: the (upper) median tile score, itself
    a tile's score, so the equality case is live"""
    rects = screen_rects(H0, W0, TILE0, HALO0, ALIGN0, margin, S0)
    if threshold is None:
        score = screen_ref(case["M1_np"], rects, 0.0)[1]
        threshold = float(np.sort(score)[len(score) // 2])
    active, score = screen_ref(case["M1_np"], rects, threshold)
    return threshold, active, score


def expected(case, active, which="plain"):
    A = torch.from_numpy(owner_mask(case["owned"], active, S0, H0, W0)).to(case["M1"].device)
    return torch.where(A, case["deep"][which], case["M1"])


def check_call(cascade, case, active, score, which="plain"):
    got = cascade(case["u8"])
    assert cascade.last_active.dtype == torch.bool and cascade.last_active.tolist() == [bool(a) for a in active]
    assert cascade.last_scores.is_cuda
    assert cascade.last_scores.cpu().numpy().view(np.int32).tolist() == score.view(np.int32).tolist()
    assert cascade.last_fraction == float(active.sum()) / len(active)
    assert cascade.last_forwards == -(-int(active.sum()) // CHUNK0)
    assert same_bits(got, expected(case, active, which))
    return got


def test_cascade_equals_where_active_deep_else_shallow(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import CascadeSceneInference
    thr, active, score = reference(case, HALO0)
    n = len(active)
    print("cascade: %d of %d tiles reach the median score %.9g" % (active.sum(), n, thr))
    assert n == 24 and 0 < active.sum() < n and (score == np.float32(thr)).any()
    cascade = CascadeSceneInference(case["model"], head=HEAD0, screen_head=1, threshold=thr, **KW)
    assert cascade.margin == HALO0
    got = check_call(cascade, case, active, score)
    assert not same_bits(got, case["deep"]["plain"]) and not same_bits(got, case["M1"])
    assert same_bits(cascade(case["u8"]), got)                          # the cached plan
    assert same_bits(cascade(case["u8"][1]), got[1:2])                  # one frame without the leading axis
    # -inf: every tile is active, the result is D; +inf: none is, the result is M1 and the deep model never runs
    cascade.threshold = float("-inf")
    _, all_on, score_inf = reference(case, HALO0, float("-inf"))
    assert all_on.all()
    assert same_bits(check_call(cascade, case, all_on, score_inf), case["deep"]["plain"])
    cascade.threshold = float("inf")
    _, none_on, _ = reference(case, HALO0, float("inf"))
    assert not none_on.any()
    from unet_nested4tiny_objects_keypoints_amd import ops
    timer = ops.LaunchTimer()
    ops.set_timer(timer)
    try:
        got = check_call(cascade, case, none_on, score_inf)
    finally:
        ops.set_timer(None)
    assert same_bits(got, case["M1"]) and cascade.last_forwards == 0 and cascade.last_fraction == 0.0
    kinds = [k[0] for k in timer.launches]
    n_screen = -(-len(rect_rows(H0, W0, TILE0, 12, ALIGN0, S0)) // CHUNK0)      # the screen stage's own forwards
    assert kinds.count("scene_screen") == 1 and kinds.count("scene_stitch") == kinds.count("warp_batch") == n_screen


def test_cascade_margin_zero_flips_and_ensemble(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import CascadeSceneInference
    thr, active, score = reference(case, 0)
    assert 0 < active.sum() < len(active)
    assert active.tolist() != reference(case, HALO0)[1].tolist()       # the margin decides something at these shapes
    cascade = CascadeSceneInference(case["model"], head=HEAD0, threshold=thr, margin=0, **KW)
    check_call(cascade, case, active, score)
    thr, active, score = reference(case, HALO0)
    for which, kw in (("flips", dict(tta="flips")), ("ensemble", dict(ensemble=True))):
        cascade = CascadeSceneInference(case["model"], head=HEAD0, threshold=thr, **dict(KW, **kw))
        check_call(cascade, case, active, score, which)


def test_cascade_graphed_equals_eager_with_a_ragged_last_chunk(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import CascadeSceneInference
    thr, active, score = reference(case, HALO0)
    assert active.sum() % CHUNK0 != 0                                   # the last deep chunk is padded
    eager = CascadeSceneInference(case["model"], head=HEAD0, threshold=thr, **KW)(case["u8"])
    graphed = CascadeSceneInference(case["model"], head=HEAD0, threshold=thr, graphed=True, **KW)
    assert same_bits(check_call(graphed, case, active, score), eager)
    assert same_bits(graphed(case["u8"]), eager)                        # a replay
    assert len(graphed.deep._graphs) == 1 and len(graphed.screen._graphs) == 1
    graphed.threshold = float("inf")
    assert same_bits(graphed(case["u8"]), case["M1"]) and graphed.last_forwards == 0


def test_cascade_detect_and_audit(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import CascadeSceneInference, PeakDetector
    thr, active, score = reference(case, HALO0)
    cascade = CascadeSceneInference(case["model"], head=HEAD0, threshold=thr, **KW)
    with pytest.raises(ValueError, match="blind"):
        cascade.detect(case["u8"], PeakDetector(threshold=float(np.nextafter(np.float32(thr), np.float32(-np.inf)))))
    want_map = expected(case, active)
    for level in (thr, 0.98):
        det = PeakDetector(threshold=level, radius=2)
        got, want = cascade.detect(case["u8"], det), det(want_map)
        assert torch.equal(got.count, want.count) and int(want.count.sum()) > 0
        assert same_bits(got.xy, want.xy) and same_bits(got.score, want.score)
    D = case["deep"]["plain"]
    _, deep_score = screen_ref(D.cpu().numpy(), case["owned"], 0.0)
    on = active.astype(bool)
    for level in (None, 0.99):
        lv = np.float32(thr if level is None else level)
        audit = cascade.audit(case["u8"], level)
        print("audit at %.6g: %s" % (lv, audit))
        assert audit.missed == int(((deep_score >= lv) & ~on).sum())
        assert audit.wasted == int(((deep_score < lv) & on).sum())
        assert (audit.n_active, audit.n_tiles) == (int(on.sum()), len(on))
        assert audit.max_abs_diff == float((want_map - D).abs().max()) and audit.max_abs_diff > 0.0
        assert audit.missed + audit.wasted > 0
