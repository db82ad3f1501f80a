"""Scene inference on the GPU (scene.py, csrc/scene.hip).

(a) unetpp_scene_stitch alone, bit for bit against the torch composition of tests/test_scene_host.py (slice, flip /
    transpose, sequential sum, true division, slice-assign): `out` starts as NaN, so every owned pixel must have been
    written; everything a tile does not own is NaN in its maps, so none of it may have been read.  Class counts 1 / 3 / 4,
    1 / 4 / 8 variants, plans aligned to 2 and to 4 (owned rectangles that start at 2 mod 4 and a frame width that is no
    multiple of 4: the scalar store path), non-square tiles, chunked calls with padding rows.
(b) 64-bit offsets: a frame map of 47000 x 47000 (2.2e9 elements, never filled), four tiles in its bottom-right corner.
(c) SceneInference end to end on a depth-3 network: below the suite's 1e-4 against the float64 oracle's WHOLE-frame head;
    bit for bit equal to per-tile ``model.infer`` outputs placed with torch slicing; graphed equals eager; uint8 and
    float32 frames; the ensemble; flips against four ``infer`` calls; bf16 storage (structure only); points(); refusals.
    Equality with the GPU's own whole-frame ``infer`` holds only where the same kernels are selected: printed, not asserted.
"""
import pytest
import torch

from tests.helpers import rel_err
from tests.test_scene_host import oracle64, owned_mean, rect_rows, stitch_ref, variant

pytestmark = pytest.mark.gpu

TOL = 1e-4
MUL = 1.0 / 255.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ------------------------------------------------------------------------------------------------ (a)
def poisoned_tiles(rects, codes, C, th, tw, dev, seed):
    """[n, K, C, th, tw]: random values where the tile owns the frame (placed through each variant's transform), NaN
    everywhere else and in padding tiles"""
    g = torch.Generator(device=dev).manual_seed(seed)
    tiles = torch.full((len(rects), len(codes), C, th, tw), float("nan"), device=dev)
    for t, (f, oy, ox, y0, y1, x0, x1) in enumerate(rects):
        if f < 0:
            continue
        for k, code in enumerate(codes):
            plain = torch.full((C, th, tw), float("nan"), device=dev)
            plain[:, y0 - oy:y1 - oy, x0 - ox:x1 - ox] = torch.randn(C, y1 - y0, x1 - x0, generator=g, device=dev)
            tiles[t, k] = variant(plain, code)
    return tiles


def run_stitch(tiles, rects, codes, out):
    from unet_nested4tiny_objects_keypoints_amd import ops
    table = ops.scene_rects(rects)
    ops.scene_stitch(tiles, table, table.to(tiles.device), codes, out)


STITCH_GEOMETRY = [   # (H, W, tile, halo, align)
    (72, 88, 32, 8, 4),
    (72, 88, 32, 8, 2),
    (70, 90, 32, 10, 2),      # owned rectangles start at 2 mod 4, rows of 90 floats: ragged quads and scalar stores
]
CODES = {1: (0,), 4: (0, 1, 2, 3), 8: tuple(range(8))}


@pytest.mark.parametrize("K", [1, 4, 8])
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("geom", STITCH_GEOMETRY, ids=["%dx%d-t%d-h%d-a%d" % g for g in STITCH_GEOMETRY])
def test_stitch_equals_the_torch_composition(dev, geom, C, K):
    H, W, tile, halo, align = geom
    S = 2
    rects = rect_rows(H, W, tile, halo, align, S)
    assert len(rects) == (2 * 4 * 5 if (H, W) == (72, 88) else 2 * 5 * 6)      # clamped last tiles on both axes
    if align == 2 and halo == 10:
        assert any(r[5] % 4 == 2 for r in rects)
    codes = CODES[K] if K != 8 else (3, 5, 0, 6, 1, 7, 2, 4)          # (any order of the eight)
    tiles = poisoned_tiles(rects, codes, C, tile, tile, dev, 1000 + 10 * C + K)
    got = torch.full((S, C, H, W), float("nan"), device=dev)
    run_stitch(tiles, rects, codes, got)
    want = stitch_ref(tiles, rects, codes, torch.full((S, C, H, W), float("nan"), device=dev))
    assert not bool(torch.isnan(want).any())                           # the plan covers the frame
    assert not bool(torch.isnan(got).any()), "a pixel was not written, or a value outside an owned rectangle was read"
    assert same_bits(got, want)


@pytest.mark.parametrize("K", [1, 4])
def test_stitch_non_square_tiles(dev, K):
    H, W, tile, halo, align, C, S = 24, 88, 32, 8, 4, 3, 1
    rects = rect_rows(H, W, tile, halo, align, S)
    assert len(rects) == 5 and rects[0][4] == 24
    tiles = poisoned_tiles(rects, CODES[K], C, 24, 32, dev, 77 + K)
    got = torch.full((S, C, H, W), float("nan"), device=dev)
    run_stitch(tiles, rects, CODES[K], got)
    want = stitch_ref(tiles, rects, CODES[K], torch.full((S, C, H, W), float("nan"), device=dev))
    assert not bool(torch.isnan(got).any()) and same_bits(got, want)
    from unet_nested4tiny_objects_keypoints_amd import ops
    with pytest.raises(RuntimeError, match="invalid argument"):       # a transposing variant of a 24x32 tile
        run_stitch(tiles[:, :1].contiguous(), rects, (4,), got)
    with pytest.raises(ValueError):
        run_stitch(tiles, rects, (0, 1), got)                          # K = 4 maps, two codes
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scene_stitch(tiles.cpu(), ops.scene_rects(rects), ops.scene_rects(rects), CODES[K], got.cpu())


def test_stitch_in_chunks_with_padding_rows_equals_one_call(dev):
    H, W, tile, halo, align, C, codes = 96, 112, 64, 24, 4, 4, CODES[4]
    rects = rect_rows(H, W, tile, halo, align)
    assert len(rects) == 12
    tiles = poisoned_tiles(rects, codes, C, tile, tile, dev, 5)
    whole = torch.full((1, C, H, W), float("nan"), device=dev)
    run_stitch(tiles, rects, codes, whole)
    parts = torch.full((1, C, H, W), float("nan"), device=dev)
    pad = (-1, 0, 0, 0, 0, 0, 0)
    for i in range(0, 12, 5):
        part = rects[i:i + 5]
        live = len(part)
        chunk = torch.full((5, len(codes), C, tile, tile), float("nan"), device=dev)
        chunk[:live] = tiles[i:i + live]
        run_stitch(chunk, part + [pad] * (5 - live), codes, parts)
    assert not bool(torch.isnan(whole).any()) and same_bits(parts, whole)
    run_stitch(tiles[:2], [pad, pad], codes, parts)                    # nothing but padding: nothing happens
    assert same_bits(parts, whole)


# ------------------------------------------------------------------------------------------------ (b)
def test_stitch_offsets_beyond_2_31_elements(dev):
    side, tile, halo, align, C = 47000, 64, 8, 2, 1
    out = torch.empty(1, C, side, side, device=dev)                    # 8.8 GB, never filled
    assert out.numel() > 2 ** 31
    from unet_nested4tiny_objects_keypoints_amd.scene import plan_tiles
    rows, cols = plan_tiles(side, side, tile, halo, align)
    corner = [(0, oy, ox, y0, y1, x0, x1) for (oy, y0, y1) in rows[-2:] for (ox, x0, x1) in cols[-2:]]
    assert len(corner) == 4 and max(r[4] for r in corner) == side and max(r[6] for r in corner) == side
    codes = CODES[8]
    tiles = poisoned_tiles(corner, codes, C, tile, tile, dev, 9)
    for r in corner:
        out[0, :, r[3]:r[4], r[5]:r[6]] = float("nan")
    run_stitch(tiles, corner, codes, out)
    for t, r in enumerate(corner):
        got = out[0, :, r[3]:r[4], r[5]:r[6]]
        assert ((0 * side + r[3]) * side + r[5]) > 2 ** 31
        assert not bool(torch.isnan(got).any()) and same_bits(got, owned_mean(tiles[t], codes, r)), r
    del out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ (c)
H0, W0, TILE0, HEAD0, S0 = 96, 112, 64, 2, 2


def _model(dev, depth=3, fs=8, bf16=False, **kw):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    ref, ctor, state = oracle64(depth, fs)
    m = UNet_Nested(**dict(ctor, **kw))
    if not kw:
        m.load_state_dict(state)
    m = m.to(dev).eval()
    if bf16:
        m.set_activation_dtype(torch.bfloat16)
    return m


@pytest.fixture(scope="module")
def case(dev):
    """frames, the normalised fp32 frames the tiles are cut from, the model, and the float64 oracle's whole-frame heads --
    computed once and left unchanged"""
    g = torch.Generator().manual_seed(41)
    u8 = torch.randint(0, 256, (S0, H0, W0, 1), generator=g, dtype=torch.uint8)
    x32 = (u8.permute(0, 3, 1, 2).float() * torch.tensor(MUL, dtype=torch.float32)).contiguous()   # pixel * mul, one rounding
    ref, _, _ = oracle64(3)
    with torch.no_grad():
        heads64 = ref(x32.double())
    return dict(u8=u8.to(dev), x32=x32.to(dev), model=_model(dev), heads64=heads64)


def placed(model, x32, head, ensemble, tile, halo, align, codes=(0,), per_tile=True):
    """the torch composition of the driver: crop each tile, run ``infer`` on it (on each of its variants: one call per
    variant code), undo the variant, mean, and place the owned block"""
    S, _, H, W = x32.shape
    th, tw = min(tile, H), min(tile, W)
    rects = rect_rows(H, W, tile, halo, align, S)
    out = torch.full((S, model.n_classes, H, W), float("nan"), device=x32.device)
    groups = [[r] for r in rects] if per_tile else [rects]
    for group in groups:
        crops = torch.stack([x32[s, :, oy:oy + th, ox:ox + tw] for (s, oy, ox, *_) in group])
        maps = torch.stack([model.infer(variant(crops, code).contiguous(), head, ensemble) for code in codes], dim=1)
        stitch_ref(maps, group, codes, out)
    return out


def test_scene_equals_whole_frame_oracle_and_per_tile_infer(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import SceneInference
    model = case["model"]
    scene = SceneInference(model, head=HEAD0, tile=TILE0, mul=MUL)
    assert (scene.halo, scene.align) == (24, 4) and abs(scene.efficiency(H0, W0) - 96 * 112 / (12 * 64 * 64)) < 1e-12
    got = scene(case["u8"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (S0, 4, H0, W0) and got.grad_fn is None
    err = rel_err(got.cpu(), case["heads64"][HEAD0 - 1])
    print("scene vs float64 whole-frame oracle: head %d rel_err %.3e" % (HEAD0, err))
    assert err < TOL, err
    want = placed(model, case["x32"], HEAD0, False, TILE0, 24, 4)
    assert same_bits(got, want)
    whole = model.infer(case["x32"], HEAD0)
    print("scene vs the GPU's own whole-frame infer: bit-identical %s, max|diff| %.3e"
          % (same_bits(got, whole), float((got - whole).abs().max())))
    # float32 frames [S, C, H, W] go through the same normalisation; one frame without the leading axis
    f32 = case["u8"].permute(0, 3, 1, 2).float().contiguous()
    assert same_bits(scene(f32), got)
    assert same_bits(scene(case["u8"][1]), got[1:2]) and same_bits(scene(f32[0]), got[0:1])
    assert same_bits(scene(case["u8"]), got)                           # the cached plan
    # a frame no larger than the tile is infer itself
    small = case["x32"][:, :, :48, :64].contiguous()
    assert same_bits(SceneInference(model, head=1, tile=TILE0, mul=1.0)(small), model.infer(small, 1))


def test_scene_graphed_equals_eager_with_a_ragged_last_chunk(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import SceneInference
    model = case["model"]
    eager = SceneInference(model, head=HEAD0, tile=TILE0, mul=MUL, chunk=5)(case["u8"])      # 24 tiles: 5, 5, 5, 5, 4
    graphed = SceneInference(model, head=HEAD0, tile=TILE0, mul=MUL, chunk=5, graphed=True)
    assert same_bits(graphed(case["u8"]), eager)
    assert same_bits(graphed(case["u8"][:1]), eager[:1])               # 12 tiles: 5, 5, 2 through the same graph
    assert len(graphed._graphs) == 1
    assert same_bits(eager, SceneInference(model, head=HEAD0, tile=TILE0, mul=MUL)(case["u8"]))   # chunk 8


def test_scene_ensemble_and_flips(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import SceneInference
    model = case["model"]
    ens = SceneInference(model, head=HEAD0, ensemble=True, tile=TILE0, mul=MUL)(case["u8"])
    want64 = sum(case["heads64"][:HEAD0]) / HEAD0
    err = rel_err(ens.cpu(), want64)
    print("scene ensemble vs float64 whole-frame oracle: rel_err %.3e" % err)
    assert err < TOL, err
    assert same_bits(ens, placed(model, case["x32"], HEAD0, True, TILE0, 24, 4))
    flips = SceneInference(model, head=HEAD0, tile=TILE0, mul=MUL, tta="flips")(case["u8"])
    assert same_bits(flips, placed(model, case["x32"], HEAD0, False, TILE0, 24, 4, codes=(0, 1, 2, 3), per_tile=False))
    # the augmented mean is still the head: the float64 oracle's mean over the four flips of the WHOLE frame
    ref, _, _ = oracle64(3)
    x64 = case["x32"].double().cpu()
    with torch.no_grad():
        mean64 = sum(variant(ref(variant(x64, c))[HEAD0 - 1], c) for c in (0, 1, 2, 3)) / 4
    err = rel_err(flips.cpu(), mean64)
    print("scene flips vs float64 oracle's mean over whole-frame flips: rel_err %.3e" % err)
    assert err < TOL, err


def test_scene_dihedral_square_tiles(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import SceneInference
    model = case["model"]
    scene = SceneInference(model, head=1, tile=TILE0, mul=MUL, tta="dihedral", chunk=3)
    got = scene(case["u8"])
    want = placed(model, case["x32"], 1, False, TILE0, 12, 4, codes=tuple(range(8)), per_tile=False)
    assert same_bits(got, want)
    with pytest.raises(ValueError, match="square"):
        scene(case["u8"][:, :48].contiguous())                         # a frame side below the tile


def test_scene_bf16_storage_structure(dev):
    from unet_nested4tiny_objects_keypoints_amd import SceneInference
    model = _model(dev, depth=3, fs=4, bf16=True)
    g = torch.Generator().manual_seed(43)
    u8 = torch.randint(0, 256, (1, H0, W0, 1), generator=g, dtype=torch.uint8).to(dev)
    x32 = (u8.permute(0, 3, 1, 2).float() * torch.tensor(MUL, dtype=torch.float32, device=dev)).contiguous()
    got = SceneInference(model, head=HEAD0, tile=TILE0, mul=MUL)(u8)
    assert got.dtype == torch.float32 and same_bits(got, placed(model, x32, HEAD0, False, TILE0, 24, 4))


def test_scene_points_equals_transfer_points(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import Heatmap, SceneInference
    scene = SceneInference(case["model"], head=HEAD0, tile=TILE0, mul=MUL)
    maps = scene(case["u8"])
    hm = Heatmap([[0], [1, 2, 3], [4], [5, 6]], W0, H0)
    pts, counts = scene.points(maps, hm, threshold=0.5)
    want_pts, want_counts = hm.transfer_points(maps, None, 0.5)
    assert torch.equal(pts, want_pts) and torch.equal(counts, want_counts)


def test_scene_refusals(dev, case):
    from unet_nested4tiny_objects_keypoints_amd import SceneInference
    model = case["model"]
    with pytest.raises(RuntimeError, match="eval"):
        SceneInference(_model(dev).train(), head=1)
    with pytest.raises(ValueError, match="align_corners"):
        SceneInference(_model(dev, is_deconv=False), head=1)
    for kw in (dict(halo=20), dict(halo=26), dict(tile=62), dict(tile=48), dict(tile=40)):
        with pytest.raises(ValueError):
            SceneInference(model, head=HEAD0, **kw)
    scene = SceneInference(model, head=HEAD0, tile=TILE0, mul=MUL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene(case["u8"].cpu())
    with pytest.raises(ValueError):
        scene(case["u8"][:, :94].contiguous())                         # H not a multiple of 4
    with pytest.raises(ValueError):
        scene(case["u8"].expand(S0, H0, W0, 3).contiguous())           # channels
    with pytest.raises(TypeError):
        scene(case["u8"].to(torch.int16))
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            scene(case["u8"])
    finally:
        model.eval()
