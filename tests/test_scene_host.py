"""Host side of scene inference (scene.py, csrc/scene.hip), no GPU:
  (1) plan_tiles: aligned origins, owned intervals that partition the axis, every owned pixel at least `halo` away from
      each tile edge that is not a frame edge -- exhaustively over small geometries;
  (2) required_halo against the measured radius table r_J = 7 * 2^J - 5;
  (3) the ABI entry's argument checks (status codes, no device touched) and the table row's layout;
  (4) the claim the feature rests on: a tiled forward of the float64 oracle, cut by the product's plan with the product's
      halo rule, equals the whole-frame forward (max |diff| <= 1e-12; measured 0.0, and up to 6.7e-16 on a host whose
      convolution takes another path for the tile's shape), and a halo of 20 where 24 is
      needed does not (the negative control);
  (5) a torch restatement of the stitch (stitch_ref below, the composition the GPU tests hold the kernel against):
      applied to the dihedral variants of a map it returns that map bit for bit.
"""
import ctypes
import os
import subprocess

import pytest
import torch

from tests.helpers import seeded_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLIP_X, FLIP_Y, TRANSPOSE = 1, 2, 4


# ---- the torch composition: slice, flip / transpose, sequential sum, divide, slice-assign ---------------------------
def variant(t, code):
    """the variant `code` of a tile [..., Th, Tw]: flip_y(flip_x(transpose(tile))), each step only if its bit is set"""
    if code & TRANSPOSE:
        t = t.transpose(-1, -2)
    if code & FLIP_X:
        t = t.flip(-1)
    if code & FLIP_Y:
        t = t.flip(-2)
    return t


def unvariant(m, code):
    """the inverse: a map of the variant back into the tile's frame"""
    if code & FLIP_Y:
        m = m.flip(-2)
    if code & FLIP_X:
        m = m.flip(-1)
    if code & TRANSPOSE:
        m = m.transpose(-1, -2)
    return m


def owned_mean(tile_maps, codes, rect):
    """tile_maps [K, C, Th, Tw] of one tile -> the owned block [C, y_hi - y_lo, x_hi - x_lo]:
    (((v_0 + v_1) + ...) + v_{K-1}) / K with a true division (the divisor is a tensor: a Python scalar may be turned
    into a multiplication by its reciprocal)."""
    _, oy, ox, y0, y1, x0, x1 = rect
    acc = None
    for k, code in enumerate(codes):
        v = unvariant(tile_maps[k], code)[:, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        acc = v if acc is None else acc + v
    if len(codes) > 1:
        acc = acc / torch.tensor(float(len(codes)), dtype=acc.dtype, device=acc.device)
    return acc


def stitch_ref(tiles, rects, codes, out):
    """tiles [n, K, C, Th, Tw], rects rows (frame, oy, ox, y_lo, y_hi, x_lo, x_hi); writes out [S, C, H, W] in place"""
    for t, rect in enumerate(rects):
        if rect[0] >= 0:
            out[rect[0], :, rect[3]:rect[4], rect[5]:rect[6]] = owned_mean(tiles[t], codes, rect)
    return out


def rect_rows(H, W, tile, halo, align, frames=1):
    from unet_nested4tiny_objects_keypoints_amd.scene import plan_tiles
    rows, cols = plan_tiles(H, W, tile, halo, align)
    return [(s, oy, ox, y0, y1, x0, x1) for s in range(frames) for (oy, y0, y1) in rows for (ox, x0, x1) in cols]


# ---- (1) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [2, 4, 8])
def test_plan_tiles_properties(align):
    from unet_nested4tiny_objects_keypoints_amd.scene import plan_tiles
    seen_clamped = seen_single = 0
    for tile in (32, 64):
        for halo in (8, 16, 24):
            if halo % align or tile <= 2 * halo:
                continue
            for L in range(32, 257, align):
                rows, cols = plan_tiles(L, 32, tile, halo, align)
                assert cols == [(0, 0, 32)]
                T = min(tile, L)
                if T == L:
                    assert rows == [(0, 0, L)]
                    seen_single += 1
                    continue
                s = T - 2 * halo
                assert [o for o, _, _ in rows] == [min(k * s, L - T) for k in range(len(rows))]
                assert rows[-1][0] == L - T and all(o < L - T for o, _, _ in rows[:-1])
                seen_clamped += rows[-1][0] != (len(rows) - 1) * s
                edge = 0
                for o, lo, hi in rows:
                    assert o % align == 0 and lo % align == 0 and hi % align == 0     # aligned
                    assert lo == edge and lo < hi                                     # a partition, nobody owns nothing
                    edge = hi
                    assert o <= lo and hi <= o + T                                    # inside the tile
                    assert o == 0 or lo - o >= halo                                   # a cut edge is at least halo away
                    assert o + T == L or o + T - hi >= halo
                assert edge == L
    assert seen_clamped and seen_single


def test_plan_tiles_refuses_bad_geometry():
    from unet_nested4tiny_objects_keypoints_amd.scene import plan_tiles
    for args in ((96, 112, 64, 24, 16), (98, 112, 64, 24, 4), (96, 110, 64, 24, 4), (96, 112, 62, 24, 4),
                 (96, 112, 64, 22, 4), (96, 112, 64, 32, 4), (96, 112, 32, 16, 4), (0, 112, 64, 24, 4),
                 (96, 112, 64, 24, 0), (96.0, 112, 64, 24, 4)):
        with pytest.raises(ValueError):
            plan_tiles(*args)
    assert plan_tiles(32, 64, 64, 32, 4) == ([(0, 0, 32)], [(0, 0, 64)])    # one tile: the halo does not matter
    assert plan_tiles(96, 112, 64, 24, 4) == ([(0, 0, 40), (16, 40, 56), (32, 56, 96)],
                                              [(0, 0, 40), (16, 40, 56), (32, 56, 72), (48, 72, 112)])


# ---- (2) ------------------------------------------------------------------------------------------------------------
def test_required_halo_table():
    from unet_nested4tiny_objects_keypoints_amd.scene import required_halo
    radius = {1: 9, 2: 23, 3: 51, 4: 107}
    for depth in (2, 3, 4, 5):
        a = 1 << (depth - 1)
        for head in range(1, depth):
            h = required_halo(depth, head)
            assert h % a == 0 and radius[head] <= h < radius[head] + a, (depth, head, h)
    assert [required_halo(2, 1), required_halo(3, 1), required_halo(3, 2), required_halo(4, 3), required_halo(5, 4)] == \
        [10, 12, 24, 56, 112]
    for bad in (0, 3, True, 1.0):
        with pytest.raises(ValueError):
            required_halo(3, bad)


def test_efficiency_and_constructor_refusals_without_gpu():
    from unet_nested4tiny_objects_keypoints_amd import SceneInference, UNet_Nested
    m = UNet_Nested(in_channels=1, feature_scale=8)
    with pytest.raises(RuntimeError, match="eval"):
        SceneInference(m)                                       # a fresh module is in training mode
    m.eval()
    scene = SceneInference(m)                                    # head 3 of depth 4: halo 56 at tile 512
    assert (scene.head, scene.halo, scene.align, scene.variants) == (3, 56, 8, (0,))
    assert scene.efficiency(512, 512) == 1.0 and scene.efficiency(256, 128) == 1.0
    assert abs(scene.efficiency(4096, 4096) - 4096.0 ** 2 / (100 * 512 ** 2)) < 1e-12
    assert abs(scene.efficiency(400 * 200 + 112, 400 * 200 + 112) - (400 / 512) ** 2) < 0.01    # about 0.61
    with pytest.raises(ValueError, match="align_corners"):
        SceneInference(UNet_Nested(in_channels=1, feature_scale=8, is_deconv=False).eval())
    for kw in (dict(halo=48), dict(halo=60), dict(tile=500), dict(tile=112), dict(tile=96), dict(head=4), dict(head=0),
               dict(tta="rot"), dict(chunk=0), dict(tile=512.0)):
        with pytest.raises(ValueError):
            SceneInference(m, **kw)
    assert SceneInference(m, head=1, tta="dihedral").variants == tuple(range(8))
    assert SceneInference(m, head=2, tta="flips", halo=32).variants == (0, 1, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene(torch.zeros(1, 64, 64, 1, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene(torch.zeros(1, 1, 64, 64))


# ---- (3) ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as entry
    entry.build()
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib


def test_scene_stitch_abi_argument_checks(built_lib):
    L = built_lib
    lib = L.lib()
    assert lib.unetpp_abi_version() == L.ABI_VERSION == 14     # an additive entry point: the version stays
    p = ctypes.c_void_p(0x1000)                               # never dereferenced: every call below is refused on the host

    def call(tiles=p, n=2, K=1, C=4, Th=32, Tw=32, codes=(0,), rows=((0, 0, 0, 0, 24, 0, 24), (0, 0, 16, 0, 24, 24, 48)),
             table="host", dev=p, out=p, S=1, H=32, W=48):
        host = (L.SceneRect * max(1, len(rows)))()
        for i, r in enumerate(rows):
            (host[i].frame, host[i].oy, host[i].ox, host[i].y_lo, host[i].y_hi, host[i].x_lo, host[i].x_hi) = r
        arr = (ctypes.c_int32 * 8)(*codes) if codes is not None else None
        return lib.unetpp_scene_stitch(tiles, n, K, C, Th, Tw, arr, host if table == "host" else None, dev, out, S, H, W,
                                       None)

    for name in ("tiles", "dev", "out"):
        assert call(**{name: None}) == -1, name
    assert call(codes=None) == -1 and call(table=None) == -1
    for name in ("n", "C", "Th", "Tw", "S", "H", "W"):
        assert call(**{name: 0}) == -1, name
        assert call(**{name: -2}) == -1, name
    for K in (0, -1, 9):
        assert call(K=K, codes=(0,) * 8) == -1, K
    assert call(codes=(8,)) == -1 and call(codes=(-1,)) == -1
    assert call(K=2, codes=(0, 4), Th=32, Tw=48, W=64, rows=((0, 0, 0, 0, 24, 0, 24),), n=1) == -1   # transposing, Th != Tw
    assert call(n=65536) == -1 and call(C=65536) == -1
    ok = (0, 0, 16, 0, 24, 24, 48)
    for bad in ((1, 0, 16, 0, 24, 24, 48),      # frame >= S
                (0, 8, 16, 8, 24, 24, 48),      # tile leaves the frame in y
                (0, 0, 24, 0, 24, 24, 48),      # ... in x
                (0, -8, 16, 0, 24, 24, 48),     # negative origin
                (0, 0, 16, 0, 24, 8, 48),       # owned rectangle leaves the tile (left)
                (0, 0, 16, 0, 33, 24, 48),      # (below)
                (0, 0, 16, 0, 24, 24, 49),      # (right)
                (0, 0, 16, 12, 12, 24, 48),     # empty
                (0, 0, 16, 0, 24, 40, 24)):     # inverted
        assert call(rows=(ok, bad)) == -1, bad
    # a chunk of nothing but padding tiles is accepted and launches nothing (the pointers are still never followed)
    assert call(rows=((-1, 0, 0, 0, 0, 0, 0), (-1, 9, 9, 9, 9, 9, 9))) == 0


def test_scene_rect_layout_matches_header(built_lib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "unetpp_hip.h"\nint main(void){'
                   'printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(unetpp_scene_rect), offsetof(unetpp_scene_rect, oy),'
                   'offsetof(unetpp_scene_rect, y_lo), offsetof(unetpp_scene_rect, x_hi),'
                   'offsetof(unetpp_scene_rect, reserved), UNETPP_SCENE_MAX_VARIANTS, UNETPP_SCENE_FLIP_X,'
                   'UNETPP_SCENE_FLIP_Y, UNETPP_SCENE_TRANSPOSE);return 0;}')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    L = built_lib
    assert got == [ctypes.sizeof(L.SceneRect), L.SceneRect.oy.offset, L.SceneRect.y_lo.offset, L.SceneRect.x_hi.offset,
                   L.SceneRect.reserved.offset, L.SCENE_MAX_VARIANTS, L.SCENE_FLIP_X, L.SCENE_FLIP_Y, L.SCENE_TRANSPOSE]
    assert ctypes.sizeof(L.SceneRect) == 32 and (FLIP_X, FLIP_Y, TRANSPOSE) == (L.SCENE_FLIP_X, L.SCENE_FLIP_Y,
                                                                                 L.SCENE_TRANSPOSE)
    from unet_nested4tiny_objects_keypoints_amd import ops
    t = ops.scene_rects([(0, 16, 32, 40, 56, 56, 72), (-1, 0, 0, 0, 0, 0, 0)])
    assert t.dtype == torch.int32 and t.tolist() == [[0, 16, 32, 40, 56, 56, 72, 0], [-1, 0, 0, 0, 0, 0, 0, 0]]


# ---- (4) ------------------------------------------------------------------------------------------------------------
_ORACLES = {}


def oracle64(depth, fs=8, in_channels=1, seed=21):
    """the float64 oracle in eval mode with the suite's seeded state (BatchNorm on non-trivial running statistics)"""
    key = (depth, fs, in_channels, seed)
    if key not in _ORACLES:
        from oracle.unet_nested_oracle import UNetNestedOracle
        ctor = dict(in_channels=in_channels, n_classes=4, feature_scale=fs, depth=depth)
        ref = UNetNestedOracle(**ctor)
        state = seeded_state(ref, seed)
        ref.load_state_dict(state)
        _ORACLES[key] = (ref.double().eval(), ctor, state)
    return _ORACLES[key]


def tiled_oracle_head(ref, x, head, tile, halo, align):
    """head `head` of the oracle over x [S, C, H, W] (float64), tile by tile: crop, forward, keep the owned block"""
    S, _, H, W = x.shape
    th, tw = min(tile, H), min(tile, W)
    rects = rect_rows(H, W, tile, halo, align, S)
    crops = torch.stack([x[s, :, oy:oy + th, ox:ox + tw] for (s, oy, ox, *_) in rects])
    with torch.no_grad():
        maps = ref(crops)[head - 1]
    out = torch.full((S, maps.shape[1], H, W), float("nan"), dtype=maps.dtype)
    return stitch_ref(maps.unsqueeze(1), rects, (0,), out)


EXACT_CASES = [   # (depth, head, tile, frames)
    (2, 1, 32, ((96, 112), (24, 50))),
    (3, 1, 32, ((96, 112), (48, 136))),
    (3, 1, 64, ((96, 112),)),
    (3, 2, 64, ((96, 112), (48, 136))),        # 96x112: the clamped last tiles overlap their neighbours; 48 < tile
    (4, 3, 128, ((160, 144), (48, 136))),
]


@pytest.mark.parametrize("depth,head,tile,frames", EXACT_CASES, ids=["d%d-h%d-t%d" % c[:3] for c in EXACT_CASES])
def test_tiled_oracle_forward_equals_whole_frame_forward(depth, head, tile, frames):
    from unet_nested4tiny_objects_keypoints_amd.scene import required_halo
    ref, _, _ = oracle64(depth)
    halo, align = required_halo(depth, head), 1 << (depth - 1)
    g = torch.Generator().manual_seed(100 * depth + head)
    for (H, W) in frames:
        x = torch.rand(1, 1, H, W, generator=g, dtype=torch.float64)
        with torch.no_grad():
            whole = ref(x)[head - 1]
        tiled = tiled_oracle_head(ref, x, head, tile, halo, align)
        diff = float((tiled - whole).abs().max())             # (a NaN left by a gap in the partition fails here too)
        print("tiled vs whole oracle: depth %d head %d tile %d halo %d frame %dx%d max|diff| %.3e"
              % (depth, head, tile, halo, H, W, diff))
        assert diff <= 1e-12, (depth, head, tile, H, W, diff)


def test_a_halo_below_the_radius_is_not_exact():
    ref, _, _ = oracle64(3)
    x = torch.rand(1, 1, 96, 112, generator=torch.Generator().manual_seed(302), dtype=torch.float64)
    with torch.no_grad():
        whole = ref(x)[1]
    diff = float((tiled_oracle_head(ref, x, 2, 64, 20, 4) - whole).abs().max())
    print("negative control: depth 3 head 2 halo 20 (24 needed) max|diff| %.3e" % diff)
    assert diff > 1e-9, diff


# ---- (5) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,codes", [((3, 32, 32), tuple(range(8))), ((2, 24, 40), (0, 1, 2, 3)), ((1, 16, 16), (5,)),
                                         ((2, 16, 16), (6, 3, 4))])
def test_stitch_restatement_returns_the_map_from_its_dihedral_variants(shape, codes):
    """Values are multiples of 2^-8 below 2^8, so the sum of up to 8 equal values is exact and the mean of equal values is
    the value itself: any difference is a misplaced pixel."""
    C, H, W = shape
    g = torch.Generator().manual_seed(7)
    m = torch.randint(0, 1 << 16, shape, generator=g).float() / 256.0
    tiles = torch.stack([variant(m, c).contiguous() for c in codes]).unsqueeze(0)        # [1, K, C, Th, Tw]
    for rect in ((0, 0, 0, 0, H, 0, W), (0, 0, 0, 4, H - 6, 2, W - 8)):
        out = torch.full((1, C, H, W), float("nan"))
        stitch_ref(tiles, [rect], codes, out)
        _, _, _, y0, y1, x0, x1 = rect
        assert torch.equal(out[0, :, y0:y1, x0:x1], m[:, y0:y1, x0:x1])
        inside = torch.zeros(H, W, dtype=torch.bool)
        inside[y0:y1, x0:x1] = True
        assert bool(torch.isnan(out[0][:, ~inside]).all())                               # nothing else was written
    # the eight variants are distinct pixel permutations, the flips those of torch
    assert len({tuple(variant(m, c).reshape(-1).tolist()) for c in range(4)}) == 4
    assert torch.equal(variant(m, 1), m.flip(-1)) and torch.equal(variant(m, 3), m.flip(-1, -2))
    if H == W:
        assert len({tuple(variant(m, c).reshape(-1).tolist()) for c in range(8)}) == 8
        assert torch.equal(variant(m, 5), torch.rot90(m, -1, (-2, -1)))                  # transpose, then flip x: clockwise
        assert torch.equal(variant(m, 6), torch.rot90(m, 1, (-2, -1)))
