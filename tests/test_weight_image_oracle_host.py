"""tests/weight_image_oracle.py held against itself and against tests/gemm_oracle.py on the CPU: the layouts are
bijections onto the valid (tap, k, n), everything else is pad; `gather` turns each engine.pack_* factory's source
description into the dense [taps][K][N] operand gemm_oracle states for the same parameter; the float32 Winograd
transform is exact where it must be."""
import numpy as np
import pytest
import torch

from tests import gemm_oracle as go
from tests import weight_image_oracle as wo

# ragged multi-view channel lists (fp32 views are multiples of 4 wide, bf16 views multiples of 8)
LISTS = {
    wo.FAST: [([12], [40]), ([20, 4, 8], [32, 12]), ([16, 8, 8], [4]), ([4] * 8, [36, 4, 4, 4, 4, 4, 4, 68])],
    wo.WINO: [([12], [40]), ([20, 4, 8], [32, 12]), ([16, 8, 8], [4]), ([4] * 8, [36, 4, 4, 4, 4, 4, 4, 68])],
    wo.BF16: [([8], [40]), ([40, 24], [32, 24]), ([16, 8, 8, 32], [8]), ([8] * 8, [40, 8, 8, 8, 8, 8, 8, 8])],
}
CASES = [(kind, taps, i, o) for kind in (wo.FAST, wo.WINO, wo.BF16) for taps in ((9,) if kind == wo.WINO else (9, 1))
         for i, o in LISTS[kind]]


def _id(c):
    return "%s-t%d-%s-%s" % (c[0], c[1], "_".join(map(str, c[2])), "_".join(map(str, c[3])))


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_layout_is_a_bijection_onto_the_valid_elements(case):
    kind, taps, in_len, out_len = case
    k, n = sum(in_len), sum(out_len)
    m = wo.slot_map(kind, taps, in_len, out_len)
    per_word = 2 if kind == wo.BF16 else 1
    n_chunks = sum(-(-c // wo.KC[kind]) for c in in_len)
    n_tiles = sum(-(-c // 32) for c in out_len)
    assert m.pad.size == per_word * wo.slot_count(kind, taps, in_len, out_len)
    assert wo.slot_count(kind, taps, in_len, out_len) == n_tiles * n_chunks * (4096 if kind == wo.WINO else taps * 512)
    valid = ~m.pad
    assert int(m.k[valid].max()) == k - 1 and int(m.n[valid].max()) == n - 1 and int(m.k[valid].min()) == 0
    if kind == wo.WINO:
        ids = (m.k[valid] * n + m.n[valid]) * 16 + m.xi[valid]
        assert np.array_equal(np.sort(ids), np.arange(k * n * 16))        # every (k, n) once per transform position
    else:
        ids = (m.tap[valid] * k + m.k[valid]) * n + m.n[valid]
        assert np.array_equal(np.sort(ids), np.arange(taps * k * n))      # every (tap, k, n) exactly once
    # the same through image(), on distinct integers (bf16, which has too few of them: distinct normal bf16 numbers)
    count = taps * k * n
    w = (1.0 + np.arange(count)).astype(np.float32).reshape(taps, k, n)
    if kind == wo.BF16:
        i = np.arange(count, dtype=np.uint32)
        assert count <= 2 * 0x7F00
        b16 = np.where(i < 0x7F00, 0x0080 + i, 0x8080 + i - 0x7F00).astype(np.uint32)
        w = (b16 << 16).view(np.float32).reshape(taps, k, n)
        assert np.unique(w).size == count and bool(np.isfinite(w).all())
    img = wo.image(kind, taps, in_len, out_len, w)
    assert img.words.size == wo.slot_count(kind, taps, in_len, out_len) and img.words.dtype == np.uint32
    if kind == wo.FAST:
        vals = img.words.view(np.float32)
        assert np.array_equal(np.sort(vals[~img.pad]), w.reshape(-1)) and not img.words[img.pad].any()
    elif kind == wo.BF16:
        halves = np.stack([img.words & 0xFFFF, img.words >> 16], 1).reshape(-1)
        vals = (halves.astype(np.uint32) << 16).view(np.float32)
        assert np.array_equal(np.sort(vals[valid]), np.sort(w.reshape(-1))) and not halves[m.pad].any()
        assert not img.words[img.pad].any()
    else:
        # xi = 0 shows g[0][0] itself, xi = 15 g[2][2]: the corner taps of every (k, n), each exactly once
        for xi, tap in ((0, 0), (3, 2), (12, 6), (15, 8)):
            sel = valid & (m.xi == xi)
            assert np.array_equal(np.sort(img.f64[sel]), np.sort(w[tap].reshape(-1).astype(np.float64)))
        assert not img.words[img.pad].any() and not img.f64[img.pad].any()


def _factories():
    from unet_nested4tiny_objects_keypoints_amd import engine
    g = torch.Generator().manual_seed(5)
    conv = torch.randn(7, 12, 3, 3, generator=g)
    conv1 = torch.randn(6, 5, 1, 1, generator=g)
    deconv = torch.randn(5, 3, 2, 2, generator=g)
    return [
        ("fwd", engine.pack_conv_fwd(conv), go.w_conv_fwd(conv)),
        ("fwd-1x1", engine.pack_conv_fwd(conv1), go.w_conv_fwd(conv1)),
        ("dgrad", engine.pack_conv_dgrad(conv), go.w_conv_dgrad(conv)),
        ("dgrad-1x1", engine.pack_conv_dgrad(conv1), go.w_conv_dgrad(conv1)),
        ("slice-0", engine.pack_conv_dgrad_slice(conv, 0, 4), go.w_conv_dgrad(conv[:, 0:4])),
        ("slice-5", engine.pack_conv_dgrad_slice(conv, 5, 7), go.w_conv_dgrad(conv[:, 5:12])),
        ("slice-1x1", engine.pack_conv_dgrad_slice(conv1, 2, 3), go.w_conv_dgrad(conv1[:, 2:5])),
        ("deconv_fwd", engine.pack_deconv_fwd(deconv), go.w_deconv_fwd(deconv)),
        ("deconv_dgrad", engine.pack_deconv_dgrad(deconv), go.w_deconv_dgrad(deconv)),
    ]


def test_gather_gives_the_weight_forms_of_the_gemm_oracle():
    seen = set()
    for name, ws, want in _factories():
        got = wo.gather(ws.t.numpy(), ws, ws.taps, ws.k, ws.n)
        assert got.shape == tuple(want.shape) == (ws.taps, ws.k, ws.n), name
        assert np.array_equal(got, want.numpy()), name
        seen.add(name.split("-")[0])
    assert seen == {"fwd", "dgrad", "slice", "deconv_fwd", "deconv_dgrad"}


def test_gather_of_the_packed_operand_is_the_operand():
    class Packed:
        s_t, s_k, s_n, s_ko, s_no, k_inner, n_inner, flip = 5 * 7, 7, 1, 0, 0, 0, 0, False
    w = np.arange(9 * 5 * 7, dtype=np.float32)
    assert np.array_equal(wo.gather(w, Packed, 9, 5, 7), w.reshape(9, 5, 7))


def test_float32_wino_transform_of_multiples_of_four_is_exact():
    rng = np.random.default_rng(11)
    w = (4 * rng.integers(-64, 65, size=(9, 13, 7))).astype(np.float32)
    u32, u64 = wo.wino_f32(w), wo.wino_f64(w)
    assert u32.dtype == np.float32 and u64.dtype == np.float64 and u32.shape == u64.shape == (16, 13, 7)
    assert np.array_equal(u32.astype(np.float64), u64)
    assert np.array_equal(u64, np.round(u64))                      # integers: two exact halvings of multiples of 4
    # against the definition, element by element
    g = w.astype(np.float64).reshape(3, 3, 13, 7)
    for ra in range(4):
        for rb in range(4):
            want = sum(wo.G[ra, r] * wo.G[rb, c] * g[r, c] for r in range(3) for c in range(3))
            assert np.array_equal(u64[4 * ra + rb], want)


def test_float32_wino_transform_stays_within_its_bound_on_full_mantissa_data():
    from tests.helpers import gamma
    rng = np.random.default_rng(12)
    w = (rng.standard_normal((9, 16, 8)) * 2.0 ** rng.integers(-3, 4, size=(9, 16, 8))).astype(np.float32)
    err = np.abs(wo.wino_f32(w).astype(np.float64) - wo.wino_f64(w))
    assert bool((err <= gamma(4) * wo.wino_abs(w)).all())
    assert float(err.max()) > 0.0                                   # (the data does round)


def test_bf16_rounding_matches_torch_on_edge_patterns():
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x3F808000, 0x3F818000, 0x3F807FFF,
                     0x3F808001, 0x3FFFFFFF, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x007FFFFF, 0x807F8000], dtype=np.uint32)
    want = torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)
    assert np.array_equal(wo.bf16_bits(bits.view(np.float32)).astype(np.uint16), want)
