"""The three weight-image layouts of csrc/weight_image.hip, stated once more in numpy index arrays (no GPU).

A fast GEMM kernel reads its B operand W[tap][k][n] as an LDS image per (column tile, K chunk).  Chunks are counted view
by view, ceil(len / kc) per input view, tiles view by view, ceil(len / 32) per output view; the image is ordered
[tile][chunk][...]; a channel or column beyond its view's length is a pad slot and holds +0.0.

    fast (kc 16)  [tap][g 2][col 32][half' 2][4] floats       channel 8 g + 4 (half' ^ ((col >> 3) & 1)) + e
                  gemm_fast.hip: lane (col j, half h) reads its four channels at  j * 8 + ((h ^ ((j >> 3) & 1)) << 2)
    bf16 (kc 32)  [tap][g 2][col 32][h 2][8] bf16             channel 16 g + 8 h + e
                  gemm_bf16.hip: the 64 lanes of a B read cover 1 KB contiguously, 16 bytes = 8 channels of one column;
                  fp32 -> bf16 by round-to-nearest-even, element 2 i in the LOW half of 32-bit word i (bf16_common.h
                  pack_bf2: bf16x2{lo, hi} bit-cast to unsigned)
    wino (kc 8)   4096 floats per (tile, chunk), slot  nh | (xi & 1) << 1 | col << 2 | gq << 6 | (xi >> 1) << 8 | s << 11
                  channel 2 gq + s, column 16 nh + col, xi = 4 ra + rb, value (G g G^T)[ra][rb] of the 3x3 filter
                  g[r][c] = W[3 r + c][k][n], G = [[1, 0, 0], [1/2, 1/2, 1/2], [1/2, -1/2, 1/2], [0, 0, 1]]

`slot_map` is the layout (which W element, or pad, every image element shows); `image` applies it to a dense float32
W[taps][K][N]; `gather` restates the address formula of struct unetpp_weight_src (include/unetpp_hip.h), which is how a
parameter in its torch layout becomes that W.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

FAST, WINO, BF16 = "fast", "wino", "bf16"
KC = {FAST: 16, WINO: 8, BF16: 32}
NCOL = 32
G = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])


def _ceil(a, b):
    return -(-a // b)


def pieces(lens, width):
    """-> (first GEMM index, valid count) of every chunk / tile, view by view"""
    first, room, base = [], [], 0
    for n in lens:
        for i in range(_ceil(n, width)):
            first.append(base + i * width)
            room.append(min(width, n - i * width))
        base += n
    return np.array(first, dtype=np.int64), np.array(room, dtype=np.int64)


def slot_count(kind, taps, in_len, out_len):
    """32-bit words of the image"""
    n_chunks = sum(_ceil(n, KC[kind]) for n in in_len)
    n_tiles = sum(_ceil(n, NCOL) for n in out_len)
    return n_tiles * n_chunks * (4096 if kind == WINO else taps * 512)


@dataclass
class SlotMap:
    """per image ELEMENT, in image order (fast / wino: one per word; bf16: two per word, the even one in the low half)"""
    tap: np.ndarray      # fast / bf16: the tap; wino: 0
    k: np.ndarray        # GEMM row (meaningless where pad)
    n: np.ndarray        # GEMM column (meaningless where pad)
    xi: np.ndarray       # wino: transform position 4 ra + rb; else 0
    pad: np.ndarray      # bool


def slot_map(kind, taps, in_len, out_len) -> SlotMap:
    assert kind in KC and (taps == 9 or (taps == 1 and kind != WINO))
    k0, k_room = pieces(in_len, KC[kind])
    n0, n_room = pieces(out_len, NCOL)
    nt, nc = len(n0), len(k0)

    def ax(values, pos, rank):
        shape = [1] * rank
        shape[pos] = len(values)
        return np.asarray(values, dtype=np.int64).reshape(shape)

    if kind == WINO:     # [tile][chunk][s 2][xi >> 1 8][gq 4][col 16][xi & 1 2][nh 2]
        r = 8
        s, xh, gq, col, xl, nh = ax(range(2), 2, r), ax(range(8), 3, r), ax(range(4), 4, r), ax(range(16), 5, r), \
            ax(range(2), 6, r), ax(range(2), 7, r)
        kk, cl, xi, tap = 2 * gq + s, 16 * nh + col, 2 * xh + xl, np.zeros([1] * r, dtype=np.int64)
    elif kind == FAST:   # [tile][chunk][tap][g 2][col 32][half' 2][e 4]
        r = 7
        tap, g, col, hp, e = ax(range(taps), 2, r), ax(range(2), 3, r), ax(range(32), 4, r), ax(range(2), 5, r), ax(range(4), 6, r)
        kk, cl, xi = 8 * g + 4 * (hp ^ ((col >> 3) & 1)) + e, col, np.zeros([1] * r, dtype=np.int64)
    else:                # [tile][chunk][tap][g 2][col 32][h 2][e 8]
        r = 7
        tap, g, col, h, e = ax(range(taps), 2, r), ax(range(2), 3, r), ax(range(32), 4, r), ax(range(2), 5, r), ax(range(8), 6, r)
        kk, cl, xi = 16 * g + 8 * h + e, col, np.zeros([1] * r, dtype=np.int64)
    k = ax(k0, 1, r) + kk
    n = ax(n0, 0, r) + cl
    pad = (kk >= ax(k_room, 1, r)) | (cl >= ax(n_room, 0, r))
    full = np.broadcast(k, n, tap, xi, pad).shape
    assert full[0] == nt and full[1] == nc
    flat = [np.broadcast_to(a, full).reshape(-1) for a in (tap, k, n, xi, pad)]
    return SlotMap(*flat)


def bf16_bits(x32):
    """float32 -> the 16 bits of its round-to-nearest-even bf16 (finite values and infinities; on the bit pattern)"""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint32)


def wino_f64(w):
    """w float [9][...] -> U [16][...] = G g G^T in float64, xi = 4 ra + rb"""
    g = np.asarray(w, dtype=np.float64).reshape((3, 3) + np.shape(w)[1:])
    return np.einsum("ar,rc...,bc->ab...", G, g, G).reshape((16,) + np.shape(w)[1:])


def wino_abs(w):
    """(|G| |g| |G^T|) [16][...]: what the rounding errors of the transform are measured against"""
    g = np.abs(np.asarray(w, dtype=np.float64)).reshape((3, 3) + np.shape(w)[1:])
    return np.einsum("ar,rc...,bc->ab...", np.abs(G), g, np.abs(G)).reshape((16,) + np.shape(w)[1:])


def _g_rows_f32(w0, w1, w2):
    """the four rows of G applied to three float32 operands, in float32: ((w0 +- w1) + w2) * 0.5"""
    half = np.float32(0.5)
    return [w0, ((w0 + w1) + w2) * half, ((w0 - w1) + w2) * half, w2]


def wino_f32(w):
    """the same transform in float32 arithmetic: down the filter rows first (per filter column), then along the columns"""
    g = np.asarray(w, dtype=np.float32).reshape((3, 3) + np.shape(w)[1:])
    t = [_g_rows_f32(g[0, c], g[1, c], g[2, c]) for c in range(3)]      # t[c][ra]
    u = [_g_rows_f32(t[0][ra], t[1][ra], t[2][ra]) for ra in range(4)]  # u[ra][rb]
    return np.stack([u[ra][rb] for ra in range(4) for rb in range(4)]).astype(np.float32)


@dataclass
class Image:
    words: np.ndarray              # uint32: the expected image (wino: the float32 restatement)
    pad: np.ndarray                # bool per word: no W element shows here, the word is +0.0 (bf16: both halves pad)
    f64: Optional[np.ndarray]      # wino: the float64 value of every word; else None
    mag: Optional[np.ndarray]      # wino: (|G| |g| |G^T|) of every word; else None


def image(kind, taps, in_len, out_len, w) -> Image:
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert w.shape == (taps, sum(in_len), sum(out_len)), (w.shape, taps, in_len, out_len)
    m = slot_map(kind, taps, in_len, out_len)
    k, n = np.where(m.pad, 0, m.k), np.where(m.pad, 0, m.n)
    if kind == WINO:
        u32, u64, mag = wino_f32(w), wino_f64(w), wino_abs(w)
        zero32 = np.float32(0.0)
        words = np.where(m.pad, zero32, u32[m.xi, k, n]).astype(np.float32).view(np.uint32)
        return Image(words, m.pad, np.where(m.pad, 0.0, u64[m.xi, k, n]), np.where(m.pad, 0.0, mag[m.xi, k, n]))
    v = np.where(m.pad, np.float32(0.0), w[m.tap, k, n]).astype(np.float32)
    if kind == FAST:
        return Image(v.view(np.uint32), m.pad, None, None)
    b = bf16_bits(v).reshape(-1, 2)
    return Image((b[:, 0] | (b[:, 1] << 16)).astype(np.uint32), m.pad.reshape(-1, 2).all(1), None, None)


def gather(src_flat, ws, taps, k, n):
    """W[taps][K][N] of struct unetpp_weight_src: element (tap, k, n) sits at
    tap' s_t + (k % k_inner) s_k + (k // k_inner) s_ko + (n % n_inner) s_n + (n // n_inner) s_no, tap' = taps - 1 - tap when
    flip; k_inner / n_inner = 0: no split.  ws: anything with those fields (ops.WSrc)."""
    src_flat = np.asarray(src_flat).reshape(-1)
    t = np.arange(taps, dtype=np.int64).reshape(-1, 1, 1)
    kk = np.arange(k, dtype=np.int64).reshape(1, -1, 1)
    nn = np.arange(n, dtype=np.int64).reshape(1, 1, -1)
    tt = taps - 1 - t if ws.flip else t
    ki, ko = (kk % ws.k_inner, kk // ws.k_inner) if ws.k_inner > 0 else (kk, 0 * kk)
    ni, no = (nn % ws.n_inner, nn // ws.n_inner) if ws.n_inner > 0 else (nn, 0 * nn)
    addr = tt * ws.s_t + ki * ws.s_k + ko * ws.s_ko + ni * ws.s_n + no * ws.s_no
    assert int(addr.min()) >= 0 and int(addr.max()) < src_flat.size, "the source formula leaves the parameter"
    return src_flat[addr]
