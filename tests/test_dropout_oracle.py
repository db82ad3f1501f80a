"""oracle/dropout_oracle.py: the numpy restatement of the heads' keep mask (csrc/dropout.h), on the CPU.

Known answers of splitmix64, the 16-bit threshold, the keying of the bf16 kernels (two quads per channel octet), and
the statistics of the mask at one seed.  tests/test_gpu_heads.py ties the restatement to the kernels bit for bit."""
import numpy as np

from oracle.dropout_oracle import keep_bits, keep_mask, keep_one, keep_threshold, mix64


def test_splitmix64_known_answers():
    # splitmix64 from state 0 (Vigna's reference generator): first two outputs.  Pixel 0, quad g -> counter g + 1.
    assert int(mix64(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF
    for c in (4, 32, 128):
        g4n = (c + 3) // 4
        assert int(keep_bits(0, 0, g4n, 0)) == 0xE220A8397B1DCDAF
    assert int(keep_bits(0, 0, 8, 1)) == 0x6E789E6AA1B965F4
    # the seed adds to the state; the pixel steps the counter by the quad count
    assert int(keep_bits(0, 1, 1, 0)) == 0x6E789E6AA1B965F4
    assert int(keep_bits(0x9E3779B97F4A7C15, 0, 8, 0)) == 0x6E789E6AA1B965F4


def test_keep_threshold():
    assert keep_threshold(0.4) == 39322
    assert keep_threshold(0.5) == 32768
    assert keep_threshold(0.0) == 65536
    assert keep_threshold(0.25) == 49152
    # p is a float32 argument: float32(0.1) widened, not the double 0.1
    assert keep_threshold(0.1) == int((1.0 - float(np.float32(0.1))) * 65536.0 + 0.5)


def test_keep_mask_matches_scalar_restatement():
    n, h, w, c, p, seed = 2, 3, 5, 6, 0.4, 0x1234567 + 0x632BE59BD9B4E019
    m = keep_mask(seed, n, h, w, c, p)
    thr = keep_threshold(p)
    g4n = (c + 3) // 4
    for pix in range(n * h * w):
        for ch in range(c):
            want = bool(keep_one(keep_bits(seed, pix, g4n, ch >> 2), ch & 3, thr))
            assert m.reshape(-1, c)[pix, ch] == want, (pix, ch)


def test_keep_mask_bf16_keying():
    """The bf16 kernels: lane cg of a pixel holds channel octet cg and draws quads 2 cg and 2 cg + 1 of 2 CG."""
    n, h, w, p, seed = 1, 7, 9, 0.4, 987654321
    for cg_count in (1, 2, 4, 8, 16):
        c = 8 * cg_count
        m = keep_mask(seed, n, h, w, c, p, chunk_pixels=11).reshape(-1, c)
        thr = keep_threshold(p)
        pix = np.arange(n * h * w, dtype=np.uint64)[:, None]
        got = np.zeros_like(m)
        for cg in range(cg_count):
            for half in range(2):
                bits = keep_bits(seed, pix, 2 * cg_count, 2 * cg + half)
                for q in range(4):
                    got[:, 8 * cg + 4 * half + q] = keep_one(bits, q, thr)[:, 0]
        assert np.array_equal(m, got), c


def test_keep_mask_rate_and_lane_independence():
    n, h, w, c, p = 2, 128, 128, 32, 0.4
    m = keep_mask(0x0123456789ABCDEF, n, h, w, c, p).reshape(-1, c).astype(np.float64)
    pixels = m.shape[0]
    keep = keep_threshold(p) / 65536.0
    sigma = (keep * (1 - keep) / pixels) ** 0.5
    rate = m.mean(0)
    assert np.abs(rate - keep).max() < 5 * sigma, rate
    centred = (m - keep) / (keep * (1 - keep)) ** 0.5
    corr = centred.T @ centred / pixels
    off = corr - np.diag(np.diag(corr))
    assert np.abs(off).max() < 5 / pixels ** 0.5      # the four lanes of a quad included
    assert keep_mask(0, 1, 4, 4, 8, 0.0).all()         # p = 0 keeps every element
