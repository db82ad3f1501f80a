"""The heads' in-kernel dropout keep mask restated in numpy (csrc/dropout.h).

One splitmix64 finaliser per (seed, pixel, channel quad) gives four 16-bit uniforms; channel c of a pixel is kept when
uniform number (c & 3) of quad c // 4 lies below a 16-bit threshold.  Pixel index = n*H*W + y*W + x, quad counter =
pixel * ceil(C/4) + quad + 1.  Every head kernel, fp32 and bf16, keys the mask this way (the bf16 kernels as two quads
per channel octet: 2*CG quads, quad 2*octet + half).  All arithmetic is uint64 and wraps, as on the device.
"""
import numpy as np
import torch

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def mix64(z):
    """splitmix64's finaliser on a uint64 array (or scalar)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def keep_bits(seed, pixel, cgroups4, g4):
    """mix64(seed + golden * (pixel * cgroups4 + g4 + 1)): the 64 bits of one channel quad of one pixel."""
    pixel = np.asarray(pixel, dtype=np.uint64)
    g4 = np.asarray(g4, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = pixel * np.uint64(cgroups4) + g4 + np.uint64(1)
        return mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + GOLDEN * ctr)


def keep_one(bits, c_in_group, thr16):
    """Keep flag of lane c_in_group (0..3) of a quad's bits."""
    bits = np.asarray(bits, dtype=np.uint64)
    lane = np.asarray(c_in_group, dtype=np.uint64)
    return ((bits >> (np.uint64(16) * lane)) & np.uint64(0xFFFF)) < np.uint64(thr16)


def keep_threshold(p_drop):
    """(uint32)((1 - (double)(float)p) * 65536 + 0.5), at most 65536 (p = 0 keeps everything)."""
    keep = 1.0 - float(np.float32(p_drop))
    t = int(keep * 65536.0 + 0.5)
    return min(t, 65536)


def keep_mask(seed, N, H, W, C, p_drop, chunk_pixels=1 << 20):
    """bool [N, H, W, C]: True where the head kernels keep x[n, y, x, c] for this seed and drop probability."""
    thr = np.uint64(keep_threshold(p_drop))
    g4n = (C + 3) // 4
    pixels = N * H * W
    out = np.empty((pixels, C), dtype=bool)
    quads = np.arange(g4n, dtype=np.uint64)
    lanes = (np.uint64(16) * np.arange(4, dtype=np.uint64))
    for p0 in range(0, pixels, chunk_pixels):
        p1 = min(pixels, p0 + chunk_pixels)
        pix = np.arange(p0, p1, dtype=np.uint64)[:, None]
        bits = keep_bits(seed, pix, g4n, quads[None, :])                    # [P, G]
        u16 = (bits[:, :, None] >> lanes[None, None, :]) & np.uint64(0xFFFF)  # [P, G, 4]: channel 4 g + lane
        out[p0:p1] = (u16 < thr).reshape(p1 - p0, 4 * g4n)[:, :C]
    return out.reshape(N, H, W, C)


class KeepMaskDropout(torch.nn.Module):
    """Stands in for the oracle's nn.Dropout in a training step whose heads drew their masks in the kernels: call i
    (head i + 1, in order; the count wraps for a second forward) applies keep_mask(seeds[i]) and scales by 1 / (1 - p).
    seeds: the step's per-head seeds (engine._Saved.seeds); shape (N, H, W, C) of the head inputs."""

    def __init__(self, seeds, N, H, W, C, p_drop):
        super().__init__()
        self.p = float(p_drop)
        self.masks = [torch.from_numpy(keep_mask(s, N, H, W, C, p_drop)).permute(0, 3, 1, 2) for s in seeds]
        self.calls = 0

    def forward(self, t):
        k = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        return t * k.to(t.dtype) / (1.0 - self.p)
