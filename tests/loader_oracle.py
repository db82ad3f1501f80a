"""The device input pipeline (csrc/loader.hip) restated in numpy: the warp in float64 (or, with dtype=np.float32, in the
kernel's own operation order as an fp32 emulation), its a-priori error bound, the label transform, the draw of the
parameter rows, and the flip / rot90 / shift construction the dihedral maps are held against.  Shared by
tests/test_loader_host.py and tests/test_gpu_loader.py (test infrastructure; no GPU here).

Conventions: coordinates are pixel indices, a pixel centre is an integer; a row is 16 numbers -- [0..5] inverse map
(output pixel -> source position), [6..11] forward map (source -> output), [12] gain, [13] bias."""
import math

import numpy as np
import torch

from oracle.dropout_oracle import GOLDEN, mix64

U = 2.0 ** -24   # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------------------------
# the warp
def warp_plane(img, m, out_size, fill, dtype=np.float64):
    """img [C, Hs, Ws] (source units), m = the 6 inverse-map entries -> v [C, Ho, Wo]: bilinear sample of the image
    padded with `fill`, in `dtype` arithmetic with the kernel's order of operations (one rounding each)."""
    dt = dtype
    C, Hs, Ws = img.shape
    Ho, Wo = out_size
    m = [dt(e) for e in m]
    xo = np.arange(Wo, dtype=dt)[None, :]
    yo = np.arange(Ho, dtype=dt)[:, None]
    xs = (m[0] * xo + m[1] * yo) + m[2]
    ys = (m[3] * xo + m[4] * yo) + m[5]
    x0, y0 = np.floor(xs), np.floor(ys)
    reach = (x0 >= -2) & (x0 <= Ws) & (y0 >= -2) & (y0 <= Hs)
    fx = np.where(reach, xs - x0, dt(0)).astype(dt)
    fy = np.where(reach, ys - y0, dt(0)).astype(dt)
    xi = np.where(reach, x0, -2).astype(np.int64) + 2
    yi = np.where(reach, y0, -2).astype(np.int64) + 2
    pad = np.full((C, Hs + 4, Ws + 4), dt(fill), dtype=dt)
    pad[:, 2:2 + Hs, 2:2 + Ws] = img.astype(dt)
    gx, gy = dt(1) - fx, dt(1) - fy
    v00, v01 = pad[:, yi, xi], pad[:, yi, xi + 1]
    v10, v11 = pad[:, yi + 1, xi], pad[:, yi + 1, xi + 1]
    return ((gx * gy) * v00 + (fx * gy) * v01) + ((gx * fy) * v10 + (fx * fy) * v11)


def plane_bound(img, m, out_size, fill):
    """bound_v [C, Ho, Wo] in source units for one sample: dx*Dx + dy*Dy + 8u*Vmax, dx = 4u (|m0| xo + |m1| yo + |m2|),
    Dx / Dy = the largest horizontal / vertical neighbour difference of the image padded by one ring of fill."""
    C, Hs, Ws = img.shape
    Ho, Wo = out_size
    m = [abs(float(e)) for e in m]
    xo = np.arange(Wo, dtype=np.float64)[None, :]
    yo = np.arange(Ho, dtype=np.float64)[:, None]
    dx = 4 * U * (m[0] * xo + m[1] * yo + m[2])
    dy = 4 * U * (m[3] * xo + m[4] * yo + m[5])
    pad = np.full((C, Hs + 2, Ws + 2), float(fill))
    pad[:, 1:-1, 1:-1] = img.astype(np.float64)
    Dx = np.abs(np.diff(pad, axis=2)).max(axis=(1, 2))[:, None, None]
    Dy = np.abs(np.diff(pad, axis=1)).max(axis=(1, 2))[:, None, None]
    vmax = np.abs(pad).max(axis=(1, 2))[:, None, None]
    return dx[None] * Dx + dy[None] * Dy + 8 * U * vmax


def warp_batch_ref(store_nchw, index, rows, out_size, mul, add, fill):
    """store_nchw [M, C, Hs, Ws] (any dtype), index [N] ints, rows [N, 16] (the fp32 rows the kernel gets) ->
    (out [N, C, Ho, Wo] float64, bound of the same shape).  An index outside [0, M) is an all-fill sample."""
    store = np.asarray(store_nchw)
    M, C = store.shape[:2]
    rows = np.asarray(rows, dtype=np.float64)
    mul = np.broadcast_to(np.asarray(mul, dtype=np.float64), (C,))[:, None, None]
    add = np.broadcast_to(np.asarray(add, dtype=np.float64), (C,))[:, None, None]
    outs, bounds = [], []
    for n, idx in enumerate(index):
        idx = int(idx)
        img = store[idx].astype(np.float64) if 0 <= idx < M else np.full(store.shape[1:], float(fill))
        r = rows[n]
        v = warp_plane(img, r[:6], out_size, fill)
        out = r[12] * (v * mul + add) + r[13]
        bv = plane_bound(img, r[:6], out_size, fill)
        bounds.append(abs(r[12]) * np.abs(mul) * bv + 4 * U * (np.abs(out) + np.abs(r[12] * add) + abs(r[13])))
        outs.append(out)
    return np.stack(outs), np.stack(bounds)


def labels_ref(labels, index, rows, out_size):
    """labels [M, S, 2] -> (labels_out [N, S, 2] float64, inside [N, S] bool, bound [N, S, 2], margin [N, S]): the
    forward map in float64; bound = 4u (|f0| x + |f1| y + |f2|) per coordinate; margin = distance of a mapped label to
    the nearest frame edge (inf for sentinels).  Sentinels and out-of-range samples come out (-1, -1), not inside."""
    labels = np.asarray(labels, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    M, S = labels.shape[:2]
    Ho, Wo = out_size
    N = len(index)
    out = np.full((N, S, 2), -1.0)
    inside = np.zeros((N, S), dtype=bool)
    bound = np.zeros((N, S, 2))
    margin = np.full((N, S), np.inf)
    for n, idx in enumerate(index):
        idx = int(idx)
        if not 0 <= idx < M:
            continue
        f = rows[n, 6:12]
        for s in range(S):
            x, y = labels[idx, s]
            if x < 0 or y < 0:
                continue
            px, py = f[0] * x + f[1] * y + f[2], f[3] * x + f[4] * y + f[5]
            out[n, s] = (px, py)
            bound[n, s] = (4 * U * (abs(f[0]) * x + abs(f[1]) * y + abs(f[2])),
                           4 * U * (abs(f[3]) * x + abs(f[4]) * y + abs(f[5])))
            inside[n, s] = 0 <= px <= Wo - 1 and 0 <= py <= Ho - 1
            margin[n, s] = min(abs(px), abs(px - (Wo - 1)), abs(py), abs(py - (Ho - 1)))
    return out, inside, bound, margin


# ---------------------------------------------------------------------------------------------------------------
# rows
def rows_from_forward(fwd, gain=1.0, bias=0.0):
    """fwd [N, 2, 3] float64 -> rows [N, 16] float64 (closed-form inverse)."""
    fwd = np.asarray(fwd, dtype=np.float64).reshape(-1, 2, 3)
    N = fwd.shape[0]
    rows = np.zeros((N, 16))
    for n in range(N):
        (a, b, c), (d, e, f) = fwd[n]
        det = a * e - b * d
        ia, ib, id_, ie = e / det, -b / det, -d / det, a / det
        rows[n, :6] = (ia, ib, -(ia * c + ib * f), id_, ie, -(id_ * c + ie * f))
        rows[n, 6:12] = fwd[n].reshape(6)
    rows[:, 12] = gain
    rows[:, 13] = bias
    return rows


_QC = (1.0, 0.0, -1.0, 0.0)
_QS = (0.0, 1.0, 0.0, -1.0)


def forward_map(flip_x, flip_y, q, theta, s, t, src_size, out_size):
    """p_o = c_o + D R(theta) Q^q s (p_s - c_s - t) as a 2x3 matrix (float64); Q = [[0, -1], [1, 0]] as whole numbers."""
    (Hs, Ws), (Ho, Wo) = src_size, out_size
    dx, dy = (-1.0 if flip_x else 1.0), (-1.0 if flip_y else 1.0)
    ct, st = math.cos(theta), math.sin(theta)
    qc, qs = _QC[q], _QS[q]
    r00, r01 = ct * qc - st * qs, -ct * qs - st * qc
    r10, r11 = -r01, r00
    a00, a01, a10, a11 = s * dx * r00, s * dx * r01, s * dy * r10, s * dy * r11
    csx, csy, cox, coy = (Ws - 1) / 2.0, (Hs - 1) / 2.0, (Wo - 1) / 2.0, (Ho - 1) / 2.0
    px, py = csx + t[0], csy + t[1]
    return np.array([[a00, a01, cox - a00 * px - a01 * py], [a10, a11, coy - a10 * px - a11 * py]])


def inverse_map(flip_x, flip_y, q, theta, s, t, src_size, out_size):
    """p_s = c_s + t + (1/s) Q^-q R(-theta) D (p_o - c_o) as a 2x3 matrix (float64)."""
    (Hs, Ws), (Ho, Wo) = src_size, out_size
    dx, dy = (-1.0 if flip_x else 1.0), (-1.0 if flip_y else 1.0)
    ct, st = math.cos(theta), math.sin(theta)
    qc, qs = _QC[q], _QS[q]
    r00, r01 = ct * qc - st * qs, -ct * qs - st * qc
    r10, r11 = -r01, r00
    i = 1.0 / s
    b00, b01, b10, b11 = i * r00 * dx, i * r10 * dy, i * r01 * dx, i * r11 * dy
    csx, csy, cox, coy = (Ws - 1) / 2.0, (Hs - 1) / 2.0, (Wo - 1) / 2.0, (Ho - 1) / 2.0
    return np.array([[b00, b01, csx + t[0] - b00 * cox - b01 * coy], [b10, b11, csy + t[1] - b10 * cox - b11 * coy]])


DIHEDRAL = [(fx, q) for fx in (False, True) for q in range(4)]   # the eight elements: an optional flip in x, q turns


def dihedral_rows(elements_shifts, src_size, out_size):
    """rows [N, 16] float64 for [(flip_x, q, (tx, ty)), ...] -- whole numbers when the sizes have matching parity."""
    rows = np.zeros((len(elements_shifts), 16))
    for n, (fx, q, t) in enumerate(elements_shifts):
        rows[n, :6] = inverse_map(fx, False, q, 0.0, 1.0, t, src_size, out_size).reshape(6)
        rows[n, 6:12] = forward_map(fx, False, q, 0.0, 1.0, t, src_size, out_size).reshape(6)
        rows[n, 12] = 1.0
    return rows


def dihedral_torch(img, flip_x, q, t, out_size, fill, ring=64):
    """The same map built from torch.roll / rot90 / flip on a canvas of `fill`: img [C, Hs, Ws] tensor -> [C, Ho, Wo].
    The content moves by -t, turns q quarter turns clockwise about the centre, flips in x, and is cropped or padded
    about the centre."""
    C, Hs, Ws = img.shape
    Ho, Wo = out_size
    assert abs(t[0]) < ring and abs(t[1]) < ring
    canvas = torch.full((C, Hs + 2 * ring, Ws + 2 * ring), fill, dtype=img.dtype)
    canvas[:, ring:ring + Hs, ring:ring + Ws] = img
    canvas = torch.roll(canvas, shifts=(-int(t[1]), -int(t[0])), dims=(1, 2))
    canvas = torch.rot90(canvas, -q, dims=(1, 2))
    if flip_x:
        canvas = torch.flip(canvas, dims=(2,))
    Hc, Wc = canvas.shape[1:]
    assert (Hc - Ho) % 2 == 0 and (Wc - Wo) % 2 == 0 and Hc >= Ho and Wc >= Wo
    y0, x0 = (Hc - Ho) // 2, (Wc - Wo) // 2
    return canvas[:, y0:y0 + Ho, x0:x0 + Wo].contiguous()


def random_rows(rng, n, src_size, out_size, shift=20.0):
    """n general maps as float64 rows: any angle, scale 0.5 to 2, a flip, a real-valued shift of up to `shift` px, gain
    0.5 to 1.5, bias +-0.2."""
    fwd = []
    for _ in range(n):
        theta = rng.uniform(-math.pi, math.pi)
        s = math.exp(rng.uniform(math.log(0.5), math.log(2.0)))
        t = (rng.uniform(-shift, shift), rng.uniform(-shift, shift))
        fwd.append(forward_map(rng.random() < 0.5, rng.random() < 0.5, 0, theta, s, t, src_size, out_size))
    return rows_from_forward(np.stack(fwd), gain=rng.uniform(0.5, 1.5, n), bias=rng.uniform(-0.2, 0.2, n))


# ---------------------------------------------------------------------------------------------------------------
# the draw
def uniforms(seed, n, k):
    """u_k of samples n (array): (mix64(seed + GOLDEN (16 n + k + 1)) >> 40) * 2^-24, a 24-bit value."""
    n = np.asarray(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = n * np.uint64(16) + np.uint64(k + 1)
        bits = mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + GOLDEN * ctr)
    return (bits >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


def draw_ref(n, seed, src_size, out_size, flip_h=0.5, flip_v=0.5, rot90=True, rotate=0.0, scale=(1.0, 1.0),
             translate=(0, 0), contrast=(1.0, 1.0), brightness=0.0):
    """What unetpp_augment_draw draws -> dict(flip_x, flip_y, q, tx, ty: arrays [n]; rows: [n, 16] float64, not yet
    rounded to fp32).  The configuration goes through fp32 as it does on its way to the device."""
    f32 = lambda v: float(np.float32(v))   # noqa: E731
    ids = np.arange(n)
    u = [uniforms(seed, ids, k) for k in range(9)]
    flip_x, flip_y = u[0] < f32(flip_h), u[1] < f32(flip_v)
    q = np.floor(4.0 * u[2]).astype(np.int64) if rot90 else np.zeros(n, dtype=np.int64)
    theta = (2.0 * u[3] - 1.0) * f32(rotate) * (math.pi / 180.0)
    ln_lo, ln_hi = math.log(f32(scale[0])), math.log(f32(scale[1]))
    s = np.exp(ln_lo + u[4] * (ln_hi - ln_lo))
    tx = np.floor((2.0 * u[5] - 1.0) * f32(translate[0]) + 0.5)
    ty = np.floor((2.0 * u[6] - 1.0) * f32(translate[1]) + 0.5)
    gain = f32(contrast[0]) + u[7] * (f32(contrast[1]) - f32(contrast[0]))
    bias = (2.0 * u[8] - 1.0) * f32(brightness)
    rows = np.zeros((n, 16))
    for i in range(n):
        args = (bool(flip_x[i]), bool(flip_y[i]), int(q[i]), float(theta[i]), float(s[i]), (tx[i], ty[i]), src_size, out_size)
        rows[i, :6] = inverse_map(*args).reshape(6)
        rows[i, 6:12] = forward_map(*args).reshape(6)
    rows[:, 12], rows[:, 13] = gain, bias
    return dict(flip_x=flip_x, flip_y=flip_y, q=q, tx=tx, ty=ty, rows=rows)
