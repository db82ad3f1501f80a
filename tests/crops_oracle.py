"""Training on scenes (crops.py, csrc/crops.hip) restated in numpy: the target maps of warped windows by brute force over
all labels, the culling rule of the kernel restated beside it, the draw of the windows, and the label sets the tests
use.  Shared by tests/test_crops_host.py and tests/test_gpu_crops.py (test infrastructure; no GPU here).

Conventions: coordinates are (x, y) pixel indices, a pixel centre is an integer; a row is 16 numbers as in
tests/loader_oracle.py.  A label's position in the window is formed in float32 with the warp's own expression, one
rounding per operation; distances are float64."""
import math

import numpy as np

from tests import loader_oracle as lo

F32, F64 = np.float32, np.float64
TILE_H, TILE_W = 16, 64       # the kernel's pixel tile


# ---------------------------------------------------------------------------------------------------------------
# targets
def window_positions(xy32, row32):
    """xy32 [L, 2] float32, row32 [16] float32 -> (xo, yo) float32 [L]: (P0 x + P1 y) + P2 rounded after every step"""
    xy32, P = np.asarray(xy32, dtype=F32), np.asarray(row32, dtype=F32)[6:12]
    x, y = xy32[:, 0], xy32[:, 1]
    return (P[0] * x + P[1] * y) + P[2], (P[3] * x + P[4] * y) + P[5]


def valid_labels(labels32, classes, C):
    labels32, classes = np.asarray(labels32), np.asarray(classes)
    return (classes >= 0) & (classes < C) & ~(labels32[..., 0] < 0) & ~(labels32[..., 1] < 0)


def brute_minima(xo, yo, Ho, Wo):
    """least dx*dx + dy*dy over the positions (float32 arrays) for every pixel -> float64 [Ho, Wo]; inf without labels"""
    m = np.full((Ho, Wo), np.inf)
    px = np.arange(Wo, dtype=F64)[None, :]
    py = np.arange(Ho, dtype=F64)[:, None]
    for a, b in zip(np.asarray(xo, dtype=F64), np.asarray(yo, dtype=F64)):
        dx, dy = px - a, py - b
        m = np.minimum(m, dx * dx + dy * dy)
    return m


def value_of(m, radius):
    """float32(exp(-0.5 sqrt(m) / radius)) in float64"""
    with np.errstate(under="ignore"):
        return np.exp(-0.5 * np.sqrt(m) / F64(F32(radius))).astype(F32)


def points_target_ref(labels, label_class, index, rows, C, out_size, radius):
    """labels [M, L, 2], label_class [M, L], index [N], rows [N, 16] (float32 values) -> float32 [N, C, Ho, Wo]: per class
    the value of the least distance over ALL valid labels of the frame, exactly 0 where the class has none and for an
    index outside [0, M)."""
    labels = np.asarray(labels, dtype=F32)
    label_class = np.asarray(label_class)
    rows = np.asarray(rows, dtype=F32)
    M = labels.shape[0]
    Ho, Wo = out_size
    out = np.zeros((len(index), C, Ho, Wo), dtype=F32)
    for n, idx in enumerate(index):
        idx = int(idx)
        if not 0 <= idx < M:
            continue
        ok = valid_labels(labels[idx], label_class[idx], C)
        xo, yo = window_positions(labels[idx], rows[n])
        for c in range(C):
            pick = ok & (label_class[idx] == c)
            if pick.any():
                out[n, c] = value_of(brute_minima(xo[pick], yo[pick], Ho, Wo), radius)
    return out


def _axis_bounds(p, a, b):
    """least / greatest squared distance from positions p (float64 array) to the pixel centres a..b, formed from the
    same rounded differences as a pixel's own distance"""
    da, db = F64(a) - p, F64(b) - p
    qa, qb = da * da, db * db
    return np.where(p < a, qa, np.where(p > b, qb, 0.0)), np.maximum(qa, qb)


def culled_minima(xo, yo, Ho, Wo, tile=(TILE_H, TILE_W)):
    """The kernel's rule restated: per pixel tile keep label l iff lo_l <= min over l' of up_l' (least / greatest squared
    distance to the tile's rectangle of pixel centres), then the minimum over the kept labels alone.
    -> (float64 [Ho, Wo], the largest number of labels any tile kept)."""
    xo, yo = np.asarray(xo, dtype=F64), np.asarray(yo, dtype=F64)
    m = np.full((Ho, Wo), np.inf)
    most = 0
    for y0 in range(0, Ho, tile[0]):
        for x0 in range(0, Wo, tile[1]):
            y1, x1 = min(y0 + tile[0], Ho) - 1, min(x0 + tile[1], Wo) - 1
            lx, ux = _axis_bounds(xo, x0, x1)
            ly, uy = _axis_bounds(yo, y0, y1)
            lo_l, up_l = lx + ly, ux + uy
            keep = lo_l <= up_l.min()
            most = max(most, int(keep.sum()))
            px = np.arange(x0, x1 + 1, dtype=F64)[None, :]
            py = np.arange(y0, y1 + 1, dtype=F64)[:, None]
            part = np.full((y1 - y0 + 1, x1 - x0 + 1), np.inf)
            for a, b in zip(xo[keep], yo[keep]):
                dx, dy = px - a, py - b
                part = np.minimum(part, dx * dx + dy * dy)
            m[y0:y1 + 1, x0:x1 + 1] = part
    return m, most


def cull_cases():
    """(name, Ho, Wo, xo, yo) of the four CPU cases: scattered, far outside, thousands over a wide neighbourhood,
    coincident"""
    rng = np.random.default_rng(41)
    f = lambda a: np.asarray(a, dtype=F32)   # noqa: E731
    yield "7 scattered", 40, 48, f(rng.uniform(-5, 53, 7)), f(rng.uniform(-5, 45, 7))
    yield "300 up to 400 px outside", 33, 70, f(rng.uniform(-400, 470, 300)), f(rng.uniform(-400, 433, 300))
    yield "2000 over 4096 px", 64, 64, f(rng.uniform(-2016, 2080, 2000)), f(rng.uniform(-2016, 2080, 2000))
    yield "300 coincident", 40, 48, f(np.full(300, 17.25)), f(np.full(300, -3.5))


# ---------------------------------------------------------------------------------------------------------------
# label sets and rows of the target tests
X0, Y0 = 1200, 1100           # where the window sits in its frame under the identity row
KINDS = ("identity", "flip", "quarter", "general")


def window_row(kind, out_size):
    """float64 row [16] of a window whose top-left pixel is source pixel (X0, Y0): the identity, a flip in x, a quarter
    turn, or a rotation by 0.6 rad at scale 1.3 with a flip in y, all about the window's centre"""
    Ho, Wo = out_size
    centre = (X0 + (Wo - 1) / 2.0, Y0 + (Ho - 1) / 2.0)
    args = {"identity": (False, False, 0, 0.0, 1.0), "flip": (True, False, 0, 0.0, 1.0),
            "quarter": (False, False, 1, 0.0, 1.0), "general": (False, True, 0, 0.6, 1.3)}[kind]
    row = np.zeros(16)
    row[:6] = lo.inverse_map(*args, centre, (1, 1), out_size).reshape(6)
    row[6:12] = lo.forward_map(*args, centre, (1, 1), out_size).reshape(6)
    row[12] = 1.0
    return row


def target_case(N, C, Ho, Wo, L, first_kind=0, seed=0):
    """One input set of the target tests -> dict(labels [M, L, 2] f32, label_class [M, L] i32, index [N] i64, rows
    [N, 16] f32, kinds).  M = N frames; sample n reads frame n with transform KINDS[(first_kind + n) % 4], except that
    with N >= 3 sample 1 has an index outside [0, M).  Planted, as L allows (positions under the identity row):
      l = 0, 1   class 0, inside the window, two pixels apart in x: the pixel between them is equidistant from both
      l = 2      the sentinel (-1, -1) with a live class          l = 3   a live position with class -1
      l = 4      lands at exactly (-1, -1)                        l = 5   the only label of class min(2, C - 1), about 540 px
                                                                         away: float32 denormals and zeros in the window
    and the rest at random, a third inside the window and the others up to 1000 px outside it, some of them sentinels or
    of a class outside 0..C-1.  With C = 4 class 3 has no label at all."""
    rng = np.random.default_rng(1000 * seed + 7 * L + Ho)
    M = N
    far = min(2, C - 1)
    low = 1 if C >= 3 else 0                      # the class of l = 4 and of half the random labels
    labels = np.zeros((M, L, 2), dtype=F32)
    classes = np.zeros((M, L), dtype=np.int32)
    for m in range(M):
        x = rng.uniform(X0 - 1000, X0 + Wo + 1000, L)
        y = rng.uniform(Y0 - 1000, Y0 + Ho + 1000, L)
        near = rng.random(L) < 1.0 / 3.0
        x[near], y[near] = rng.uniform(X0, X0 + Wo - 1, near.sum()), rng.uniform(Y0, Y0 + Ho - 1, near.sum())
        cls = np.where(rng.random(L) < 0.5, 0, low)
        odd = rng.random(L)
        cls = np.where(odd < 0.05, C, np.where(odd < 0.10, -1, cls))          # outside the class range
        gone = (odd > 0.95)
        x[gone], y[gone] = -1.0, -1.0                                         # sentinels
        ax, ay = X0 + Wo // 3 + m, Y0 + Ho // 2 - m
        plant = [(ax, ay, 0), (ax + 2, ay, 0), (-1, -1, 0), (X0 + 3, Y0 + 4, -1), (X0 - 1, Y0 - 1, low),
                 (X0 + Wo + 500, Y0 - 200, far)]
        for l, (a, b, c) in enumerate(plant[:L]):
            x[l], y[l], cls[l] = a, b, c
        if L == 1:
            x[0], y[0] = ax + 0.25, ay - 0.5       # a lone label off the pixel grid
        labels[m, :, 0], labels[m, :, 1], classes[m] = x, y, cls
    index = np.arange(N, dtype=np.int64)
    if N >= 3:
        index[1] = M + 2
    kinds = [KINDS[(first_kind + n) % 4] for n in range(N)]
    rows = np.stack([window_row(k, (Ho, Wo)) for k in kinds]).astype(F32)
    return dict(labels=labels, label_class=classes, index=index, rows=rows, kinds=kinds)


# ---------------------------------------------------------------------------------------------------------------
# the draw
def _origin(centre, src, win):
    if src < win:
        return np.full(centre.shape, -((win - src) // 2), dtype=np.int64)
    return np.clip(centre - win // 2, 0, src - win).astype(np.int64)


def crops_draw_ref(n, seed, M, src_size, out_size, centre_frame, centre_xy, p_object, jitter, flip_h=0.5, flip_v=0.5,
                   rot90=True, rotate=0.0, scale=(1.0, 1.0), contrast=(1.0, 1.0), brightness=0.0):
    """What unetpp_crops_draw draws -> dict(object: bool [n]; index: int64 [n]; origin: int64 [n, 2] as (ox, oy); rows:
    [n, 16] float64, not yet rounded to fp32).  The configuration goes through fp32 as it does on its way to the device."""
    f32 = lambda v: float(F32(v))   # noqa: E731
    (Hs, Ws), (Ho, Wo) = src_size, out_size
    ids = np.arange(n)
    u = [lo.uniforms(seed, ids, k) for k in range(13)]
    frame_tab = np.asarray(centre_frame, dtype=np.int64).reshape(-1)
    xy_tab = np.asarray(centre_xy, dtype=F32).reshape(-1, 2).astype(F64)
    V = frame_tab.size
    obj = (u[9] < f32(p_object)) if V > 0 else np.zeros(n, dtype=bool)
    pick = lambda uu, count: np.minimum(np.floor(uu * count), count - 1)   # noqa: E731
    frame = pick(u[10], M).astype(np.int64)
    cx, cy = pick(u[11], Ws), pick(u[12], Hs)
    if V > 0:
        j = pick(u[10], V).astype(np.int64)
        ocx = np.floor(xy_tab[j, 0] + 0.5) + np.floor((2.0 * u[11] - 1.0) * f32(jitter[0]) + 0.5)
        ocy = np.floor(xy_tab[j, 1] + 0.5) + np.floor((2.0 * u[12] - 1.0) * f32(jitter[1]) + 0.5)
        frame, cx, cy = np.where(obj, frame_tab[j], frame), np.where(obj, ocx, cx), np.where(obj, ocy, cy)
    ox, oy = _origin(cx, Ws, Wo), _origin(cy, Hs, Ho)
    index = np.where((frame >= 0) & (frame < M), frame, -1)

    flip_x, flip_y = u[0] < f32(flip_h), u[1] < f32(flip_v)
    q = np.floor(4.0 * u[2]).astype(np.int64) if rot90 else np.zeros(n, dtype=np.int64)
    theta = (2.0 * u[3] - 1.0) * f32(rotate) * (math.pi / 180.0)
    ln_lo, ln_hi = math.log(f32(scale[0])), math.log(f32(scale[1]))
    s = np.exp(ln_lo + u[4] * (ln_hi - ln_lo))
    gain = f32(contrast[0]) + u[7] * (f32(contrast[1]) - f32(contrast[0]))
    bias = (2.0 * u[8] - 1.0) * f32(brightness)
    rows = np.zeros((n, 16))
    for i in range(n):
        centre = (ox[i] + (Wo - 1) / 2.0, oy[i] + (Ho - 1) / 2.0)     # takes the place of c_s + t
        args = (bool(flip_x[i]), bool(flip_y[i]), int(q[i]), float(theta[i]), float(s[i]), centre, (1, 1), out_size)
        rows[i, :6] = lo.inverse_map(*args).reshape(6)
        rows[i, 6:12] = lo.forward_map(*args).reshape(6)
    rows[:, 12], rows[:, 13] = gain, bias
    return dict(object=obj, index=index, origin=np.stack([ox, oy], axis=1), rows=rows, flip_x=flip_x, flip_y=flip_y, q=q)
