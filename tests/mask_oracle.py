"""Ignore masks (ignore.py: IgnoreMask / IgnoreUnion, csrc/mask.hip) restated in numpy.  Shared by
tests/test_mask_host.py and tests/test_gpu_mask.py (test infrastructure; no GPU here).

  * the pack layout: bit x & 31 of word x >> 5 of a row is pixel x, tail bits zero;
  * the polygon rule, the float64 expression operation for operation (numpy rounds every operation on its own), and
    the same rule in whole numbers for coordinates that are multiples of 1 / 256;
  * the lookup rule and ``mark_mask_bits``, built on ignore_oracle.source_positions;
  * the case generators of both test files, and MUTATIONS: what the host tests plant and the cases must catch.
"""
import functools

import numpy as np

from tests import ignore_oracle as io

F32, F64, I32, U32 = np.float32, np.float64, np.int32, np.uint32

EDGE_CHUNK = 256          # csrc/mask.hip kEdgeChunk: edges of a ring held in LDS at a time
TILE_H, TILE_W = 16, 64   # its tile

MUTATIONS = ("endpoints_not_ordered", "d_ge_zero", "straddle_upper_inclusive", "closing_edge_dropped",
             "clear_rings_ignored", "list_order_reversed", "floor_not_nearest", "class_plane_for_every_class",
             "tail_bits_not_zeroed", "cull_drops_touching_row")


# ---------------------------------------------------------------------------------------------------------------------
# the layout
def nonzero(mask):
    """the pack rule: set iff !(v == 0) -- a NaN sets the bit, -0.0 does not"""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(mask) == 0)


def pack(on, mutation=None):
    """bool [..., W] -> int32 [..., ceil(W / 32)]"""
    on = np.asarray(on, bool)
    w = on.shape[-1]
    wd = (w + 31) // 32
    padded = np.zeros(on.shape[:-1] + (wd * 32,), np.uint8)
    padded[..., :w] = on
    if mutation == "tail_bits_not_zeroed":
        padded[..., w:] = 1
    return np.packbits(padded, axis=-1, bitorder="little").view(U32).view(I32).reshape(on.shape[:-1] + (wd,))


def unpack(bits, w):
    """int32 [..., Wd] -> bool [..., W]; the tail bits are dropped (tails() tells what they hold)"""
    b = np.ascontiguousarray(np.asarray(bits, I32)).view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little")[..., :w].astype(bool)


def tails(bits, w):
    """the bits of the last word of every row above pixel W - 1, as one or-ed word (0: the tails are clean)"""
    if w % 32 == 0:
        return 0
    last = np.asarray(bits, I32)[..., -1].view(U32)
    return int(np.bitwise_or.reduce((last >> U32(w % 32)).ravel()))


# ---------------------------------------------------------------------------------------------------------------------
# the polygon rule
def ring_is_padding(verts32, count, V):
    if count < 3 or count > V:
        return True
    return not np.isfinite(np.asarray(verts32, F32)[:count]).all()


def ring_inside(verts32, size, mutation=None):
    """bool [H, W]: the pixels inside one ring (verts32 [n, 2] float32, all used), float64, operation for operation"""
    H, W = size
    v = np.asarray(verts32, F32).astype(F64)
    n = len(v)
    px = np.arange(W, dtype=F64)[None, :]
    py = np.arange(H, dtype=F64)[:, None]
    toggles = np.zeros((H, W), np.int64)
    edges = n - 1 if mutation == "closing_edge_dropped" else n
    for i in range(edges):
        (xa, ya), (xb, yb) = v[i], v[(i + 1) % n]
        if ya > yb and mutation != "endpoints_not_ordered":
            x0, y0, x1, y1 = xb, yb, xa, ya
        else:
            x0, y0, x1, y1 = xa, ya, xb, yb
        if y0 == y1:
            continue
        if mutation == "straddle_upper_inclusive":
            straddles = (y0 < py) & (py <= y1)
        else:
            straddles = (y0 <= py) & (py < y1)         # (unordered endpoints: a descending edge straddles nothing)
        a = F64(x1 - x0) * (py - y0)
        b = (px - x0) * F64(y1 - y0)
        d = a - b
        hit = (d >= 0) if mutation == "d_ge_zero" else (d > 0)
        toggles += straddles & hit
    return (toggles & 1).astype(bool)


def _cull_rows(verts32, H, mutation):
    """bool [H]: the rows whose tile keeps the ring (all True without the planted mutation: culling changes nothing)"""
    keep = np.ones(H, bool)
    if mutation != "cull_drops_touching_row":
        return keep
    ymin = F32(np.min(np.asarray(verts32, F32)[:, 1]))
    for y_lo in range(0, H, TILE_H):
        y_hi = min(y_lo + TILE_H, H) - 1
        if not F32(y_hi) > ymin:                       # (the rule: y_hi >= ymin)
            keep[y_lo:y_hi + 1] = False
    return keep


def polygons(vertices, counts, size, poly_plane=None, poly_clear=None, planes=1, mutation=None):
    """unetpp_mask_polygons -> bool [S, P, H, W].  vertices [S, G, V, 2] float32, counts [S, G]"""
    vertices = np.asarray(vertices, F32)
    S, G, V = vertices.shape[:3]
    H, W = size
    counts = np.asarray(counts).reshape(S, G)
    plane = np.zeros((S, G), int) if poly_plane is None else np.broadcast_to(np.asarray(poly_plane), (S, G))
    clear = np.zeros((S, G), bool) if poly_clear is None else np.broadcast_to(np.asarray(poly_clear), (S, G)).astype(bool)
    out = np.zeros((S, planes, H, W), bool)
    order = range(G - 1, -1, -1) if mutation == "list_order_reversed" else range(G)
    for s in range(S):
        for g in order:
            n, p = int(counts[s, g]), int(plane[s, g])
            if ring_is_padding(vertices[s, g], n, V) or not 0 <= p < planes:
                continue
            inside = ring_inside(vertices[s, g, :n], size, mutation) & _cull_rows(vertices[s, g, :n], H, mutation)[:, None]
            if clear[s, g]:
                if mutation != "clear_rings_ignored":
                    out[s, p] &= ~inside
            else:
                out[s, p] |= inside
    return out


def ring_inside_int(verts_q, size, unit=256):
    """the rule in whole numbers: verts_q [n, 2] integers, the coordinates times `unit` -> bool [H, W] (int64: exact
    for |coordinate| < 2^20 pixels)"""
    H, W = size
    v = np.asarray(verts_q, np.int64)
    n = len(v)
    px = np.arange(W, dtype=np.int64)[None, :] * unit
    py = np.arange(H, dtype=np.int64)[:, None] * unit
    toggles = np.zeros((H, W), np.int64)
    for i in range(n):
        (x0, y0), (x1, y1) = v[i], v[(i + 1) % n]
        if y0 > y1:
            x0, y0, x1, y1 = x1, y1, x0, y0
        if y0 == y1:
            continue
        d = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)
        toggles += (y0 <= py) & (py < y1) & (d > 0)
    return (toggles & 1).astype(bool)


# ---------------------------------------------------------------------------------------------------------------------
# the lookup rule
def nearest_pixel(xs32, ys32, size, mutation=None):
    """-> (in_frame bool, xi, yi int64) of float32 positions; xi / yi are 0 where the position is not in the frame"""
    H, W = size
    xs, ys = np.asarray(xs32, F32), np.asarray(ys32, F32)
    with np.errstate(invalid="ignore"):
        inside = (0 <= xs) & (xs <= F32(W - 1)) & (0 <= ys) & (ys <= F32(H - 1))
    x = np.where(inside, xs, F32(0))
    y = np.where(inside, ys, F32(0))
    if mutation == "floor_not_nearest":
        xi, yi = np.floor(x), np.floor(y)
    else:
        xi, yi = np.floor((x + F32(0.5)).astype(F32)), np.floor((y + F32(0.5)).astype(F32))
    return inside, np.clip(xi.astype(np.int64), 0, W - 1), np.clip(yi.astype(np.int64), 0, H - 1)


def _applies(k, cls, C, mutation):
    """does a plane of class k apply to class cls (array)"""
    if k == -1:
        return np.ones(np.shape(cls), bool)
    if mutation == "class_plane_for_every_class":
        return np.ones(np.shape(cls), bool)
    if k < 0 or (C is not None and k >= C):
        return np.zeros(np.shape(cls), bool)
    return np.asarray(cls) == k


def contains(raster, plane_class, frame, cls, xy, mutation=None):
    """IgnoreMask.contains: raster bool [S, P, H, W], plane_class [P]; frame / cls broadcastable to xy[..., 0]"""
    raster = np.asarray(raster, bool)
    S, P, H, W = raster.shape
    xy = np.asarray(xy, F32)
    x, y = xy[..., 0], xy[..., 1]
    frame = np.broadcast_to(np.asarray(frame), x.shape)
    cls = np.broadcast_to(np.asarray(cls), x.shape)
    inside, xi, yi = nearest_pixel(x, y, (H, W), mutation)
    known = inside & (frame >= 0) & (frame < S)
    f = np.clip(frame, 0, S - 1)
    out = np.zeros(x.shape, bool)
    for p in range(P):
        out |= raster[f, p, yi, xi] & _applies(int(plane_class[p]), cls, None, mutation)
    return out & known


def mark_mask_bits(raster, plane_class, index, rows, C, out_size, outside, mutation=None, n_frames=None):
    """bool [N, C, Ho, Wo]: the elements unetpp_target_ignore_mask sets to -1.  raster bool [M, P, Hs, Ws] (P may be 0:
    give n_frames then), plane_class [P], index [N], rows [N, 16]."""
    raster = np.asarray(raster, bool)
    M, P, Hs, Ws = raster.shape
    M = M if n_frames is None else n_frames
    Ho, Wo = out_size
    N = len(index)
    out = np.zeros((N, C, Ho, Wo), bool)
    cls = np.arange(C).reshape(C, 1, 1)
    for n in range(N):
        idx = int(index[n])
        live = 0 <= idx < M
        xs, ys = io.source_positions(np.asarray(rows, F32)[n], Ho, Wo)
        inside, xi, yi = nearest_pixel(xs, ys, (Hs, Ws), mutation)
        if live:
            for p in range(P):
                hit = raster[idx, p][yi, xi] & inside
                out[n] |= hit[None] & _applies(int(plane_class[p]), np.broadcast_to(cls, (C, Ho, Wo)), C, mutation)
        if outside:
            out[n] |= ~(inside & live)[None]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# polygon cases
POLY_FRAMES = ((33, 70), (129, 257))      # (H, W)
POLY_G = (0, 1, 40)
POLY_PLANES = 3
LONG_RING = EDGE_CHUNK + 44               # vertices of the ring that needs a second chunk of edges


def _q(a):
    """round to multiples of 1 / 256: d is then exact in float64 for frame-sized coordinates"""
    return (np.round(np.asarray(a, F64) * 256.0) / 256.0).astype(F32)


def _star(cx, cy, r_out, r_in, n, phase=0.0):
    t = phase + 2.0 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, r_out, r_in)
    return _q(np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1))


def _convex(rng, cx, cy, r, n):
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1)


@functools.lru_cache(maxsize=None)
def polygon_case(H, W, G, seed=0):
    """-> dict(vertices [S, G, V, 2] f32, counts [S, G] i32, poly_plane, poly_clear [S, G] i32, planes, size).  S = 2.
    G = 40 plants, per frame (the rest random convex rings of 3..9 vertices, any plane, a quarter of them clearing,
    half of them on the 1 / 256 grid, some across the frame's edges):
      0  an axis-aligned ring on integer corners: level edges, vertices on pixel centres, d == 0 along its sides
      1  a triangle                                   2  a convex ring of 7 vertices
      3  a star of LONG_RING vertices over most of the frame: a second chunk of edges
      4  a clearing ring inside it: a hole            5  a ring inside the hole: an island
      6  a ring wholly outside the frame              7  the whole frame, with a NaN vertex: padding
      8  two vertices: padding                        9  plane 1      10  plane 2      11  plane 5: padding
      12 rows 15 <= y < 15.5: touches the first tile row by exactly its last pixel row
      13 the whole frame, with an inf vertex: padding 14 a bow tie (self-intersecting)
      15 a triangle from x = -3e7 into the frame      16 a triangle from the frame out to x = 3e7
      17 the last row of the frame alone              18 a count above V: padding
    G = 1: the star in frame 0, the convex ring of 7 in frame 1.  G = 0: nothing."""
    rng = np.random.default_rng(4100 + 13 * seed + H + 7 * G)
    S, V = 2, (LONG_RING if G else 4)
    vertices = np.zeros((S, G, V, 2), F32)
    counts = np.zeros((S, G), I32)
    plane = np.zeros((S, G), I32)
    clear = np.zeros((S, G), I32)
    nan, inf = float("nan"), float("inf")
    for s in range(S):
        cx, cy, r = W / 2.0 + s, H / 2.0 - s, min(H, W) / 2.0 - 1.5
        star = _star(cx, cy, r, 0.6 * r, LONG_RING, 0.1 * s)
        seven = _q(_convex(rng, cx, cy, 0.8 * r, 7))
        if G == 1:
            rings = [(star if s == 0 else seven, 0, 0)]
        elif G == 0:
            rings = []
        else:
            whole = [(-2, -2), (W + 2, -2), (W + 2, H + 2), (-2, H + 2)]
            rings = [([(3, 2), (W - 20 + s, 2), (W - 20 + s, 11), (3, 11)], 0, 0),
                     (_q(_convex(rng, W * 0.3, H * 0.6, 0.25 * r + 2, 3)), 0, 0),
                     (seven, 0, 0),
                     (star, 0, 0),
                     (_q(_convex(rng, cx, cy, 0.4 * r, 8)), 0, 1),
                     (_q(_convex(rng, cx, cy, 0.2 * r, 5)), 0, 0),
                     ([(W + 10, 5), (W + 40, 5), (W + 25, 30)], 0, 0),
                     ([whole[0], whole[1], (nan, 3.0), whole[2], whole[3]], 0, 0),
                     ([(1, 1), (30, 30)], 0, 0),
                     (_q(_convex(rng, cx, cy, 0.7 * r, 6)), 1, 0),
                     (_q(_convex(rng, cx - 3, cy + 2, 0.5 * r, 9)), 2, 0),
                     (whole, 5, 0),
                     ([(W - 18.0, 15.0), (W - 2.5, 15.0), (W - 2.5, 15.5), (W - 18.0, 15.5)], 0, 0),
                     ([whole[0], whole[1], whole[2], (3.0, inf)], 0, 0),
                     ([(W - 16, 18), (W - 3, 30), (W - 3, 18), (W - 16, 30)], 1, 0),
                     ([(-3e7, H * 0.5), (W * 0.25, H * 0.25 + 0.125), (W * 0.25, H * 0.75)], 2, 0),
                     ([(W * 0.75, H * 0.25), (3e7, H * 0.5 + 0.5), (W * 0.75, H * 0.75)], 2, 0),
                     ([(2, H - 1), (W - 5.5, H - 1), (W - 5.5, H + 3), (2, H + 3)], 1, 0),
                     (whole, 0, 0)]
            while len(rings) < G:
                n = int(rng.integers(3, 10))
                ring = _convex(rng, rng.uniform(-4, W + 4), rng.uniform(-4, H + 4), rng.uniform(1.5, 0.3 * r + 2), n)
                ring = _q(ring) if len(rings) % 2 else ring.astype(F32)
                rings.append((ring, int(rng.integers(0, POLY_PLANES)), int(rng.random() < 0.25)))
        for g, (ring, p, c) in enumerate(rings):
            ring = np.asarray(ring, F32)
            vertices[s, g, :len(ring)] = ring
            vertices[s, g, len(ring):] = nan                      # unused vertices are never read into a result
            counts[s, g], plane[s, g], clear[s, g] = len(ring), p, c
        if G > 1:
            counts[s, 18] = V + 1
    for a in (vertices, counts, plane, clear):
        a.setflags(write=False)
    return dict(vertices=vertices, counts=counts, poly_plane=plane, poly_clear=clear, planes=POLY_PLANES, size=(H, W))


@functools.lru_cache(maxsize=None)
def polygon_expected(H, W, G, seed=0, mutation=None):
    """the oracle's raster of polygon_case, computed once and shared (read-only)"""
    c = polygon_case(H, W, G, seed)
    out = polygons(c["vertices"], c["counts"], c["size"], c["poly_plane"], c["poly_clear"], c["planes"], mutation)
    out.setflags(write=False)
    return out


def permuted_sets(case, seed=0):
    """the case with its rings permuted inside every run of consecutive non-clearing rings: no clearing ring changes
    its place among the others, so no bit may change"""
    rng = np.random.default_rng(77 + seed)
    out = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    S, G = case["counts"].shape
    for s in range(S):
        perm, run = [], []
        for g in range(G):
            if case["poly_clear"][s, g]:
                perm += list(rng.permutation(run)) + [g]
                run = []
            else:
                run.append(g)
        perm += list(rng.permutation(run))
        perm = np.asarray(perm, int)
        for k in ("vertices", "counts", "poly_plane", "poly_clear"):
            out[k][s] = case[k][s][perm]
    return out


def case_facts(case):
    """what the planted rings of a case exercise -> dict of bools / counts (asserted by the host tests)"""
    v, counts = case["vertices"], case["counts"]
    H, W = case["size"]
    S, G, V = v.shape[:3]
    facts = dict(level_edge=False, vertex_on_centre=False, d_zero=False, long_ring=False, outside_ring=False,
                 nan_ring=False, inf_ring=False, clear_ring=bool(np.any(case["poly_clear"])),
                 planes_used=len(set(int(p) for p in np.unique(case["poly_plane"]) if 0 <= p < case["planes"])))
    px = np.arange(W, dtype=F64)[None, :]
    py = np.arange(H, dtype=F64)[:, None]
    for s in range(S):
        for g in range(G):
            n = int(counts[s, g])
            if n < 3 or n > V:
                continue
            ring = v[s, g, :n]
            if np.isnan(ring).any():
                facts["nan_ring"] = True
            if np.isinf(ring).any():
                facts["inf_ring"] = True
            if not np.isfinite(ring).all():
                continue
            facts["long_ring"] |= n > EDGE_CHUNK
            facts["outside_ring"] |= bool(ring[:, 0].min() > W - 1 or ring[:, 0].max() < 0 or ring[:, 1].min() > H - 1
                                          or ring[:, 1].max() < 0)
            whole = (ring == np.round(ring)).all(axis=1) & (ring[:, 0] >= 0) & (ring[:, 0] < W) & (ring[:, 1] >= 0) & \
                (ring[:, 1] < H)
            facts["vertex_on_centre"] |= bool(whole.any())
            r64 = ring.astype(F64)
            for i in range(n):
                (x0, y0), (x1, y1) = r64[i], r64[(i + 1) % n]
                if y0 > y1:
                    x0, y0, x1, y1 = x1, y1, x0, y0
                if y0 == y1:
                    facts["level_edge"] = True
                    continue
                if n > 16:
                    continue
                d = F64(x1 - x0) * (py - y0) - (px - x0) * F64(y1 - y0)
                facts["d_zero"] |= bool(((y0 <= py) & (py < y1) & (d == 0)).any())
    return facts


# ---------------------------------------------------------------------------------------------------------------------
# mark cases
DIHEDRAL = tuple((fx, False, q, 0.0, 1.0) for fx in (False, True) for q in (0, 1, 2, 3))      # the eight flips and turns


def window_row8(code, origin, out_size):
    """float64 row [16] of a window whose top-left pixel under the identity is source pixel origin = (ox, oy), under
    dihedral element DIHEDRAL[code] about the window's centre (ignore_oracle.window_row for all eight)"""
    from tests import loader_oracle as lo
    Ho, Wo = out_size
    centre = (origin[0] + (Wo - 1) / 2.0, origin[1] + (Ho - 1) / 2.0)
    row = np.zeros(16)
    row[:6] = lo.inverse_map(*DIHEDRAL[code], centre, (1, 1), out_size).reshape(6)
    row[6:12] = lo.forward_map(*DIHEDRAL[code], centre, (1, 1), out_size).reshape(6)
    row[12] = 1.0
    return row


def region_raster(M, P, src_size, box, seed=0, full_planes=()):
    """bool [M, P, Hs, Ws]: zero but for the box (x_lo, y_lo, x_hi, y_hi), clipped to the frame, where coarse blocks of
    5 x 3 pixels are on with probability 0.35 and single pixels flip with probability 0.1; a plane in full_planes is
    all ones inside the box"""
    rng = np.random.default_rng(5200 + seed)
    Hs, Ws = src_size
    x_lo, y_lo, x_hi, y_hi = max(box[0], 0), max(box[1], 0), min(box[2], Ws - 1), min(box[3], Hs - 1)
    h, w = y_hi - y_lo + 1, x_hi - x_lo + 1
    out = np.zeros((M, P, Hs, Ws), bool)
    for m in range(M):
        for p in range(P):
            coarse = rng.random(((h + 2) // 3, (w + 4) // 5)) < 0.35
            fine = np.repeat(np.repeat(coarse, 3, axis=0), 5, axis=1)[:h, :w] ^ (rng.random((h, w)) < 0.1)
            out[m, p, y_lo:y_hi + 1, x_lo:x_hi + 1] = True if p in full_planes else fine
    return out


def mark_planes(C, P):
    """plane classes of the mark cases: every class, class 0, class min(1, C - 1), and C -- a plane of no class, which
    the cases fill with ones"""
    return np.asarray([-1, 0, min(1, C - 1), C][:P], I32)


def mark_case(N, C, Ho, Wo, P, first_kind=0, seed=0):
    """ignore_oracle.mark_case's windows (index, rows, kinds, src_size: the four window kinds in turn, an index outside
    [0, M) with N >= 3) over rasters that are busy about the window -> dict(raster [M, P, Hs, Ws] bool, plane_class,
    index, rows, kinds, src_size)"""
    from tests import crops_oracle as co
    base = io.mark_case(N, C, Ho, Wo, 0, first_kind=first_kind, seed=seed)
    box = (co.X0 - 80, co.Y0 - 80, co.X0 + Wo + 80, co.Y0 + Ho + 80)
    raster = region_raster(N, P, base["src_size"], box, seed=seed + 3 * P + Ho, full_planes=(3,))
    return dict(raster=raster, plane_class=mark_planes(C, P), index=base["index"], rows=base["rows"], kinds=base["kinds"],
                src_size=base["src_size"])


@functools.lru_cache(maxsize=None)
def dihedral_case(Ho, Wo, seed=0):
    """A frame of 50 x 30 (Hs x Ws), as ignore_oracle.outside_case: eleven samples -- the eight flips and turns at an
    origin that overhangs the frame on the left and right, one shifted to overhang the bottom, one general (rotated and
    scaled) window, and one with index -1.  C = 3, P = 4, two frames."""
    Hs, Ws, C, P = 50, 30, 3, 4
    spec = [(code, (-9, 4 + code), code % 2) for code in range(8)] + [(0, (-9, 25), 1), (5, (3, -7), 0), (0, (-9, 4), -1)]
    rows = np.stack([window_row8(c, o, (Ho, Wo)) for c, o, _ in spec])
    rows[9] = io.window_row("general", (-9, 5), (Ho, Wo))
    raster = region_raster(2, P, (Hs, Ws), (0, 0, Ws - 1, Hs - 1), seed=seed + 40, full_planes=(3,))
    return dict(raster=raster, plane_class=mark_planes(C, P), index=np.asarray([s[2] for s in spec], np.int64),
                rows=rows.astype(F32), src_size=(Hs, Ws), C=C, out_size=(Ho, Wo))


def affine_rows(Ho, Wo, centre, seed=0, n=4):
    """opt-in rotation and scale: forward maps [n, 2, 3] about `centre` of the frame for loader.affine_params"""
    rng = np.random.default_rng(6100 + seed)
    out = np.zeros((n, 2, 3))
    for i in range(n):
        th, s = rng.uniform(-np.pi, np.pi), rng.uniform(0.6, 1.7)
        a = s * np.asarray([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        c_out = np.asarray([(Wo - 1) / 2.0, (Ho - 1) / 2.0])
        out[i, :, :2] = a
        out[i, :, 2] = c_out - a @ (np.asarray(centre, F64) + rng.uniform(-3, 3, 2))
    return out


def rects_raster(rects, rect_class, C, src_size):
    """whole-number rectangles [M, R, 4] (both ends inclusive, as IgnoreRegions) -> (raster [M, C + 1, Hs, Ws],
    plane_class [-1, 0 .. C - 1]): what the rectangle path ignores at whole-number positions"""
    rects = np.asarray(rects, F32)
    M, R = rects.shape[:2]
    Hs, Ws = src_size
    out = np.zeros((M, C + 1, Hs, Ws), bool)
    for m in range(M):
        for (x0, y0, x1, y1), k in zip(rects[m], np.asarray(rect_class)[m]):
            k = int(k)
            if not (k == -1 or 0 <= k < C) or not np.isfinite([x0, y0, x1, y1]).all() or x1 < x0 or y1 < y0:
                continue
            xa, ya = int(max(np.ceil(x0), 0)), int(max(np.ceil(y0), 0))
            xb, yb = int(min(np.floor(x1), Ws - 1)), int(min(np.floor(y1), Hs - 1))
            if xa <= xb and ya <= yb:
                out[m, k + 1, ya:yb + 1, xa:xb + 1] = True
    return out, np.arange(-1, C, dtype=I32)


# ---------------------------------------------------------------------------------------------------------------------
# the partition property
PARTITION_SIZE = (40, 44)


def partition_case(seed=0):
    """A convex ring of 9..13 vertices on the 1 / 256 grid about (20, 18), cut by a chord through two of its vertices
    into two rings.  The two are the whole-number points (20 +- 12, 18 +- 9): the chord passes through seven pixel
    centres, where d == 0 for both halves.  -> dict(whole, left, right: float32 [n, 2]; whole_q, left_q, right_q: the
    same times 256 as integers)"""
    rng = np.random.default_rng(8300 + seed)
    n = int(rng.integers(7, 12))
    t = np.sort(np.concatenate([rng.uniform(0, 2 * np.pi, n), [np.arctan2(9, 12), np.arctan2(-9, -12) + 2 * np.pi]]))
    ring = _q(np.stack([20 + 15 * np.cos(t), 18 + 15 * np.sin(t)], axis=1))
    i, j = [int(np.argmin(np.abs(t - a))) for a in (np.arctan2(9, 12), np.arctan2(-9, -12) + 2 * np.pi)]
    ring[i], ring[j] = (32, 27), (8, 9)
    left = ring[i:j + 1]
    right = np.concatenate([ring[j:], ring[:i + 1]])
    out = dict(whole=ring, left=left, right=right)
    for k in ("whole", "left", "right"):
        q = out[k].astype(F64) * 256.0
        assert (q == np.round(q)).all()
        out[k + "_q"] = q.astype(np.int64)
    return out


def rings_as_case(rings, size, planes=None):
    """rings: list of [n, 2] arrays, ring g on plane g (or planes[g]) of one frame -> the arguments of polygons()"""
    G, V = len(rings), max(len(r) for r in rings)
    vertices = np.full((1, G, V, 2), np.nan, F32)
    counts = np.zeros((1, G), I32)
    for g, r in enumerate(rings):
        vertices[0, g, :len(r)] = r
        counts[0, g] = len(r)
    plane = np.arange(G, dtype=I32)[None] if planes is None else np.asarray(planes, I32)[None]
    return dict(vertices=vertices, counts=counts, poly_plane=plane, poly_clear=np.zeros((1, G), I32),
                planes=int(plane.max()) + 1, size=size)
