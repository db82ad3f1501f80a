"""Copy-paste of tiny objects (crops.py: ObjectPaste, csrc/paste.hip) restated in numpy: the source-table rule, the blend
weights, the draw bit for bit including the hash, the pixels in float32 with the kernel's order of operations, the
merge into the target, the union target by brute force over frame labels plus pasted labels, and the input sets the
tests use.  Shared by tests/test_paste_host.py and tests/test_gpu_paste.py (test infrastructure; no GPU here).

The restatement is a class, ``Paste``: every rule a planted mutation bends is a method of its own, so a mutation is a
subclass that overrides one of them (tests/test_paste_host.py) and everything else stays the restatement.

Conventions: coordinates are (x, y) pixel indices, a pixel centre is an integer; a row is 16 numbers as in
tests/loader_oracle.py; a code 0..7 is q = code & 3 quarter turns, then a flip in x when code & 4."""
import math

import numpy as np

from oracle.dropout_oracle import GOLDEN, mix64
from tests import crops_oracle as co
from tests import ignore_oracle as io

F32, F64 = np.float32, np.float64
SLOTS = 64                    # UNETPP_PASTE_MAX_SLOTS: the stride of a window in the uniforms' counter
_QC, _QS = (1, 0, -1, 0), (0, 1, 0, -1)


# ---------------------------------------------------------------------------------------------------------------
# the host's tables
def source_table_ref(labels, label_class, C, src_size, R, rects=None, rect_class=None):
    """labels [S, L, 2] float32, label_class [S, L] -> (frame [T] int32, xy [T, 2] float32, cls [T] int32), label by
    label: valid, the patch about c = floor(xy + 0.5) inside the frame, no other valid label of the frame within Chebyshev
    distance R + 1 of c, c in no live ignore rectangle (class -1 or in [0, C)) of the frame."""
    labels, label_class = np.asarray(labels, dtype=F32), np.asarray(label_class)
    Hs, Ws = src_size
    frame, xy, cls = [], [], []
    for s in range(labels.shape[0]):
        ok = co.valid_labels(labels[s], label_class[s], C)
        pos = labels[s].astype(F64)
        for l in np.flatnonzero(ok):
            cx, cy = math.floor(pos[l, 0] + 0.5), math.floor(pos[l, 1] + 0.5)
            if not (R <= cx <= Ws - 1 - R and R <= cy <= Hs - 1 - R):
                continue
            others = ok.copy()
            others[l] = False
            cheb = np.maximum(np.abs(pos[others, 0] - cx), np.abs(pos[others, 1] - cy))
            if (cheb <= R + 1).any():
                continue
            if rects is not None and any(-1 <= k < C and r[0] <= cx <= r[2] and r[1] <= cy <= r[3]
                                         for r, k in zip(np.asarray(rects[s], dtype=F64), np.asarray(rect_class[s]))):
                continue
            frame.append(s), xy.append(labels[s, l]), cls.append(label_class[s, l])
    return (np.asarray(frame, dtype=np.int32), np.asarray(xy, dtype=F32).reshape(-1, 2), np.asarray(cls, dtype=np.int32))


def alpha_ref(R, core):
    """float32 [2R+1, 2R+1]: clamp((R + 0.5 - d) / (R + 0.5 - core), 0, 1) in float64, rounded once"""
    i = np.arange(-R, R + 1, dtype=F64)
    d = np.sqrt(i[None, :] ** 2 + i[:, None] ** 2)
    return np.clip((R + 0.5 - d) / (R + 0.5 - F64(core)), 0.0, 1.0).astype(F32)


def uniform(seed, n, k, j):
    """u_j of slot k of window n: (mix64(seed + GOLDEN ((64 n + k) 8 + j + 1)) >> 40) * 2^-24, a 24-bit value"""
    with np.errstate(over="ignore"):
        ctr = (np.uint64(n) * np.uint64(SLOTS) + np.uint64(k)) * np.uint64(8) + np.uint64(j + 1)
        bits = mix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + GOLDEN * ctr)
    return float(bits >> np.uint64(40)) * 2.0 ** -24


def _pick(u, count):
    return int(min(math.floor(u * count), count - 1))


def source_row(src_frame, src_xy, src_class, t, M, C, src_size, R):
    """-> (ok, cx, cy): whether row t can be pasted, and its rounded centre"""
    Hs, Ws = src_size
    x, y = F64(src_xy[t][0]), F64(src_xy[t][1])
    if not (0 <= int(src_frame[t]) < M and 0 <= int(src_class[t]) < C and np.isfinite(x) and np.isfinite(y)):
        return False, 0, 0
    cx, cy = math.floor(x + 0.5), math.floor(y + 0.5)
    return bool(R <= cx <= Ws - 1 - R and R <= cy <= Hs - 1 - R), int(cx), int(cy)


class Paste:
    """The restatement.  The methods up to `stores` are the rules the planted mutations bend."""

    # -- rules ---------------------------------------------------------------------------------------------------
    def pixel_offset(self, code, i, j):
        """the source offset destination offset (i, j) reads: T_code^-1 (i, j) = Q^-q D (i, j)"""
        qc, qs, dx = _QC[code & 3], _QS[code & 3], (-1 if code & 4 else 1)
        fi = dx * i
        return qc * fi + qs * j, qc * j - qs * fi

    def label_offset(self, code, ox, oy):
        """T_code (ox, oy) = D Q^q (ox, oy), the way the pixels go"""
        qc, qs, dx = _QC[code & 3], _QS[code & 3], (-1 if code & 4 else 1)
        return dx * (qc * ox - qs * oy), qs * ox + qc * oy

    def gain_bias(self, rows, n):
        return F32(rows[n][12]), F32(rows[n][13])

    def channel(self, mul, add, c):
        return F32(mul[c]), F32(add[c])

    def too_close(self, d2, clearance2):
        return d2 < clearance2

    def overlaps(self, cheb, R):
        return cheb <= 2 * R

    def keeps(self, t):
        """a target value the merge never overwrites"""
        return t < 0

    def stores(self, v, t):
        return v > t

    # -- the draw ------------------------------------------------------------------------------------------------
    def draw(self, N, K, seed, src_frame, src_xy, src_class, labels, label_class, index, rows, C, src_size, out_size, p, R,
             clearance, dihedral=True):
        """unetpp_paste_draw -> dict(src [N, K] i32, dst [N, K, 2] i32, code [N, K] i32, xy [N, K, 2] f32, cls [N, K] i32)"""
        labels, label_class = np.asarray(labels, dtype=F32), np.asarray(label_class)
        rows = np.asarray(rows, dtype=F32)
        src_xy = np.asarray(src_xy, dtype=F32).reshape(-1, 2)
        M, T = labels.shape[0], len(src_frame)
        Ho, Wo = out_size
        cl2 = F64(F32(clearance)) * F64(F32(clearance))
        src = np.full((N, K), -1, dtype=np.int32)
        dst = np.zeros((N, K, 2), dtype=np.int32)
        code = np.zeros((N, K), dtype=np.int32)
        xy = np.full((N, K, 2), -1.0, dtype=F32)
        cls = np.full((N, K), -1, dtype=np.int32)
        for n in range(N):
            idx = int(index[n])
            live = 0 <= idx < M
            if live:
                ok_l = (label_class[idx] >= 0) & ~(labels[idx, :, 0] < 0) & ~(labels[idx, :, 1] < 0)
                xo, yo = co.window_positions(labels[idx], rows[n])
                xo, yo = xo[ok_l].astype(F64), yo[ok_l].astype(F64)
            accepted = []
            for k in range(K):
                u = [uniform(seed, n, k, j) for j in range(5)]
                t = _pick(u[1], T)
                cd = int(math.floor(8.0 * u[2])) if dihedral else 0
                px, py = R + _pick(u[3], Wo - 2 * R), R + _pick(u[4], Ho - 2 * R)
                dst[n, k], code[n, k] = (px, py), cd
                if not (F32(u[0]) < F32(p) and live):
                    continue
                ok, cx, cy = source_row(src_frame, src_xy, src_class, t, M, C, src_size, R)
                if not ok:
                    continue
                with np.errstate(invalid="ignore"):
                    dx, dy = xo - F64(px), yo - F64(py)
                    if self.too_close(dx * dx + dy * dy, cl2).any():
                        continue
                if any(self.overlaps(max(abs(px - ax), abs(py - ay)), R) for ax, ay in accepted):
                    continue
                accepted.append((px, py))
                sx, sy = F64(src_xy[t, 0]), F64(src_xy[t, 1])
                tx, ty = self.label_offset(cd, sx - math.floor(sx + 0.5), sy - math.floor(sy + 0.5))
                src[n, k], cls[n, k] = t, src_class[t]
                xy[n, k] = (F32(F64(px) + tx), F32(F64(py) + ty))
        return dict(src=src, dst=dst, code=code, xy=xy, cls=cls)

    # -- the pixels ----------------------------------------------------------------------------------------------
    def apply(self, inputs, src, dst, code, src_frame, src_xy, src_class, store_nchw, rows, mul, add, alpha, C):
        """unetpp_paste_apply on a copy of inputs [N, Cin, Ho, Wo] float32; store_nchw [M, Cin, Hs, Ws] of either type.
        Rows of any content: one that names no patch inside its frame and window is skipped."""
        out = np.array(inputs, dtype=F32)
        store = np.asarray(store_nchw)
        alpha = np.asarray(alpha, dtype=F32)
        rows = np.asarray(rows, dtype=F32)
        N, Cin, Ho, Wo = out.shape
        M, _, Hs, Ws = store.shape
        R = alpha.shape[0] // 2
        T = len(src_frame)
        for n in range(N):
            for k in range(src.shape[1]):
                t, (px, py), cd = int(src[n, k]), (int(v) for v in dst[n, k]), int(code[n, k])
                if not (0 <= t < T and 0 <= cd <= 7 and R <= px <= Wo - 1 - R and R <= py <= Ho - 1 - R):
                    continue
                ok, cx, cy = source_row(src_frame, src_xy, src_class, t, M, C, (Hs, Ws), R)
                if not ok:
                    continue
                gain, bias = self.gain_bias(rows, n)
                f = int(src_frame[t])
                for c in range(Cin):
                    mc, ac = self.channel(mul, add, c)
                    for j in range(-R, R + 1):
                        for i in range(-R, R + 1):
                            si, sj = self.pixel_offset(cd, i, j)
                            v = F32(store[f, c, cy + sj, cx + si])
                            pv = gain * (v * mc + ac) + bias
                            a, d = alpha[j + R, i + R], out[n, c, py + j, px + i]
                            out[n, c, py + j, px + i] = pv if a == 1 else d if a == 0 else d + a * (pv - d)
        return out

    # -- the targets ---------------------------------------------------------------------------------------------
    def pasted_minima(self, xy, cls, n, c, out_size):
        """least squared distance over the live pasted labels of class c of window n -> float64 [Ho, Wo] or None"""
        live = np.asarray(cls[n]) == c
        if not live.any():
            return None
        return co.brute_minima(np.asarray(xy, dtype=F32)[n, live, 0], np.asarray(xy, dtype=F32)[n, live, 1], *out_size)

    def merge(self, target, xy, cls, radius):
        """unetpp_paste_target on a copy of target [N, C, Ho, Wo] float32 -> (the target, bool mask of the elements the
        rule stores)"""
        out = np.array(target, dtype=F32)
        wrote = np.zeros(out.shape, dtype=bool)
        N, C, Ho, Wo = out.shape
        for n in range(N):
            for c in range(C):
                m = self.pasted_minima(xy, cls, n, c, (Ho, Wo))
                if m is None:
                    continue
                v = co.value_of(m, radius)
                with np.errstate(invalid="ignore"):
                    put = self.stores(v, out[n, c]) & ~self.keeps(out[n, c])
                out[n, c][put] = v[put]
                wrote[n, c] = put
        return out, wrote


def paste_draw_ref(*args, **kwargs):
    """unetpp_paste_draw by the unmutated restatement: Paste().draw"""
    return Paste().draw(*args, **kwargs)


def paste_apply_ref(*args, **kwargs):
    """unetpp_paste_apply by the unmutated restatement: Paste().apply"""
    return Paste().apply(*args, **kwargs)


def union_target_ref(labels, label_class, index, rows, C, out_size, radius, xy, cls):
    """The target by brute force over the frame's valid labels PLUS the live pasted labels of the window: what
    crops_oracle.points_target_ref gives with the pasted labels in the list -> (float32 [N, C, Ho, Wo], frame-only minima
    float64 [N, C, Ho, Wo], pasted-only minima likewise; inf where there is none)"""
    labels, label_class = np.asarray(labels, dtype=F32), np.asarray(label_class)
    rows = np.asarray(rows, dtype=F32)
    M = labels.shape[0]
    Ho, Wo = out_size
    N = len(index)
    out = np.zeros((N, C, Ho, Wo), dtype=F32)
    m_frame = np.full((N, C, Ho, Wo), np.inf)
    m_paste = np.full((N, C, Ho, Wo), np.inf)
    rule = Paste()
    for n in range(N):
        idx = int(index[n])
        if 0 <= idx < M:
            ok = co.valid_labels(labels[idx], label_class[idx], C)
            xo, yo = co.window_positions(labels[idx], rows[n])
            for c in range(C):
                pick = ok & (label_class[idx] == c)
                if pick.any():
                    m_frame[n, c] = co.brute_minima(xo[pick], yo[pick], Ho, Wo)
        for c in range(C):
            m = rule.pasted_minima(xy, cls, n, c, out_size)
            if m is not None:
                m_paste[n, c] = m
    both = np.minimum(m_frame, m_paste)
    some = np.isfinite(both)
    out[some] = co.value_of(both[some], radius)
    return out, m_frame, m_paste


# ---------------------------------------------------------------------------------------------------------------
# input sets
HS, WS = 96, 128              # the two frames
X0, Y0 = 30, 20               # where the windows sit in their frame under the identity row
RADIUS = 3.0
# name: N, Ho, Wo, Cin, uint8 store, R, K, L, n_classes, seed -- the seeds were chosen on the CPU with Paste().draw so that
# what each case is there for happens (tests/test_paste_host.py asserts it)
CASES = {
    "3x40x48-c1-u8-r4-k4-l7": (3, 40, 48, 1, True, 4, 4, 7, 2, 12),
    "2x33x70-c3-f32-r4-k4-l300": (2, 33, 70, 3, False, 4, 4, 300, 5, 1),
    "3x40x48-c3-u8-r1-k9-l1": (3, 40, 48, 3, True, 1, 9, 1, 5, 6),
    "2x33x70-c1-f32-r1-k1-l7": (2, 33, 70, 1, False, 1, 1, 7, 2, 8),
    "3x40x48-c3-f32-r4-k9-l300": (3, 40, 48, 3, False, 4, 9, 300, 2, 4),
}
KINDS_OF = {3: ("identity", "flip", "three_quarters"), 2: ("identity", "general")}   # 33 x 70 has no whole quarter turn


def case(name, p=1.0, plant=True):
    """One input set -> dict.  Two frames of HS x WS, random pixels (so every patch is asymmetric); sample n reads frame
    n % 2 under KINDS_OF[N][n] with its own gain and bias, except that with N = 3 sample 1 has index -1.  A source table
    of eight rows off the pixel grid that can be pasted and four that cannot (a frame out of range, a patch off the
    frame, a class >= C, a NaN).  L labels per frame, scattered up to 400 px around the window and never within the
    clearance + 2 of a window pixel -- except, with plant, the last label of frame 0: it is put at exactly the clearance
    from the first slot window 0 accepts without it, on the far side in x (its squared distance IS clearance^2)."""
    N, Ho, Wo, Cin, u8, R, K, L, C, seed = CASES[name]
    rng = np.random.default_rng(100 * seed + Ho)
    M = 2
    if u8:
        store = rng.integers(0, 256, (M, Cin, HS, WS), dtype=np.uint8)
    else:
        store = rng.uniform(-1.0, 1.0, (M, Cin, HS, WS)).astype(F32)
    mul = rng.uniform(0.5, 1.5, Cin).astype(F32) * (F32(1.0 / 255.0) if u8 else F32(1.0))
    add = rng.uniform(-0.2, 0.2, Cin).astype(F32)
    kinds = KINDS_OF[N]
    rows = np.stack([io.window_row(k, (X0, Y0), (Ho, Wo)) for k in kinds])
    rows[:, 12], rows[:, 13] = rng.uniform(0.5, 1.5, N), rng.uniform(-0.2, 0.2, N)
    rows = rows.astype(F32)
    index = np.arange(N, dtype=np.int64) % M
    if N == 3:
        index[1] = -1
    clearance = 2.0 * R
    # the source table
    src_frame = np.array([0, 1, 0, 1, 0, 1, 0, 1, M, 0, 1, 0], dtype=np.int32)
    src_xy = np.stack([rng.uniform(R + 1, WS - 2 - R, 12), rng.uniform(R + 1, HS - 2 - R, 12)], axis=1).astype(F32)
    src_class = rng.integers(0, C, 12).astype(np.int32)
    src_xy[9] = (R - 0.75, 40.25)                        # the patch leaves the frame on the left
    src_class[10] = C
    src_xy[11] = (np.nan, 30.0)
    # the labels: a few near the window, the rest far from it
    labels = np.zeros((M, L, 2), dtype=F32)
    classes = np.zeros((M, L), dtype=np.int32)
    for m in range(M):
        x = rng.uniform(X0 - 400, X0 + Wo + 400, L)
        y = rng.uniform(Y0 - 400, Y0 + Ho + 400, L)
        near = (x > X0 - clearance - 2) & (x < X0 + Wo + clearance + 2) & (y > Y0 - clearance - 2) & (y < Y0 + Ho + clearance + 2)
        x[near] += Wo + 2 * clearance + 4
        cls = rng.integers(0, C, L)
        if L >= 7:
            x[:3] = X0 + rng.uniform(0, Wo - 1, 3)
            y[:3] = Y0 + rng.uniform(0, Ho - 1, 3)
            x[3], y[3], cls[3] = -1.0, -1.0, 0             # a sentinel
            x[4], y[4], cls[4] = X0 + Wo / 2.0, Y0 + Ho / 2.0, -1   # a live position with class -1: not a label
            cls[2] = C + 1                                 # a class no map has: still keeps pastes away
        labels[m, :, 0], labels[m, :, 1], classes[m] = x, y, cls
    inputs = rng.uniform(-1.0, 1.0, (N, Cin, Ho, Wo)).astype(F32)
    out = dict(name=name, N=N, Ho=Ho, Wo=Wo, Cin=Cin, u8=u8, R=R, K=K, L=L, C=C, seed=seed, M=M, p=p, clearance=clearance,
               store=store, mul=mul, add=add, rows=rows, kinds=kinds, index=index, src_frame=src_frame, src_xy=src_xy,
               src_class=src_class, labels=labels, label_class=classes, inputs=inputs, alpha=alpha_ref(R, 0.6 * R),
               planted=None)
    if plant:
        first = draw_of(out)
        took = np.flatnonzero(first["src"][0] >= 0)
        if took.size:
            px, py = first["dst"][0, took[0]]
            labels[0, L - 1] = (X0 + px + clearance, Y0 + py)       # window 0 is the identity: xo = x - X0 exactly
            classes[0, L - 1] = 0
            out["planted"] = (int(px), int(py))
    return out


def draw_of(cs, rule=None):
    """the draw of an input set under a rule (default: the restatement)"""
    rule = rule or Paste()
    return rule.draw(cs["N"], cs["K"], cs["seed"], cs["src_frame"], cs["src_xy"], cs["src_class"], cs["labels"],
                     cs["label_class"], cs["index"], cs["rows"], cs["C"], (HS, WS), (cs["Ho"], cs["Wo"]), cs["p"], cs["R"],
                     cs["clearance"])


def apply_of(cs, rows_of, rule=None):
    rule = rule or Paste()
    return rule.apply(cs["inputs"], rows_of["src"], rows_of["dst"], rows_of["code"], cs["src_frame"], cs["src_xy"],
                      cs["src_class"], cs["store"], cs["rows"], cs["mul"], cs["add"], cs["alpha"], cs["C"])


def ignore_rects(cs):
    """one rectangle per frame for every class over the left part of the window's place, and the marks it makes"""
    rects = np.zeros((cs["M"], 1, 4), dtype=F32)
    rects[:, 0] = (X0 - 5, Y0 - 5, X0 + cs["Wo"] // 2, Y0 + cs["Ho"] + 5)
    rect_class = np.full((cs["M"], 1), -1, dtype=np.int32)
    mask = io.mark_mask(rects, rect_class, cs["index"], cs["rows"], cs["C"], (cs["Ho"], cs["Wo"]), (HS, WS), False)
    return rects, rect_class, mask
