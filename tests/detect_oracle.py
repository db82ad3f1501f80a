"""The detection pass and the detection matcher (csrc/detect.hip) restated as plain numpy loops: float64 exactly where
the kernels use it, in the same operation order, so the GPU results are held against these bit for bit.  Also the
all-points average precision of ``detect.score_matches`` as a loop.  Shared by tests/test_detect_host.py and
tests/test_gpu_detect.py (test infrastructure; no GPU here).

Conventions: coordinates are (x, y), a pixel centre is an integer; raster order is row by row, x fastest."""
import numpy as np

F32, F64 = np.float32, np.float64


def is_peak(a, y, x, r):
    """a [H, W] float32: does no pixel of the (2r+1)^2 window around (y, x), clipped to the map, beat it?  q beats p
    when v_q > v_p, or v_q == v_p and q is earlier in raster order (plain comparisons: NaN never wins)."""
    H, W = a.shape
    v = a[y, x]
    for yy in range(max(y - r, 0), min(y + r, H - 1) + 1):
        for xx in range(max(x - r, 0), min(x + r, W - 1) + 1):
            q = a[yy, xx]
            earlier = yy < y or (yy == y and xx < x)
            if q > v or (q == v and earlier):
                return False
    return True


def parabola_offset(fa, fb, fc):
    """three float32 values at -1, 0, +1 -> the vertex offset in float64: den = (a - 2 b) + c; den < 0:
    (0.5 (a - c)) / den limited to [-0.5, 0.5] by comparisons; otherwise (den >= 0 or NaN) 0"""
    with np.errstate(all="ignore"):
        a, b, c = F64(fa), F64(fb), F64(fc)
        den = (a - (F64(2.0) * b)) + c
        off = F64(0.0)
        if den < 0.0:
            off = (F64(0.5) * (a - c)) / den
            if off < -0.5:
                off = F64(-0.5)
            if off > 0.5:
                off = F64(0.5)
    return off


def refine_peak(a, y, x, refine=True, origin=(0, 0)):
    """(x, y) of the peak at pixel (y, x) as float32: integer + offset per axis (0 at the map's edge), rounded once.
    origin = (x0, y0): `a` is the bottom-right crop of a larger map that starts there (the integer part is x + x0)"""
    H, W = a.shape
    ox = oy = F64(0.0)
    if refine:
        if 0 < x < W - 1:
            ox = parabola_offset(a[y, x - 1], a[y, x], a[y, x + 1])
        if 0 < y < H - 1:
            oy = parabola_offset(a[y - 1, x], a[y, x], a[y + 1, x])
    return F32(F64(x + origin[0]) + ox), F32(F64(y + origin[1]) + oy)


def peaks_of_map(a, threshold, radius, refine=True, candidates=None, origin=(0, 0)):
    """a [H, W] float32 -> [(x, y, score), ...] of all peaks in raster order.  candidates: (y, x) pairs to test instead
    of every pixel (a test that knows where the map is non-zero); they are visited in raster order."""
    a = np.asarray(a, dtype=F32)
    thr = F32(threshold)
    if candidates is None:
        with np.errstate(invalid="ignore"):
            candidates = np.argwhere(a >= thr)          # row-major: raster order
    else:
        candidates = sorted((int(y), int(x)) for y, x in candidates)
    out = []
    for y, x in candidates:
        y, x = int(y), int(x)
        v = a[y, x]
        if not v >= thr:
            continue
        if is_peak(a, y, x, radius):
            px, py = refine_peak(a, y, x, refine, origin)
            out.append((px, py, v))
    return out


def pack_peaks(lists, cap):
    """per-map peak lists -> (xy [M, cap, 2], score [M, cap], count [M]) as unetpp_peaks_detect lays them out"""
    M = len(lists)
    xy = np.full((M, cap, 2), -1.0, dtype=F32)
    score = np.full((M, cap), -np.inf, dtype=F32)
    count = np.zeros(M, dtype=np.int32)
    for m, peaks in enumerate(lists):
        count[m] = len(peaks)
        for k, (px, py, v) in enumerate(peaks[:cap]):
            xy[m, k, 0], xy[m, k, 1], score[m, k] = px, py, v
    return xy, score, count


def peaks_detect(maps, threshold, radius, cap, refine=True):
    """maps [M, H, W] -> (xy, score, count): the whole of unetpp_peaks_detect"""
    return pack_peaks([peaks_of_map(a, threshold, radius, refine) for a in np.asarray(maps, dtype=F32)], cap)


def detect_match(xy, n_pred, order, labels, label_class, tolerance):
    """xy [S, C, cap, 2], n_pred [S, C], order [S, C, cap], labels [S, L, 2], label_class [S, L], tolerance ->
    (pred_label [S, C, cap], label_pred [S, L], stats [S, C, 3]): the whole of unetpp_detect_match"""
    xy, labels = np.asarray(xy, dtype=F32), np.asarray(labels, dtype=F32)
    S, C, cap = xy.shape[:3]
    L = labels.shape[1]
    tol = F64(F32(tolerance))
    tol2 = tol * tol
    pred_label = np.full((S, C, cap), -1, dtype=np.int32)
    label_pred = np.full((S, L), -1, dtype=np.int32)
    stats = np.zeros((S, C, 3), dtype=np.int32)
    for s in range(S):
        for c in range(C):
            mine = [l for l in range(L) if int(label_class[s, l]) == c]
            tp = served = 0
            for kk in range(min(max(int(n_pred[s, c]), 0), cap)):
                p = int(order[s, c, kk])
                if p < 0 or p >= cap:
                    continue
                served += 1
                best, bl = None, -1
                for l in mine:
                    if label_pred[s, l] >= 0:
                        continue
                    with np.errstate(all="ignore"):
                        dx = F32(xy[s, c, p, 0] - labels[s, l, 0])
                        dy = F32(xy[s, c, p, 1] - labels[s, l, 1])
                        d = F64(dx) * F64(dx) + F64(dy) * F64(dy)
                    if d <= tol2 and (bl < 0 or d < best):
                        best, bl = d, l
                if bl >= 0:
                    tp += 1
                    label_pred[s, bl] = p
                    pred_label[s, c, p] = bl
            stats[s, c] = (tp, served - tp, len(mine) - tp)
    return pred_label, label_pred, stats


def average_precision(score, served, hit, n_labels):
    """score / served / hit [P] in tie order: the served predictions by descending score (equal scores in the order
    given), precision after each, its envelope from the right; the sum over the hits / n_labels (0 without labels)"""
    idx = [i for i in range(len(score)) if served[i]]
    idx.sort(key=lambda i: -float(score[i]))            # Python's sort is stable
    tp = fp = 0
    prec, hits = [], []
    for i in idx:
        if hit[i]:
            tp += 1
        else:
            fp += 1
        prec.append(tp / float(tp + fp))
        hits.append(bool(hit[i]))
    best, total = 0.0, 0.0
    for i in range(len(prec) - 1, -1, -1):
        best = max(best, prec[i])
        if hits[i]:
            total += best
    return total / n_labels if n_labels > 0 else 0.0


def blob(H, W, cx, cy, radius=3.0):
    """the project's target shape (csrc/keypoints.hip, unetpp_heatmap_pattern): exp(-0.5 * dist / radius), dist the
    Euclidean distance to (cx, cy), evaluated in float64 and rounded to float32"""
    yy, xx = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    dx, dy = xx - F64(cx), yy - F64(cy)
    return np.exp(-0.5 * np.sqrt(dx * dx + dy * dy) / F64(radius)).astype(F32)
