"""From the maps of a scene to detections, and from detections to a score (csrc/detect.hip).

    scene = SceneInference(model.eval(), head=3, tile=512)
    dets = scene.detect(frames, PeakDetector(threshold=0.5, radius=2))      # Detections, on the device
    result = evaluate(dets, labels, label_class, tolerance=3.0)             # DetectionScore, on the device
    print(float(result.f1), float(result.average_precision), dets.tolist(0, 0)[:5])

``Heatmap.transfer_points`` is the reference's validation helper: a fixed number of points per map, blobs judged
against the map's largest one.  A scene holds an unknown number of tiny objects, so ``PeakDetector`` applies a local
rule instead -- a pixel is a detection when it reaches the threshold and nothing in its (2 radius + 1)^2 window beats it
-- in one streaming pass with no host read-back, and ``evaluate`` matches lists of any length to labelled points at a
distance tolerance: true / false positives, precision, recall, F1, mean distance and average precision.

Coordinates are (x, y) with pixel centres at integers, the labels' convention everywhere in the package.  The reference
has no counterpart of either step.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from . import ops

__all__ = ["PeakDetector", "Detections", "DetectionScore", "evaluate", "score_matches", "classes_from_pattern"]


@dataclass
class Detections:
    """xy [S, C, cap, 2] float32 (x, y), score [S, C, cap] float32, count [S, C] int32, all on the device.  Every
    (frame, class) list is sorted by score, brightest first, ties in raster order; slots k >= min(count, cap) are
    xy = -1, score = -inf.  count is the number of peaks in the map and may exceed cap: then the list holds the first cap
    peaks in raster order (not the cap brightest), and ``truncated()`` says so."""
    xy: torch.Tensor
    score: torch.Tensor
    count: torch.Tensor

    @property
    def cap(self) -> int:
        return int(self.score.shape[-1])

    def truncated(self) -> torch.Tensor:
        """[S, C] bool on the device: the map had more peaks than the list holds"""
        return self.count > self.cap

    def tolist(self, s: int, c: int) -> List[Tuple[float, float, float]]:
        """[(x, y, score), ...] of frame s, class c, brightest first (reads back: for people, not for loops)"""
        n = min(int(self.count[s, c]), self.cap)
        xy, score = self.xy[s, c, :n].cpu().tolist(), self.score[s, c, :n].cpu().tolist()
        return [(p[0], p[1], v) for p, v in zip(xy, score)]


class PeakDetector:
    """detector(maps) -> Detections for maps [S, C, H, W] float32 on the GPU.  threshold: least value of a detection;
    radius (1..8): a detection is the maximum of its (2 radius + 1)^2 window, clipped to the map, the first pixel in
    raster order among equals -- so a plateau is one detection and equal maxima more than `radius` apart are two;
    refine: add the per-axis three-point parabola offset (at most half a pixel); max_points: the capacity of a list."""

    def __init__(self, threshold: float = 0.5, radius: int = 2, refine: bool = True, max_points: int = 4096):
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold must not be NaN")
        if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= 8:
            raise ValueError("radius must be an int in 1..8, got %r" % (radius,))
        if isinstance(max_points, bool) or not isinstance(max_points, int) or max_points < 1:
            raise ValueError("max_points must be a positive int, got %r" % (max_points,))
        self.threshold, self.radius, self.refine, self.max_points = threshold, radius, bool(refine), max_points

    def __call__(self, maps: torch.Tensor) -> Detections:
        if not isinstance(maps, torch.Tensor) or maps.dim() != 4:
            raise ValueError("maps must be a [S, C, H, W] tensor")
        ops._need(maps, "maps")
        s, c, h, w = (int(v) for v in maps.shape)
        xy, score, count = ops.peaks_detect(maps.view(s * c, h, w), self.threshold, self.radius, self.max_points,
                                            self.refine)
        # brightest first; a stable sort keeps equal scores in raster order and the -inf padding at the end
        score, idx = torch.sort(score, dim=1, descending=True, stable=True)
        xy = torch.gather(xy, 1, idx.unsqueeze(-1).expand(-1, -1, 2))
        cap = self.max_points
        return Detections(xy.view(s, c, cap, 2), score.view(s, c, cap), count.view(s, c))


@dataclass
class DetectionScore:
    """What ``evaluate`` returns; every tensor is on the device of the detections.  tp / fp / fn [S, C] int64 per (frame,
    class), *_total 0-d; precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn) of the totals
    (0-d float64) and per class over all frames (class_* [C]), 0 / 0 = 0; mean_distance: float64 mean of the Euclidean
    distance of the matched pairs, NaN when nothing matched; average_precision (0-d) and class_average_precision [C]: the
    all-points area under the precision envelope, predictions of all frames pooled (0 without labels); pred_label
    [S, C, cap] / label_pred [S, L] int32: the matcher's indices (-1: unmatched); served [S, C, cap] bool: the detections
    that took part (inside the list's count, at or above the score threshold, outside every ignore region) -- ``evaluate``
    always fills it, a hand-built score may leave it None."""
    tp: torch.Tensor
    fp: torch.Tensor
    fn: torch.Tensor
    tp_total: torch.Tensor
    fp_total: torch.Tensor
    fn_total: torch.Tensor
    precision: torch.Tensor
    recall: torch.Tensor
    f1: torch.Tensor
    class_precision: torch.Tensor
    class_recall: torch.Tensor
    class_f1: torch.Tensor
    mean_distance: torch.Tensor
    average_precision: torch.Tensor
    class_average_precision: torch.Tensor
    pred_label: torch.Tensor
    label_pred: torch.Tensor
    served: Optional[torch.Tensor] = None


def _ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den in float64 with 0 / 0 = 0 (den >= num >= 0 are counts)"""
    ok = den > 0
    return torch.where(ok, num.double() / torch.where(ok, den, torch.ones_like(den)).double(),
                       torch.zeros_like(den, dtype=torch.float64))


def _average_precision(score: torch.Tensor, served: torch.Tensor, hit: torch.Tensor, n_labels: torch.Tensor):
    """score / served / hit [P] in tie order, n_labels 0-d: predictions by descending score (stable), precision after
    each, its envelope from the right, summed over the hits and divided by the number of labels."""
    key = torch.where(served, score, torch.full_like(score, float("-inf")))
    idx = torch.sort(key, descending=True, stable=True).indices
    tps = (served & hit)[idx].long()
    fps = (served & ~hit)[idx].long()
    ctp, cfp = tps.cumsum(0), fps.cumsum(0)
    prec = _ratio(ctp, ctp + cfp)
    env = torch.cummax(prec.flip(0), 0).values.flip(0)
    return _ratio_f(torch.where(tps > 0, env, torch.zeros_like(env)).sum(), n_labels)


def _ratio_f(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    ok = den > 0
    return torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)).double(), torch.zeros_like(num))


def score_matches(xy, score, served, pred_label, label_pred, stats, labels, label_class) -> DetectionScore:
    """The arithmetic of ``evaluate`` after the matcher, torch ops on small arrays (any device): xy [S, C, cap, 2],
    score [S, C, cap], served [S, C, cap] bool (the prediction took part), pred_label [S, C, cap], label_pred [S, L],
    stats [S, C, 3] (tp, fp, fn), labels [S, L, 2], label_class [S, L] (-1: padding).  Average precision: predictions
    pooled over the frames in (frame, slot) order per class -- (frame, class, slot) for the overall figure -- and
    ordered by descending score with a stable sort; a prediction is a hit when the matcher gave it a label."""
    S, C, cap = (int(v) for v in score.shape)
    st = stats.long()
    tp, fp, fn = st[..., 0], st[..., 1], st[..., 2]
    tpt, fpt, fnt = tp.sum(), fp.sum(), fn.sum()
    tpc, fpc, fnc = tp.sum(0), fp.sum(0), fn.sum(0)
    matched = label_pred >= 0
    frame = torch.arange(S, device=score.device).view(S, 1).expand_as(label_pred)
    p = xy[frame, label_class.clamp(min=0, max=C - 1).long(), label_pred.clamp(min=0).long()]   # [S, L, 2]
    diff = (p - labels).double()
    dist = torch.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1])
    mean_distance = torch.where(matched, dist, torch.zeros_like(dist)).sum() / matched.sum().double()   # 0 / 0 = NaN
    hit = pred_label >= 0
    class_ap = torch.stack([_average_precision(score[:, c].reshape(-1), served[:, c].reshape(-1), hit[:, c].reshape(-1),
                                               tpc[c] + fnc[c]) for c in range(C)])
    ap = _average_precision(score.reshape(-1), served.reshape(-1), hit.reshape(-1), tpt + fnt)
    return DetectionScore(tp, fp, fn, tpt, fpt, fnt, _ratio(tpt, tpt + fpt), _ratio(tpt, tpt + fnt),
                          _ratio(2 * tpt, 2 * tpt + fpt + fnt), _ratio(tpc, tpc + fpc), _ratio(tpc, tpc + fnc),
                          _ratio(2 * tpc, 2 * tpc + fpc + fnc), mean_distance, ap, class_ap, pred_label, label_pred, served)


def evaluate(dets: Detections, labels, label_class, tolerance: float,
             score_threshold: Optional[float] = None, ignore=None) -> DetectionScore:
    """Score detections against labelled points.  labels [S, L, 2] (x, y); label_class [S, L] or [L]: the class (map
    index) of every label, -1 for padding; a label at (-1, -1) is padding whatever its class.  Per (frame, class) the
    detections are served brightest first and each takes the nearest label of its class within `tolerance` (Euclidean,
    inclusive) that no brighter detection took, ties to the lowest label index (unetpp_detect_match).
    score_threshold: detections below it are dropped before matching.  ignore: an ``IgnoreRegions`` over the same frames
    -- a detection inside a rectangle of its frame and class (or of every class) is dropped before matching, neither a
    true nor a false positive; a label inside one becomes padding, neither matched nor a false negative.  An
    ``IgnoreMask`` or an ``IgnoreUnion`` serves as well: only ``len``, ``to`` and ``contains`` are used, and a mask's
    ``contains`` looks up the nearest pixel's bit (ignore.py).  Nothing is read back."""
    xy, score, count = dets.xy, dets.score, dets.count
    dev = xy.device
    S, C, cap = (int(v) for v in score.shape)
    labels = torch.as_tensor(labels, dtype=torch.float32).to(dev)
    if labels.dim() != 3 or labels.shape[0] != S or labels.shape[2] != 2:
        raise ValueError("labels must be [%d, L, 2]" % S)
    L = int(labels.shape[1])
    cls = torch.as_tensor(label_class).to(device=dev, dtype=torch.int32)
    if cls.dim() == 1:
        cls = cls.view(1, -1).expand(S, -1)
    if tuple(cls.shape) != (S, L):
        raise ValueError("label_class must be [%d, %d] or [%d]" % (S, L, L))
    if L == 0:   # a scene without labels: one padding label
        labels = torch.full((S, 1, 2), -1.0, dtype=torch.float32, device=dev)
        cls = torch.full((S, 1), -1, dtype=torch.int32, device=dev)
    padding = (labels[..., 0] == -1) & (labels[..., 1] == -1)
    cls = torch.where(padding, torch.full_like(cls, -1), cls).contiguous()
    if ignore is not None:
        if len(ignore) != S:
            raise ValueError("ignore holds %d frames, the detections %d" % (len(ignore), S))
        ignore = ignore.to(dev)
        frame = torch.arange(S, device=dev)
        dropped = ignore.contains(frame.view(S, 1), cls, labels)
        cls = torch.where(dropped, torch.full_like(cls, -1), cls).contiguous()
    labels = labels.contiguous()
    served = torch.arange(cap, device=dev).view(1, 1, cap) < count.clamp(max=cap).unsqueeze(-1)
    if score_threshold is not None:
        served = served & (score >= float(score_threshold))
    if ignore is not None:
        served = served & ~ignore.contains(frame.view(S, 1, 1), torch.arange(C, device=dev).view(1, C, 1), xy)
    key = torch.where(served, score, torch.full_like(score, float("-inf")))
    order = torch.sort(key, dim=-1, descending=True, stable=True).indices.to(torch.int32)
    n_pred = served.sum(-1).to(torch.int32)
    pred_label, label_pred, stats = ops.detect_match(xy.contiguous(), n_pred, order, labels, cls, tolerance)
    return score_matches(xy, score, served, pred_label, label_pred, stats, labels, cls)


def classes_from_pattern(pattern, n_labels: int) -> torch.Tensor:
    """The label_class row (int32 [n_labels], CPU) of reference-style labels [N, n_labels, 2] under a ``Heatmap``
    pattern: label i has class c when pattern[c] lists i, and -1 when no map does."""
    row = [-1] * int(n_labels)
    for c, hmap in enumerate(pattern):
        for i in hmap:
            i = int(i)
            if not 0 <= i < n_labels:
                raise ValueError("pattern indexes labels 0..%d, got %d" % (n_labels - 1, i))
            if row[i] != -1:
                raise ValueError("label %d appears twice in the pattern" % i)
            row[i] = c
    return torch.tensor(row, dtype=torch.int32)
