"""Training on large scenes (csrc/crops.hip): windows drawn where the objects are, and their targets.

    crops = SceneCrops(frames, labels, label_class, n_classes=4, crop=(256, 256), p_object=0.75)
    for inputs, target, points, inside in crops.batches(batch_size=32, steps=1000):
        train_step(model, optimizer, criterion, inputs, target)
    dets = scene.detect(frames, PeakDetector(threshold=0.5))
    score = evaluate(dets, labels, label_class, tolerance=3.0)
    crops.add_centres(*false_positive_centres(dets, score))          # hard-negative mining, between epochs

``DeviceLoader`` takes one window per image, a crop or a pad about the centre.  A frame thousands of pixels on a side
with a few hundred three-pixel objects is almost all background, so ``SceneCrops`` draws every window of a batch on the
device: with probability ``p_object`` about a row of a centre table (the labels to begin with, whatever the caller adds
later) plus a jitter, otherwise anywhere in any frame.  The window is cut by the loader's warp under the loader's
``Augment`` (flips, quarter turns, rotation, scale, contrast, brightness; no shift -- the window's place is its origin),
and its target comes from the frame's whole label list, any number of objects per class: per class the map is
exp(-0.5 d / radius) of the distance d to the nearest label, the maximum over the labels of the package's blob, so an
object just outside the window shines into it.  Three launches per batch (draw, warp, targets), no host data work.

Partially labelled scenes: ``ignore=IgnoreRegions(...)`` and / or ``ignore_outside=True`` add a fourth launch that writes
-1 into the target wherever the pixel's source position lies in an ignore rectangle of its frame (of that class or of
every class) or outside the frame; a criterion built with ``ignore_negative=True`` leaves those elements out.

Coordinates are (x, y) with pixel centres at integers, the labels' convention everywhere in the package.  The reference
has no counterpart.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import ops
from .ignore import IgnoreRegions
from .loader import Augment, _channels, _per_channel, _source_size

__all__ = ["SceneCrops", "false_positive_centres"]


def _centre_table(frame, xy, n_frames: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(frame [V] int32, xy [V, 2] float32) on `device` from anything torch.as_tensor takes; ValueError for a frame
    outside [0, n_frames), a coordinate that is not finite or mismatched shapes.  Reads back: not for the training loop."""
    frame = torch.as_tensor(frame).reshape(-1)
    xy = torch.as_tensor(xy, dtype=torch.float32).reshape(-1, 2)
    if frame.numel() == 0:
        frame = frame.to(torch.int32)
    if frame.is_floating_point() or frame.dtype == torch.bool:
        raise ValueError("frame must hold whole numbers")
    if frame.numel() != xy.shape[0]:
        raise ValueError("one (x, y) per frame entry: got %d frames and %d points" % (frame.numel(), xy.shape[0]))
    if frame.numel() and (int(frame.min()) < 0 or int(frame.max()) >= n_frames):
        raise ValueError("a centre's frame must lie in [0, %d)" % n_frames)
    if not bool(torch.isfinite(xy).all()):
        raise ValueError("centres must be finite")
    return (frame.to(device=device, dtype=torch.int32).contiguous(), xy.to(device=device).contiguous())


class SceneCrops:
    """Windows of scenes held on the device, with their targets.  frames: uint8 [S, H, W, C] (decoded, channels last) or
    float32 [S, C, H, W]; labels [S, L, 2] as (x, y) and label_class [S, L] or [L] as ``evaluate`` takes them (class -1
    or a negative coordinate: padding); all on the GPU.  crop = (Ho, Wo); p_object: the share of windows centred on a row
    of the centre table; jitter = (jx, jy): that centre moves by up to so many whole pixels; augment: an ``Augment``
    with translate = (0, 0) (rot90 needs a square crop); radius: of the target's blobs;
    inputs = gain * (pixel * mul[c] + add[c]) + bias, `fill` (source units) outside the frame.

    batch(n) -> (inputs [n, C, Ho, Wo], target [n, n_classes, Ho, Wo], points [n, L, 2], inside [n, L] uint8): three
    launches, nothing synchronises with the host; ``last`` holds the batch's (params [n, 16], index [n], origin [n, 2]
    as (ox, oy)).  A run is reproducible from `seed`: the per-batch seeds come from a host generator.

    ignore: an ``IgnoreRegions`` over the same frames -- target = -1 where the pixel's source position lies in one of
    the frame's rectangles (class -1: every class map; class c: map c), whatever label is there; ignore_outside: also
    where it lies outside the frame (a bilinear neighbour is `fill`), and all of an all-fill sample.  Either makes
    batch(n) a fourth launch (unetpp_target_ignore) after the targets, still without a host synchronisation.

    The centre table starts as the valid labels; set_centres / add_centres replace / extend it -- a sampling policy such
    as class balancing is a matter of what the caller puts there."""

    def __init__(self, frames, labels, label_class, n_classes: int, crop=(256, 256), p_object: float = 0.75,
                 jitter=(32, 32), augment: Optional[Augment] = None, radius: float = 3.0, mul=1.0 / 255.0, add=0.0,
                 fill: float = 0.0, seed: int = 0, ignore=None, ignore_outside: bool = False):
        self.augment = Augment() if augment is None else augment
        self.crop = (int(crop[0]), int(crop[1]))
        if min(self.crop) < 1:
            raise ValueError("crop = (Ho, Wo), both positive")
        if self.augment.translate != (0.0, 0.0):
            raise ValueError("Augment.translate must be (0, 0) here: a window's place is its origin (use jitter)")
        if self.augment.rot90 and self.crop[0] != self.crop[1]:
            raise ValueError("Augment.rot90 needs a square crop, got %dx%d" % self.crop)
        self.p_object, self.radius = float(p_object), float(radius)
        self.jitter = (float(jitter[0]), float(jitter[1]))
        if not 0.0 <= self.p_object <= 1.0 or not min(self.jitter) >= 0.0 or not self.radius > 0.0:
            raise ValueError("p_object lies in [0, 1], jitter is a pair of magnitudes and radius is positive")
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= 65535:
            raise ValueError("n_classes must lie in 1..65535")
        for name, t in (("frames", frames), ("labels", labels), ("label_class", label_class)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("%s must live on the GPU: this path has no CPU fallback" % name)
        if frames.dtype not in (torch.uint8, torch.float32):
            raise TypeError("frames must be uint8 [S, H, W, C] or float32 [S, C, H, W], got %s" % frames.dtype)
        c = _channels(frames)
        self.frames = frames.contiguous()
        self.device = frames.device
        self.src_size = _source_size(frames)
        s = int(frames.shape[0])
        if labels.dim() != 3 or labels.shape[0] != s or labels.shape[2] != 2:
            raise ValueError("labels must be [%d, L, 2]" % s)
        n_labels = int(labels.shape[1])
        cls = label_class.to(device=self.device, dtype=torch.int32)
        if cls.dim() == 1:
            cls = cls.view(1, -1).expand(s, -1)
        if tuple(cls.shape) != (s, n_labels):
            raise ValueError("label_class must be [%d, %d] or [%d]" % (s, n_labels, n_labels))
        labels = labels.to(device=self.device, dtype=torch.float32)
        if n_labels == 0:   # a scene without labels: one padding label
            labels = torch.full((s, 1, 2), -1.0, dtype=torch.float32, device=self.device)
            cls = torch.full((s, 1), -1, dtype=torch.int32, device=self.device)
        self.labels, self.label_class = labels.contiguous(), cls.contiguous()
        self.mul, self.add = _per_channel(mul, c, self.device), _per_channel(add, c, self.device)
        self.fill = float(fill)
        self.seed = int(seed)
        self._seeds = torch.Generator().manual_seed(self.seed)
        self.last = None
        valid = ((self.label_class >= 0) & (self.label_class < self.n_classes)
                 & ~(self.labels[..., 0] < 0) & ~(self.labels[..., 1] < 0))
        where = valid.nonzero()
        self.centre_frame = where[:, 0].to(torch.int32).contiguous()
        self.centre_xy = self.labels[valid].contiguous()
        self.ignore_outside = bool(ignore_outside)
        self.ignore = None
        if ignore is not None:
            if not isinstance(ignore, IgnoreRegions):
                raise TypeError("ignore must be an IgnoreRegions")
            if len(ignore) != s:
                raise ValueError("ignore holds %d frames, the scenes %d" % (len(ignore), s))
            self.ignore = ignore.to(self.device)

    def __len__(self):
        return int(self.frames.shape[0])

    def set_centres(self, frame, xy) -> None:
        """Replace the centre table: frame [V] whole numbers in [0, S), xy [V, 2] as (x, y); V may be 0, every window is
        then uniform.  Reads back to check the frames: between epochs, not per step."""
        self.centre_frame, self.centre_xy = _centre_table(frame, xy, len(self), self.device)

    def add_centres(self, frame, xy, repeat: int = 1) -> None:
        """Extend the centre table by the rows (frame, xy), each `repeat` times (its weight in the draw)."""
        if isinstance(repeat, bool) or not isinstance(repeat, int) or repeat < 1:
            raise ValueError("repeat must be a positive int, got %r" % (repeat,))
        f, p = _centre_table(frame, xy, len(self), self.device)
        self.centre_frame = torch.cat([self.centre_frame, f.repeat(repeat)]).contiguous()
        self.centre_xy = torch.cat([self.centre_xy, p.repeat(repeat, 1)]).contiguous()

    def _next_seed(self) -> int:
        return int(torch.randint(0, 2 ** 62, (1,), generator=self._seeds, dtype=torch.int64))

    def batch(self, n: int):
        """n windows: (inputs [n, C, Ho, Wo], target [n, n_classes, Ho, Wo], points [n, L, 2], inside [n, L] uint8)."""
        params, index, origin = ops.crops_draw(n, self._next_seed(), len(self), self.src_size, self.crop,
                                               self.centre_frame, self.centre_xy, self.p_object, self.jitter,
                                               self.augment.desc(), self.device)
        inputs, points, inside = ops.warp_batch(self.frames, index, params, self.crop, self.mul, self.add, self.fill,
                                                self.labels)
        target = ops.points_target(self.labels, self.label_class, index, params, self.n_classes, self.crop, self.radius)
        if self.ignore is not None or self.ignore_outside:
            ign = self.ignore
            ops.target_ignore(target, ign.rects if ign is not None else None, ign.rect_class if ign is not None else None,
                              index, params, self.src_size, self.ignore_outside, n_frames=len(self))
        self.last = (params, index, origin)
        return inputs, target, points, inside

    def batches(self, batch_size: int, steps: int):
        """Yields batch(batch_size) `steps` times."""
        if batch_size < 1 or steps < 0:
            raise ValueError("batch_size must be positive and steps non-negative")
        for _ in range(int(steps)):
            yield self.batch(int(batch_size))


def false_positive_centres(dets, score, min_score: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(frame [K] int32, xy [K, 2] float32) of the served detections that ``evaluate`` left unmatched
    (score.pred_label == -1): the false positives of `dets`, as rows for ``SceneCrops.add_centres``.  min_score: the
    score_threshold the evaluation was made with (detections below it were not served).  The served set is
    ``score.served`` when the score carries it (``evaluate`` fills it: detections inside an ignore region are not in
    it), otherwise the first min(count, cap) slots.  Torch ops on the small arrays,
    on whatever device they live; the result's length depends on the data, so this SYNCHRONISES with the host -- it is
    meant to run between epochs, not inside the training loop."""
    cap = dets.cap
    served = getattr(score, "served", None)
    if served is None:
        served = torch.arange(cap, device=dets.score.device).view(1, 1, cap) < dets.count.clamp(max=cap).unsqueeze(-1)
    elif tuple(served.shape) != tuple(dets.score.shape):
        raise ValueError("score is not the evaluation of these detections")
    if min_score is not None:
        served = served & (dets.score >= float(min_score))
    if tuple(score.pred_label.shape) != tuple(served.shape):
        raise ValueError("score is not the evaluation of these detections")
    wrong = served & (score.pred_label == -1)
    return wrong.nonzero()[:, 0].to(torch.int32), dets.xy[wrong].contiguous()
