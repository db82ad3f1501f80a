"""Ignore regions of partially labelled scenes: rectangles of a frame in which nothing is known.

    ign   = IgnoreRegions(rects, rect_class=None)
    crops = SceneCrops(frames, labels, label_class, 4, ignore=ign, ignore_outside=True)    # target -1 inside them
    crit  = PenaltyReducedFocalLoss(ignore_negative=True)                                   # a negative target: no loss
    score = evaluate(dets, labels, label_class, 3.0, ignore=ign)                            # neither tp, fp nor fn

One convention carries it through training: a target element that is negative is ignored, so no new tensor passes
through ``train_step``, ``GraphedTrainStep``, ``dp``, ``loss_and_backward`` or ``forward_pruned``.  This class is the
single statement of the rule for scoring; ``unetpp_target_ignore`` (csrc/crops.hip) applies the same comparisons to the
source positions of a window's pixels.

Coordinates are (x, y) with pixel centres at integers, the labels' convention everywhere in the package.
"""
from __future__ import annotations

import torch

__all__ = ["IgnoreRegions"]


class IgnoreRegions:
    """rects: float32 [S, R, 4] as (x0, y0, x1, y1) in source-frame pixel coordinates, both ends inclusive; a row with
    x1 < x0 or y1 < y0, or holding a NaN, is padding; R may be 0.  rect_class: int [S, R] or [R]; -1 (the default) applies
    to every class, c to class c only, any other value outside 0..C-1 is padding (it matches no class).  Lives on the
    device of `rects`; ``to(device)`` gives a copy elsewhere."""

    def __init__(self, rects, rect_class=None):
        rects = torch.as_tensor(rects, dtype=torch.float32)
        if rects.dim() != 3 or rects.shape[2] != 4:
            raise ValueError("rects must be [S, R, 4] as (x0, y0, x1, y1)")
        s, r = int(rects.shape[0]), int(rects.shape[1])
        if rect_class is None:
            cls = torch.full((s, r), -1, dtype=torch.int32, device=rects.device)
        else:
            cls = torch.as_tensor(rect_class)
            if cls.is_floating_point() or cls.dtype == torch.bool:
                raise ValueError("rect_class must hold whole numbers")
            cls = cls.to(device=rects.device, dtype=torch.int32)
            if cls.dim() == 1:
                cls = cls.view(1, -1).expand(s, -1)
            if tuple(cls.shape) != (s, r):
                raise ValueError("rect_class must be [%d, %d] or [%d]" % (s, r, r))
        self.rects, self.rect_class = rects.contiguous(), cls.contiguous()

    def __len__(self):
        return int(self.rects.shape[0])

    @property
    def device(self):
        return self.rects.device

    def to(self, device) -> "IgnoreRegions":
        device = torch.device(device)
        if device == self.rects.device:
            return self
        return IgnoreRegions(self.rects.to(device), self.rect_class.to(device))

    def contains(self, frame, cls, xy) -> torch.Tensor:
        """bool tensor of the shape of xy[..., 0]: true where x0 <= x <= x1 and y0 <= y <= y1 for some rectangle of the
        point's frame whose class is -1 or the point's class.  frame / cls: integer tensors (or ints) broadcastable to
        xy[..., 0]; a frame outside [0, S) holds no rectangle.  Plain float32 comparisons on whatever device: a NaN
        coordinate is never inside."""
        dev = self.rects.device
        xy = torch.as_tensor(xy, dtype=torch.float32).to(dev)
        x, y = xy[..., 0], xy[..., 1]
        frame = torch.as_tensor(frame).to(dev).long().expand(x.shape)
        cls = torch.as_tensor(cls).to(dev).long().expand(x.shape)
        s, r = int(self.rects.shape[0]), int(self.rects.shape[1])
        if s == 0 or r == 0:
            return torch.zeros(x.shape, dtype=torch.bool, device=dev)
        known = (frame >= 0) & (frame < s)
        f = frame.clamp(0, s - 1)
        rc = self.rects[f]                                   # [..., R, 4]
        k = self.rect_class[f].long()                        # [..., R]
        xe, ye = x.unsqueeze(-1), y.unsqueeze(-1)
        inside = (rc[..., 0] <= xe) & (xe <= rc[..., 2]) & (rc[..., 1] <= ye) & (ye <= rc[..., 3])
        applies = (k == -1) | ((k >= 0) & (k == cls.unsqueeze(-1)))
        return (inside & applies).any(-1) & known
