"""Ignore regions of partially labelled scenes: where in a frame nothing is known.

    ign   = IgnoreRegions(rects, rect_class=None)                      # axis-aligned rectangles
    ign   = IgnoreMask.from_raster(no_data)                            # a raster mask [S, H, W], packed to bit planes
    ign   = IgnoreMask.from_polygons(vertices, counts, (H, W))         # polygon rings, holes by clearing rings
    ign   = IgnoreUnion(regions, mask)                                 # the or of several
    crops = SceneCrops(frames, labels, label_class, 4, ignore=ign, ignore_outside=True)    # target -1 inside them
    crit  = PenaltyReducedFocalLoss(ignore_negative=True)                                   # a negative target: no loss
    score = evaluate(dets, labels, label_class, 3.0, ignore=ign)                            # neither tp, fp nor fn

One convention carries it through training: a target element that is negative is ignored, so no new tensor passes
through ``train_step``, ``GraphedTrainStep``, ``dp``, ``loss_and_backward`` or ``forward_pruned``.  These classes are the
single statement of the rules for scoring; ``unetpp_target_ignore`` (csrc/crops.hip) and ``unetpp_target_ignore_mask``
(csrc/mask.hip) apply the same comparisons to the source positions of a window's pixels.

Coordinates are (x, y) with pixel centres at integers, the labels' convention everywhere in the package.

The mask layout.  ``bits`` is int32 [S, P, H, ceil(W / 32)]: bit ``x & 31`` of word ``x >> 5`` of row y is pixel (x, y);
the unused high bits of a row's last word are zero.  ``plane_class`` is int32 [P] with the meanings of ``rect_class``:
-1 every class, c class c only, anything else no class.

The lookup rule (the mark kernel and ``IgnoreMask.contains``).  A float32 position (xs, ys) is in the frame when
0 <= xs <= W - 1 and 0 <= ys <= H - 1 -- the comparisons of the rectangle kernel's `outside` test, so a NaN is outside.
Its pixel is xi = clamp(int(floorf(xs + 0.5f)), 0, W - 1), yi likewise.  It is ignored for class c when some plane whose
class is -1 or c has that bit set.  Outside the frame nothing is contained: the mark kernel's `outside` flag decides
there, as it does for rectangles.

The polygon rule (``from_polygons``).  A pixel is its centre, the integer point (px, py).  For each used edge of a ring,
the closing edge included, order the endpoints so that y0 <= y1; an edge with y0 == y1 is skipped.  The edge straddles
when y0 <= py < y1.  For a straddling edge, d = (x1 - x0) * (py - y0) - (px - x0) * (y1 - y0) in float64, in exactly this
order, every operation rounded on its own; the edge toggles the pixel when d > 0.  The pixel is inside the ring when
the number of toggles is odd.  The endpoint ordering makes two rings that share an edge compute the same d, so a pixel
on the shared edge belongs to exactly one of them in floating point as well.  A pixel's bit in plane p is the result of
walking that plane's rings in list order: set by an inside, non-clearing ring, cleared by an inside, clearing ring.
For an axis-aligned ring on integer corners (x0, y0)-(x1, y1) this gives the pixels x0 <= px < x1, y0 <= py < y1: left
and top sides inclusive, right and bottom exclusive.
"""
from __future__ import annotations

import torch

__all__ = ["IgnoreRegions", "IgnoreMask", "IgnoreUnion"]


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


def _plane_class(plane_class, p, device) -> torch.Tensor:
    if plane_class is None:
        return torch.full((p,), -1, dtype=torch.int32, device=device)
    k = torch.as_tensor(plane_class)
    if k.is_floating_point() or k.dtype == torch.bool:
        raise ValueError("plane_class must hold whole numbers")
    k = k.to(device=device, dtype=torch.int32).reshape(-1)
    if int(k.numel()) != p:
        raise ValueError("plane_class must be [%d]" % p)
    return k.contiguous()


def _per_ring(v, s, g, device, what, default) -> torch.Tensor:
    """[S, G] or [G] -> int32 [S, G] on the device"""
    if v is None:
        return torch.full((s, g), default, dtype=torch.int32, device=device)
    t = torch.as_tensor(v)
    if t.is_floating_point():
        raise ValueError("%s must hold whole numbers or bools" % what)
    t = t.to(device=device, dtype=torch.int32)
    if t.dim() == 1:
        t = t.view(1, -1).expand(s, -1)
    if tuple(t.shape) != (s, g):
        raise ValueError("%s must be [%d, %d] or [%d]" % (what, s, g, g))
    return t.contiguous()


class IgnoreMask:
    """Packed bit planes of S frames of (H, W) pixels (the module docstring has the layout and the lookup rule): bits
    int32 [S, P, H, ceil(W / 32)], plane_class int32 [P], size = (H, W).  Built by ``from_raster`` or
    ``from_polygons``; lives on the device of `bits`."""

    def __init__(self, bits, size, plane_class=None):
        bits = torch.as_tensor(bits)
        h, w = int(size[0]), int(size[1])
        if bits.dtype != torch.int32 or bits.dim() != 4:
            raise ValueError("bits must be int32 [S, P, H, ceil(W / 32)]")
        if h < 1 or w < 1 or int(bits.shape[2]) != h or int(bits.shape[3]) != (w + 31) // 32:
            raise ValueError("bits %s do not hold frames of %d x %d" % (tuple(bits.shape), h, w))
        self.bits, self.size = bits.contiguous(), (h, w)
        self.plane_class = _plane_class(plane_class, int(bits.shape[1]), bits.device)

    # ---- construction
    @classmethod
    def from_raster(cls, mask, plane_class=None) -> "IgnoreMask":
        """mask [S, H, W] or [S, P, H, W], bool, uint8 or float: a non-zero pixel sets the bit (a NaN is non-zero, -0.0
        is zero).  On the GPU one launch (unetpp_mask_pack) for bool, uint8 and float32 -- another type is compared
        with zero first; on the CPU packed with torch ops."""
        mask = torch.as_tensor(mask)
        if mask.dim() == 3:
            mask = mask.unsqueeze(1)
        if mask.dim() != 4 or min(int(v) for v in mask.shape[2:]) < 1:
            raise ValueError("mask must be [S, H, W] or [S, P, H, W]")
        s, p, h, w = (int(v) for v in mask.shape)
        if mask.is_cuda and s * p > 0:
            from . import ops
            bits = ops.mask_pack(mask.contiguous())
        else:
            bits = _pack_torch(mask != 0)
        return cls(bits, (h, w), plane_class)

    @classmethod
    def from_polygons(cls, vertices, counts, size, poly_plane=None, poly_clear=None, plane_class=None) -> "IgnoreMask":
        """vertices float32 [S, G, V, 2] as (x, y); counts int [S, G], the vertices used per ring (fewer than 3 or more
        than V, or a NaN / inf in a used vertex: padding); size = (H, W); poly_plane [S, G] or [G], default 0 (a plane
        outside 0..P-1: padding); poly_clear [S, G] or [G] bool: a clearing ring removes what earlier rings of its
        plane set.  The number of planes is len(plane_class), or max(poly_plane) + 1 (a host read), or 1.  One launch
        (unetpp_mask_polygons) by the polygon rule of the module docstring; there is no CPU path."""
        from . import ops
        vertices = torch.as_tensor(vertices, dtype=torch.float32)
        if vertices.dim() != 4 or vertices.shape[3] != 2:
            raise ValueError("vertices must be [S, G, V, 2] as (x, y)")
        if not vertices.is_cuda:
            raise RuntimeError("vertices must live on the GPU: this path has no CPU fallback")
        dev = vertices.device
        s, g = int(vertices.shape[0]), int(vertices.shape[1])
        counts = _per_ring(counts, s, g, dev, "counts", 0)
        plane = _per_ring(poly_plane, s, g, dev, "poly_plane", 0)
        clear = _per_ring(poly_clear, s, g, dev, "poly_clear", 0)
        if plane_class is not None:
            p = int(torch.as_tensor(plane_class).numel())
        else:
            p = max(1, int(plane.max()) + 1) if poly_plane is not None and plane.numel() > 0 else 1
        if p < 1:
            raise ValueError("a mask has at least one plane")
        h, w = int(size[0]), int(size[1])
        bits = ops.mask_polygons(vertices.contiguous(), counts, plane, clear, p, (h, w))
        return cls(bits, (h, w), plane_class)

    # ---- the container
    def __len__(self):
        return int(self.bits.shape[0])

    @property
    def device(self):
        return self.bits.device

    @property
    def planes(self) -> int:
        return int(self.bits.shape[1])

    def to(self, device) -> "IgnoreMask":
        device = torch.device(device)
        if device == self.bits.device:
            return self
        return IgnoreMask(self.bits.to(device), self.size, self.plane_class.to(device))

    def to_raster(self) -> torch.Tensor:
        """bool [S, P, H, W] (torch ops)"""
        h, w = self.size
        shifts = torch.arange(32, device=self.bits.device, dtype=torch.int32)
        out = (self.bits.unsqueeze(-1) >> shifts) & 1                     # [S, P, H, Wd, 32]
        return out.reshape(*self.bits.shape[:3], -1)[..., :w].ne(0)

    def coverage(self) -> torch.Tensor:
        """float64 [S, P]: the share of set pixels per frame and plane"""
        h, w = self.size
        return self.to_raster().sum(dim=(2, 3)).to(torch.float64) / float(h * w)

    def union(self, other: "IgnoreMask") -> "IgnoreMask":
        """word-wise or of two masks of the same geometry and plane classes"""
        if not isinstance(other, IgnoreMask):
            raise TypeError("union takes an IgnoreMask")
        other = other.to(self.device)
        if tuple(other.bits.shape) != tuple(self.bits.shape) or other.size != self.size or \
                not torch.equal(other.plane_class, self.plane_class):
            raise ValueError("a union needs equal geometry and plane_class")
        return IgnoreMask(self.bits | other.bits, self.size, self.plane_class)

    def contains(self, frame, cls, xy) -> torch.Tensor:
        """bool tensor of the shape of xy[..., 0] by the lookup rule: true where the point is in the frame and the bit
        of its nearest pixel is set in some plane of the point's frame whose class is -1 or the point's class.  frame /
        cls: integer tensors (or ints) broadcastable to xy[..., 0]; a frame outside [0, S) holds nothing.  float32
        arithmetic on whatever device: a NaN coordinate is never inside."""
        dev = self.bits.device
        xy = torch.as_tensor(xy, dtype=torch.float32).to(dev)
        x, y = xy[..., 0], xy[..., 1]
        frame = torch.as_tensor(frame).to(dev).long().expand(x.shape)
        cls = torch.as_tensor(cls).to(dev).long().expand(x.shape)
        s, p = int(self.bits.shape[0]), int(self.bits.shape[1])
        h, w = self.size
        if s == 0 or p == 0:
            return torch.zeros(x.shape, dtype=torch.bool, device=dev)
        known = (frame >= 0) & (frame < s) & (x >= 0) & (x <= float(w - 1)) & (y >= 0) & (y <= float(h - 1))
        half = torch.tensor(0.5, dtype=torch.float32, device=dev)
        xi = torch.floor(torch.where(known, x, torch.zeros_like(x)) + half).long().clamp(0, w - 1)
        yi = torch.floor(torch.where(known, y, torch.zeros_like(y)) + half).long().clamp(0, h - 1)
        f = frame.clamp(0, s - 1)
        words = self.bits[f, :, yi, xi >> 5]                              # [..., P]
        bit = ((words >> (xi & 31).to(torch.int32).unsqueeze(-1)) & 1).ne(0)
        k = self.plane_class.long()
        applies = (k == -1) | ((k >= 0) & (k == cls.unsqueeze(-1)))
        return (bit & applies).any(-1) & known


def _pack_torch(on: torch.Tensor) -> torch.Tensor:
    """bool [S, P, H, W] -> int32 [S, P, H, ceil(W / 32)] with torch ops (the CPU path of from_raster)"""
    s, p, h, w = (int(v) for v in on.shape)
    wd = (w + 31) // 32
    padded = torch.zeros(s, p, h, wd * 32, dtype=torch.int64, device=on.device)
    padded[..., :w] = on.to(torch.int64)
    weights = torch.ones(32, dtype=torch.int64, device=on.device) << torch.arange(32, device=on.device)
    words = (padded.view(s, p, h, wd, 32) * weights).sum(-1)              # 0 .. 2^32 - 1
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)
    return words.to(torch.int32).contiguous()


class IgnoreUnion:
    """The or of several ``IgnoreRegions`` / ``IgnoreMask`` over the same number of frames: ``len``, ``to`` and
    ``contains``, which is all ``evaluate`` asks of an ignore object; ``SceneCrops`` marks with one launch per part."""

    def __init__(self, *parts):
        if len(parts) == 1 and isinstance(parts[0], (list, tuple)):
            parts = tuple(parts[0])
        flat = []
        for part in parts:
            if isinstance(part, IgnoreUnion):
                flat.extend(part.parts)
            elif isinstance(part, (IgnoreRegions, IgnoreMask)):
                flat.append(part)
            else:
                raise TypeError("the parts of an IgnoreUnion are IgnoreRegions and IgnoreMask objects")
        if not flat:
            raise ValueError("an IgnoreUnion needs at least one part")
        if any(len(part) != len(flat[0]) for part in flat):
            raise ValueError("the parts of an IgnoreUnion must hold the same number of frames")
        self.parts = tuple(flat)

    def __len__(self):
        return len(self.parts[0])

    @property
    def device(self):
        return self.parts[0].device

    def to(self, device) -> "IgnoreUnion":
        device = torch.device(device)
        if all(part.device == device for part in self.parts):
            return self
        return IgnoreUnion(*[part.to(device) for part in self.parts])

    def contains(self, frame, cls, xy) -> torch.Tensor:
        dev = self.parts[0].device
        out = None
        for part in self.parts:
            hit = part.contains(frame, cls, xy).to(dev)
            out = hit if out is None else out | hit
        return out
