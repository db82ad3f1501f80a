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

Copy-paste of tiny objects: ``paste=ObjectPaste(max_pastes=4, p=0.5, patch_radius=4)`` copies the few pixels of labelled
objects to new places of a window, with their label (csrc/paste.hip): three more launches per batch
(where, the pixels, the targets), still without host data work.  ``points`` and ``inside`` stay the frame's labels; the
pasted ones are in ``last_paste``.

Coordinates are (x, y) with pixel centres at integers, the labels' convention everywhere in the package.  The reference
has no counterpart.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib, ops
from .ignore import IgnoreMask, IgnoreRegions, IgnoreUnion
from .loader import Augment, _channels, _per_channel, _source_size

__all__ = ["SceneCrops", "ObjectPaste", "PasteRows", "false_positive_centres"]

_PASTE_SEED = 0x5041535445524F57   # the paste's seed is the batch's seed xor this: one draw of the host generator per batch


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


class PasteRows(NamedTuple):
    """What a batch pasted, K slots per window, on the device: src [N, K] int32 (the row of the source table, -1: a void
    slot), dst [N, K, 2] int32 as (px, py), code [N, K] int32 (0..7: q = code & 3 quarter turns, then a flip in x when
    code & 4), xy [N, K, 2] float32 (the pasted label, (-1, -1) when void), cls [N, K] int32 (its class, -1 when void)."""
    src: torch.Tensor
    dst: torch.Tensor
    code: torch.Tensor
    xy: torch.Tensor
    cls: torch.Tensor


def paste_alpha(patch_radius: int, core: float) -> torch.Tensor:
    """The blend weights [2R+1, 2R+1] float32 (CPU): clamp((R + 0.5 - d) / (R + 0.5 - core), 0, 1) of the distance d from
    the patch's centre, formed in float64 and rounded once; 1 within `core`, 0 from R + 0.5 on, linear between.  The
    table is symmetric under the eight flips and quarter turns."""
    r = int(patch_radius)
    edge = r + 0.5
    rows = [[min(1.0, max(0.0, (edge - math.sqrt(float(i * i + j * j))) / (edge - float(core))))
             for i in range(-r, r + 1)] for j in range(-r, r + 1)]
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32)


def paste_source_table(labels: torch.Tensor, label_class: torch.Tensor, n_classes: int, src_size, patch_radius: int,
                       ignore=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(frame [T] int32, xy [T, 2] float32, cls [T] int32) of the labels whose patch can be pasted, on the labels' device:
    labels [S, L, 2] float32 and label_class [S, L] of frames of src_size = (Hs, Ws).  A label is admitted when it is valid
    (class in [0, n_classes), no negative coordinate), the (2R+1) x (2R+1) patch about its rounded centre c = floor(xy +
    0.5) lies inside the frame, no other valid label of the frame lies within Chebyshev distance R + 1 of c (the patch
    then holds exactly one object), and c lies in no rectangle of `ignore` of its frame -- for an ``IgnoreMask`` or an
    ``IgnoreUnion``: ``ignore.contains`` is false at c for the label's class.  Torch ops, frame by frame; the length
    depends on the data, so this synchronises with the host: for a constructor, not for the training loop."""
    r, (hs, ws) = int(patch_radius), (int(src_size[0]), int(src_size[1]))
    xy = labels.to(torch.float64)
    cls = label_class.to(torch.int64)
    valid = (cls >= 0) & (cls < int(n_classes)) & ~(labels[..., 0] < 0) & ~(labels[..., 1] < 0)
    c = torch.floor(xy + 0.5)
    inside = (c[..., 0] >= r) & (c[..., 0] <= ws - 1 - r) & (c[..., 1] >= r) & (c[..., 1] <= hs - 1 - r)
    ok = valid & inside
    for s in range(int(labels.shape[0])):   # [L, L] per frame: centre a against label b
        cheb = (xy[s].unsqueeze(0) - c[s].unsqueeze(1)).abs().amax(dim=-1)
        crowd = (cheb <= r + 1) & valid[s].unsqueeze(0)
        crowd.fill_diagonal_(False)
        ok[s] &= ~crowd.any(dim=1)
    if isinstance(ignore, (IgnoreMask, IgnoreUnion)):
        frame = torch.arange(int(labels.shape[0]), device=labels.device).view(-1, 1)
        known = torch.where(valid, cls, torch.full_like(cls, -2))      # (an invalid label is dropped anyway)
        ok &= ~ignore.contains(frame, known, c.to(torch.float32)).to(labels.device)
    elif ignore is not None and int(ignore.rects.shape[1]) > 0:
        rc = ignore.rects.to(labels.device).to(torch.float64).unsqueeze(1)         # [S, 1, R, 4]
        k = ignore.rect_class.to(labels.device).unsqueeze(1)
        cx, cy = c[..., 0].unsqueeze(-1), c[..., 1].unsqueeze(-1)
        hit = (rc[..., 0] <= cx) & (cx <= rc[..., 2]) & (rc[..., 1] <= cy) & (cy <= rc[..., 3])
        ok &= ~(hit & (k >= -1) & (k < int(n_classes))).any(dim=-1)
    where = ok.nonzero()
    return (where[:, 0].to(torch.int32).contiguous(), labels[ok].to(torch.float32).contiguous(),
            label_class[ok].to(torch.int32).contiguous())


class ObjectPaste:
    """Copy-paste augmentation for ``SceneCrops(..., paste=ObjectPaste(...))``: per window max_pastes = K slots, each of
    which attempts a paste with probability p.  A paste copies the (2R+1) x (2R+1) whole pixels (R = patch_radius) about a
    row of the source table to a place of the window where no label of the frame lies within `clearance` (default 2R)
    and no earlier paste of the window overlaps, under one of the eight flips and quarter turns (dihedral) -- or is void.
    The patch is blended in with weight 1 within `core` pixels of its centre (core < R + 0.5), falling linearly to 0 at
    R + 0.5.  The source table is built by ``SceneCrops`` from its labels (``paste_source_table``); ``set_sources``
    replaces it.  One object serves one ``SceneCrops``."""

    def __init__(self, max_pastes: int = 4, p: float = 0.5, patch_radius: int = 4, core: float = 2.5,
                 clearance: Optional[float] = None, dihedral: bool = True):
        for name, v in (("max_pastes", max_pastes), ("patch_radius", patch_radius)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError("%s must be an int, got %r" % (name, v))
        if not 1 <= max_pastes <= _lib.PASTE_MAX_SLOTS:
            raise ValueError("max_pastes must lie in 1..%d, got %r" % (_lib.PASTE_MAX_SLOTS, max_pastes))
        if not 0 <= patch_radius <= _lib.PASTE_MAX_RADIUS:
            raise ValueError("patch_radius must lie in 0..%d, got %r" % (_lib.PASTE_MAX_RADIUS, patch_radius))
        self.max_pastes, self.patch_radius = max_pastes, patch_radius
        self.p, self.core = float(p), float(core)
        if not 0.0 <= self.p <= 1.0:
            raise ValueError("p lies in [0, 1], got %r" % (p,))
        if not 0.0 <= self.core < patch_radius + 0.5:
            raise ValueError("core must lie in [0, patch_radius + 0.5), got %r" % (core,))
        self.clearance = 2.0 * patch_radius if clearance is None else float(clearance)
        if not self.clearance >= 0.0 or math.isinf(self.clearance):
            raise ValueError("clearance must be a finite number that is not negative, got %r" % (clearance,))
        self.dihedral = bool(dihedral)
        self.alpha = paste_alpha(patch_radius, self.core)
        self.src_frame = self.src_xy = self.src_class = None
        self._frames = self._classes = None

    def _bind(self, crops: "SceneCrops") -> None:
        """the source table from the scenes' labels; ValueError when no label can be pasted"""
        r = self.patch_radius
        if min(crops.crop) < 2 * r + 1:
            raise ValueError("the window must be at least %d on both sides for patch_radius %d" % (2 * r + 1, r))
        self._frames, self._classes = len(crops), crops.n_classes
        self.alpha = self.alpha.to(crops.device).contiguous()
        f, xy, c = paste_source_table(crops.labels, crops.label_class, crops.n_classes, crops.src_size, r, crops.ignore)
        if f.numel() == 0:
            raise ValueError("no label can be pasted: none is valid, %d pixels inside its frame, alone in its patch and "
                             "outside every ignore region" % r)
        self.src_frame, self.src_xy, self.src_class = f, xy, c

    def set_sources(self, frame, xy, cls) -> None:
        """Replace the source table: frame [T] whole numbers in [0, S), xy [T, 2] as (x, y), finite, cls [T] whole numbers
        in [0, n_classes); T >= 1.  A row whose patch is not inside its frame is never pasted (the kernels test it).  Reads
        back to check: between epochs, not per step."""
        if self._frames is None:
            raise ValueError("set_sources needs the scenes: pass the object to SceneCrops(paste=...) first")
        device = self.alpha.device
        f, p = _centre_table(frame, xy, self._frames, device)
        c = torch.as_tensor(cls).reshape(-1)
        if c.is_floating_point() or c.dtype == torch.bool:
            raise ValueError("cls must hold whole numbers")
        if c.numel() != f.numel() or f.numel() == 0:
            raise ValueError("one class per source and at least one source: got %d frames and %d classes"
                             % (f.numel(), c.numel()))
        if int(c.min()) < 0 or int(c.max()) >= self._classes:
            raise ValueError("a source's class must lie in [0, %d)" % self._classes)
        self.src_frame, self.src_xy = f, p
        self.src_class = c.to(device=device, dtype=torch.int32).contiguous()


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
    batch(n) a fourth launch (unetpp_target_ignore) after the targets, still without a host synchronisation.  An
    ``IgnoreMask`` of the frames' size (bit planes from a raster or from polygons) marks by one bit lookup per pixel and
    plane instead (unetpp_target_ignore_mask); an ``IgnoreUnion`` takes one launch per part, and ignore_outside is
    applied by exactly one of them.

    paste: an ``ObjectPaste`` -- batch(n) then also copies objects of its source table into the windows (three more
    launches: unetpp_paste_draw, unetpp_paste_apply after the warp, unetpp_paste_target after the targets and before the
    ignore marks, so a patch that lands in an ignore region is ignored like anything else there); ``last_paste`` holds
    the batch's ``PasteRows``.  points and inside stay the frame's labels.  The paste draws from the batch's own seed:
    with p = 0 the batches are those of an object without paste, bit for bit.

    The centre table starts as the valid labels; set_centres / add_centres replace / extend it -- a sampling policy such
    as class balancing is a matter of what the caller puts there.

    teacher: float32 [S, n_classes, H, W] on the frames' device and of the frames' size -- what
    ``SceneInference(...)(frames)`` returns -- as a soft target for ``TeacherDistillLoss``: batch(n) then cuts the same
    windows out of it by one more unetpp_warp_batch launch (the batch's own index and params rows with gain 1 and bias 0,
    mul 1, add 0, fill -1) into ``last_teacher`` [n, n_classes, Ho, Wo]: every element is a teacher element, or -1
    ("no teacher") outside the frame.  Only under the augmentations that resample nothing (rotate = 0, scale = (1, 1)),
    with at most 8 classes (the warp's channel limit) and without paste (a pasted object is not in the teacher's map):
    anything else raises ValueError.  The teacher's values are finite.  inputs, target, points and inside are the bits
    of an object without teacher; the seed stream is untouched."""

    def __init__(self, frames, labels, label_class, n_classes: int, crop=(256, 256), p_object: float = 0.75,
                 jitter=(32, 32), augment: Optional[Augment] = None, radius: float = 3.0, mul=1.0 / 255.0, add=0.0,
                 fill: float = 0.0, seed: int = 0, ignore=None, ignore_outside: bool = False,
                 paste: Optional[ObjectPaste] = None, teacher: Optional[torch.Tensor] = None):
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
            if not isinstance(ignore, (IgnoreRegions, IgnoreMask, IgnoreUnion)):
                raise TypeError("ignore must be an IgnoreRegions, an IgnoreMask or an IgnoreUnion")
            if len(ignore) != s:
                raise ValueError("ignore holds %d frames, the scenes %d" % (len(ignore), s))
            for part in ignore.parts if isinstance(ignore, IgnoreUnion) else (ignore,):
                if isinstance(part, IgnoreMask) and tuple(part.size) != tuple(self.src_size):
                    raise ValueError("an ignore mask of %d x %d over frames of %d x %d" % (part.size + tuple(self.src_size)))
            self.ignore = ignore.to(self.device)
        self.paste, self.last_paste = None, None
        if paste is not None:
            if not isinstance(paste, ObjectPaste):
                raise TypeError("paste must be an ObjectPaste")
            paste._bind(self)
            self.paste = paste
        self.teacher, self.last_teacher = None, None
        if teacher is not None:
            self._bind_teacher(teacher)

    def _bind_teacher(self, teacher) -> None:
        if not isinstance(teacher, torch.Tensor) or not teacher.is_cuda:
            raise RuntimeError("teacher must live on the GPU: this path has no CPU fallback")
        if teacher.dtype != torch.float32:
            raise TypeError("teacher must be float32 [S, n_classes, H, W], got %s" % teacher.dtype)
        if self.augment.rotate != 0.0 or self.augment.scale != (1.0, 1.0):
            raise ValueError("a teacher is cut only under augmentations that resample nothing: rotate = 0 and "
                             "scale = (1, 1), got %r" % (self.augment,))
        if self.paste is not None:
            raise ValueError("paste and teacher do not go together: a pasted object is not in the teacher's map")
        if self.n_classes > _lib.WARP_MAX_C:
            raise ValueError("a teacher has at most %d classes (the warp's channel limit), got %d"
                             % (_lib.WARP_MAX_C, self.n_classes))
        want = (len(self), self.n_classes, int(self.src_size[0]), int(self.src_size[1]))
        if tuple(teacher.shape) != want:
            raise ValueError("teacher must be [%d, %d, %d, %d], got %s" % (want + (tuple(teacher.shape),)))
        if teacher.device != self.device:
            raise ValueError("teacher must live on the device of the frames")
        self.teacher = teacher.detach().contiguous()
        # a drawn row's gain and bias belong to the pixels: a probability keeps its value
        a = self.augment
        self._teacher_rows_drawn = a.contrast == (1.0, 1.0) and a.brightness == 0.0   # gain 1 and bias +-0 as drawn
        self._teacher_unit = torch.tensor([1.0, 0.0], dtype=torch.float32, device=self.device)
        self._teacher_mul = torch.ones(self.n_classes, dtype=torch.float32, device=self.device)
        self._teacher_add = torch.zeros(self.n_classes, dtype=torch.float32, device=self.device)

    def _cut_teacher(self, index, params) -> torch.Tensor:
        rows = params
        if not self._teacher_rows_drawn:
            rows = params.clone()
            rows[:, 12:14] = self._teacher_unit
        return ops.warp_batch(self.teacher, index, rows, self.crop, self._teacher_mul, self._teacher_add, -1.0)

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
        seed = self._next_seed()
        params, index, origin = ops.crops_draw(n, seed, len(self), self.src_size, self.crop,
                                               self.centre_frame, self.centre_xy, self.p_object, self.jitter,
                                               self.augment.desc(), self.device)
        inputs, points, inside = ops.warp_batch(self.frames, index, params, self.crop, self.mul, self.add, self.fill,
                                                self.labels)
        ps = self.paste
        if ps is not None:
            rows = PasteRows(*ops.paste_draw(ps.max_pastes, seed ^ _PASTE_SEED, ps.src_frame, ps.src_xy, ps.src_class,
                                             self.labels, self.label_class, index, params, self.n_classes, self.src_size,
                                             self.crop, ps.p, ps.patch_radius, ps.clearance, ps.dihedral))
            ops.paste_apply(inputs, rows.src, rows.dst, rows.code, ps.src_frame, ps.src_xy, ps.src_class, self.frames,
                            params, self.mul, self.add, ps.alpha, self.n_classes)
        target = ops.points_target(self.labels, self.label_class, index, params, self.n_classes, self.crop, self.radius)
        if ps is not None:
            ops.paste_target(target, rows.xy, rows.cls, self.radius)
            self.last_paste = rows
        if self.ignore is not None or self.ignore_outside:
            ign = self.ignore
            parts = ign.parts if isinstance(ign, IgnoreUnion) else (ign,)
            for i, part in enumerate(parts):
                outside = self.ignore_outside and i == 0          # applied by exactly one launch
                if isinstance(part, IgnoreMask):
                    ops.target_ignore_mask(target, part.bits, part.plane_class, index, params, self.src_size, outside,
                                           n_frames=len(self))
                else:
                    ops.target_ignore(target, part.rects if part is not None else None,
                                      part.rect_class if part is not None else None, index, params, self.src_size,
                                      outside, n_frames=len(self))
        self.last = (params, index, origin)
        if self.teacher is not None:
            self.last_teacher = self._cut_teacher(index, params)
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
