"""Device-resident input pipeline (csrc/loader.hip): the data set stays on the GPU as decoded images and key-point
labels, and a training batch -- gathered, augmented, normalised, labels carried through the same transform -- is one or
two launches with no host data work per step.

The reference's DatasetsBase.__getitem__ decodes a PIL image and applies an empty transforms.Compose; its trainer builds
the float batch on the host.  Here:

    loader = DeviceLoader(images_u8, labels, out_size=(256, 256), augment=Augment(translate=(8, 8)))
    for inputs, points, inside in loader.epoch(batch_size=32):
        target = heatmap.create_heatmap(points)
        train_step(model, optimizer, criterion, inputs, target)

Conventions.  Coordinates are pixel indices and a pixel centre is an integer (align_corners=True).  A sample's transform
is a row of 16 floats: the inverse map (output pixel -> source position) the image is resampled by, the forward map
(source -> output) its labels go through, a gain and a bias: out = gain * (v * mul[c] + add[c]) + bias.  The default
Augment is the exact family -- flips, quarter turns and whole-pixel shifts are pixel permutations under the bilinear
kernel, so a three-pixel blob is never blurred; rotation and scale are opt-in.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops

__all__ = ["affine_params", "warp_batch", "Augment", "DeviceLoader"]


def affine_params(forward_3x2, gain=1.0, bias=0.0) -> torch.Tensor:
    """Parameter rows [N, 16] (CPU float32) from forward maps, source -> output: forward_3x2 is [N, 2, 3] or [2, 3],
    rows (a, b, c) of x_o = a x_s + b y_s + c and y_o likewise.  The inverse is taken in float64.  gain / bias: scalars
    or [N]."""
    f = torch.as_tensor(forward_3x2, dtype=torch.float64).reshape(-1, 2, 3)
    n = f.shape[0]
    lin = f[:, :, :2]
    det = lin[:, 0, 0] * lin[:, 1, 1] - lin[:, 0, 1] * lin[:, 1, 0]
    if bool((det == 0).any()) or not bool(torch.isfinite(f).all()):
        raise ValueError("a forward map must be finite and invertible")
    inv = torch.empty_like(f)
    inv[:, 0, 0], inv[:, 0, 1] = lin[:, 1, 1] / det, -lin[:, 0, 1] / det
    inv[:, 1, 0], inv[:, 1, 1] = -lin[:, 1, 0] / det, lin[:, 0, 0] / det
    inv[:, :, 2] = -(inv[:, :, :2] @ f[:, :, 2:]).squeeze(2)
    rows = torch.zeros(n, _lib.WARP_PARAMS, dtype=torch.float64)
    rows[:, 0:6] = inv.reshape(n, 6)
    rows[:, 6:12] = f.reshape(n, 6)
    rows[:, 12] = torch.as_tensor(gain, dtype=torch.float64)
    rows[:, 13] = torch.as_tensor(bias, dtype=torch.float64)
    return rows.float()


def _per_channel(v, c, device) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        t = v.to(device=device, dtype=torch.float32).reshape(-1)
        return t.expand(c).contiguous() if t.numel() == 1 else t.contiguous()
    if isinstance(v, (int, float)):
        return torch.full((c,), float(v), dtype=torch.float32, device=device)
    return torch.tensor([float(e) for e in v], dtype=torch.float32, device=device)


def _channels(store: torch.Tensor) -> int:
    if store.dim() != 4:
        raise ValueError("store must be uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws]")
    return int(store.shape[3] if store.dtype == torch.uint8 else store.shape[1])


def _source_size(store: torch.Tensor):
    return (int(store.shape[1]), int(store.shape[2])) if store.dtype == torch.uint8 else (int(store.shape[2]), int(store.shape[3]))


def warp_batch(store, index, params, out_size, mul=1.0, add=0.0, fill=0.0, labels=None, out=None):
    """inputs [N, C, Ho, Wo] float32 = samples index [N] (int64) of the store, each resampled by its row of params
    [N, 16], out = gain * (v * mul[c] + add[c]) + bias; with labels [M, S, 2] as (x, y): (inputs, labels_out [N, S, 2],
    inside [N, S] uint8).  store: uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws] on the GPU.  mul / add: scalars,
    sequences or tensors of C values.  fill (source units) is what lies outside the source frame.  An index outside
    [0, M) gives an all-fill sample and (-1, -1) labels.  One launch; everything stays on the device."""
    if not isinstance(store, torch.Tensor) or not store.is_cuda:
        raise RuntimeError("store must live on the GPU: this path has no CPU fallback")
    c = _channels(store)
    dev = store.device
    return ops.warp_batch(store, index, params, out_size, _per_channel(mul, c, dev), _per_channel(add, c, dev), fill,
                          labels, out)


class Augment:
    """What DeviceLoader draws per sample.  flip_h / flip_v: probabilities; rot90: 0..3 quarter turns; rotate: degrees,
    uniform in [-rotate, rotate]; scale: (lo, hi), log-uniform; translate: (max_x, max_y) source pixels, always rounded
    to whole pixels; contrast: (lo, hi) gain; brightness: bias uniform in [-brightness, brightness] (output units).
    The defaults resample nothing: with rotate = 0 and scale = (1, 1) every output pixel is a source pixel or fill
    (given source and output sizes of equal parity; a quarter turn pairs the output width with the source height)."""

    def __init__(self, flip_h=0.5, flip_v=0.5, rot90=True, rotate=0.0, scale=(1.0, 1.0), translate=(0, 0),
                 contrast=(1.0, 1.0), brightness=0.0):
        self.flip_h, self.flip_v, self.rot90, self.rotate = float(flip_h), float(flip_v), bool(rot90), float(rotate)
        self.scale = (float(scale[0]), float(scale[1]))
        self.translate = (float(translate[0]), float(translate[1]))
        self.contrast = (float(contrast[0]), float(contrast[1]))
        self.brightness = float(brightness)
        if not (0.0 <= self.flip_h <= 1.0 and 0.0 <= self.flip_v <= 1.0):
            raise ValueError("flip probabilities lie in [0, 1]")
        if not 0.0 < self.scale[0] <= self.scale[1]:
            raise ValueError("scale = (lo, hi) with 0 < lo <= hi")
        if self.rotate < 0 or min(self.translate) < 0 or self.brightness < 0 or self.contrast[0] > self.contrast[1]:
            raise ValueError("rotate, translate and brightness are magnitudes; contrast = (lo, hi) with lo <= hi")

    def desc(self) -> "_lib.AugmentDesc":
        return _lib.AugmentDesc(self.flip_h, self.flip_v, int(self.rot90), self.rotate, self.scale[0], self.scale[1],
                                self.translate[0], self.translate[1], self.contrast[0], self.contrast[1],
                                self.brightness, 0)

    def draw(self, n: int, seed: int, src_size, out_size, device) -> torch.Tensor:
        """params [n, 16] on the device for n samples from a 64-bit seed: one launch."""
        return ops.augment_draw(n, seed, src_size, out_size, self.desc(), device)

    def __repr__(self):
        return ("Augment(flip_h=%g, flip_v=%g, rot90=%s, rotate=%g, scale=%s, translate=%s, contrast=%s, brightness=%g)"
                % (self.flip_h, self.flip_v, self.rot90, self.rotate, self.scale, self.translate, self.contrast,
                   self.brightness))


class DeviceLoader:
    """A data set held on the device.  images: uint8 [M, Hs, Ws, C] (decoded, channels last) or float32 [M, C, Hs, Ws];
    labels: float32 [M, S, 2] as (x, y), (-1, -1) = none, or None; both on the GPU.  out_size = (Ho, Wo): a crop or a pad
    about the centre when it differs from the source size.  inputs = gain * (pixel * mul[c] + add[c]) + bias.

    batch(index) -> (inputs [N, C, Ho, Wo], labels [N, S, 2], inside [N, S] uint8): two launches (draw, warp), or one with
    augment=None (a centred identity row built once).  epoch() yields such batches.  A run is reproducible from `seed`:
    the per-batch seeds come from a host generator, the epoch's permutation from a device generator seeded by seed and
    the epoch count.  Nothing here synchronises with the host."""

    def __init__(self, images, labels, out_size, mul=1.0 / 255.0, add=0.0, fill=0.0, augment: Optional[Augment] = None,
                 seed: int = 0):
        if not isinstance(images, torch.Tensor) or not images.is_cuda:
            raise RuntimeError("images must live on the GPU: this path has no CPU fallback")
        if images.dtype not in (torch.uint8, torch.float32):
            raise TypeError("images must be uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws], got %s" % images.dtype)
        c = _channels(images)
        if labels is not None:
            if not labels.is_cuda:
                raise RuntimeError("labels must live on the GPU: this path has no CPU fallback")
            if labels.dim() != 3 or labels.shape[0] != images.shape[0] or labels.shape[2] != 2:
                raise ValueError("labels must be [M, S, 2] with the images' M")
            labels = labels.to(torch.float32).contiguous()
        self.images, self.labels = images.contiguous(), labels
        self.device = images.device
        self.out_size = (int(out_size[0]), int(out_size[1]))
        self.src_size = _source_size(images)
        self.mul, self.add = _per_channel(mul, c, self.device), _per_channel(add, c, self.device)
        self.fill = float(fill)
        self.augment = augment
        self.seed = int(seed)
        self.epochs = 0
        self._seeds = torch.Generator().manual_seed(self.seed)
        (hs, ws), (ho, wo) = self.src_size, self.out_size
        self._identity = affine_params([[1.0, 0.0, (wo - 1) / 2.0 - (ws - 1) / 2.0],
                                        [0.0, 1.0, (ho - 1) / 2.0 - (hs - 1) / 2.0]]).to(self.device)
        self._identity_rows = {}

    def __len__(self):
        return int(self.images.shape[0])

    def _next_seed(self) -> int:
        return int(torch.randint(0, 2 ** 62, (1,), generator=self._seeds, dtype=torch.int64))

    def _rows(self, n: int) -> torch.Tensor:
        if self.augment is not None:
            return self.augment.draw(n, self._next_seed(), self.src_size, self.out_size, self.device)
        rows = self._identity_rows.get(n)
        if rows is None:
            rows = self._identity_rows[n] = self._identity.expand(n, _lib.WARP_PARAMS).contiguous()
        return rows

    def batch(self, index):
        """index: int64 [N] on the device (a list or a CPU tensor is copied over)."""
        if not isinstance(index, torch.Tensor):
            index = torch.tensor(index, dtype=torch.int64)
        index = index.to(device=self.device, dtype=torch.int64).contiguous()
        got = ops.warp_batch(self.images, index, self._rows(int(index.numel())), self.out_size, self.mul, self.add,
                             self.fill, self.labels)
        return got if self.labels is not None else (got, None, None)

    def epoch(self, batch_size: int, shuffle: bool = True, drop_last: bool = True):
        """Yields batch(index) over the whole data set once, in an order drawn on the device."""
        m = len(self)
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        if shuffle:
            g = torch.Generator(device=self.device)
            g.manual_seed((self.seed * 1000003 + self.epochs) & 0x7FFFFFFFFFFFFFFF)
            order = torch.randperm(m, generator=g, device=self.device)
        else:
            order = torch.arange(m, device=self.device)
        self.epochs += 1
        stop = m - m % batch_size if drop_last else m
        for i in range(0, stop, batch_size):
            yield self.batch(order[i:min(i + batch_size, stop)])
