"""One validation batch on the device: the loop body of the reference's ``val_epoch_`` (trainer/trainer.py:203-223).

Per batch the reference runs the eval forward, builds the target maps with ``heatmaper.create_heatmap(labels)`` and, for
every head, ``FocalLoss_BCE_2d`` against them, ``heatmaper.transfer_points`` (heat map -> key points) and
``nn.MSELoss()(preds, labels)``.  Its matcher is unfinished (tools/misc/heatmap.py:57-79), so that landmark loss never
ran.  Here it is defined as MSELoss over the labels a prediction was matched to (``Heatmap.match_points``), and the
whole batch stays on the device:

- the heads' FocalLoss_BCE_2d values: one launch for every head (``ops.focal_bce_heads``, same bits as the criterion);
- key points of every map of every head: one ``ops.keypoints_extract`` over the stacked heads;
- matching and landmark loss of every head: one launch (csrc/validate.hip).

Nothing is read back to the host beyond the convergence flags the extraction reads.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import torch

from . import _lib, ops
from .losses import FocalLoss_BCE_2d


class ValidateResult(NamedTuple):
    outputs: Tuple[torch.Tensor, ...]   # the heads, as the forward returned them
    heatmap_losses: torch.Tensor        # [heads] criterion(head, target)
    landmark_losses: torch.Tensor       # [heads] MSELoss over the matched coordinates, NaN where nothing matched
    points: torch.Tensor                # [heads, N, S, 2] prediction matched to label s, (-1, -1) where none
    mask: torch.Tensor                  # [heads, N, S] bool, label s matched
    matched_count: torch.Tensor         # [heads] int32


def _check_labels(heatmaper, labels, batch=None):
    if labels.dim() != 3 or labels.shape[2] != 2:
        raise ValueError("labels must be [N, S, 2] as (x, y)")
    if batch is not None and labels.shape[0] != batch:
        raise ValueError("labels hold %d images, the batch %d" % (labels.shape[0], batch))
    ops.check_match_pattern(heatmaper.pattern, labels.shape[1])


def _heads_of(outputs):
    return tuple(outputs) if isinstance(outputs, (tuple, list)) else (outputs,)


def _head_losses(criterion, heads, target):
    """criterion(head, target) for every head -> [heads]; this package's FocalLoss_BCE_2d on fp32 GPU heads in one launch"""
    if (isinstance(criterion, FocalLoss_BCE_2d) and len(heads) <= _lib.MAX_HEADS
            and all(o.is_cuda and o.dtype == torch.float32 and o.shape == target.shape and o.is_contiguous()
                    and o.device == target.device for o in heads)):
        rows = target.numel() if criterion.size_average else target.shape[0] * target.shape[1]
        loss, _ = ops.focal_bce_heads(list(heads), target, rows, float(criterion.gamma), want_grad=False)
        return loss[1:]
    return torch.stack([criterion(o, target).reshape(()) for o in heads])


def validate_outputs(outputs, criterion, heatmaper, labels, threshold=0.5) -> ValidateResult:
    """Everything of a validation batch after the forward: `outputs` = the head tuple (or one map) [N, C, H, W] fp32 on the
    GPU, `labels` [N, S, 2] on the GPU, `heatmaper` a ``Heatmap`` whose pattern has C maps of H x W."""
    heads = _heads_of(outputs)
    c = len(heatmaper.pattern)
    for o in heads:
        if o.dim() != 4 or o.shape[1] != c:
            raise ValueError("heads must be [N, %d, H, W]: one channel per map of the pattern" % c)
        if (o.shape[2], o.shape[3]) != (heatmaper.h, heatmaper.w):
            raise ValueError("heads are %dx%d, the heat-map helper makes %dx%d maps" % (
                o.shape[2], o.shape[3], heatmaper.h, heatmaper.w))
        if o.shape != heads[0].shape:
            raise ValueError("every head must have the same shape")
    _check_labels(heatmaper, labels, heads[0].shape[0])
    if not (labels.is_cuda and all(o.is_cuda for o in heads)):
        raise RuntimeError("validate_outputs runs on the GPU: this path has no CPU fallback")
    labels = labels.to(torch.float32).contiguous()
    with torch.no_grad():
        target = heatmaper.create_heatmap(labels)
        heatmap_losses = _head_losses(criterion, heads, target)
        n, _, h, w = heads[0].shape
        stacked = torch.stack(heads).view(len(heads) * n * c, h, w)
        _, _, lengths = ops.match_pattern_tensors(heatmaper.pattern, labels.device)
        points, counts = ops.keypoints_extract(stacked, int(max(len(m) for m in heatmaper.pattern)), float(threshold),
                                               segmentation=heatmaper.segmentation)
        found = torch.minimum(counts.view(-1, c), lengths).view(-1)   # capped at the map's labels, as transfer_points
        matched, mask, loss, count = ops.match_points(points, found, labels, heatmaper.pattern, heads=len(heads))
    return ValidateResult(outputs, heatmap_losses, loss, matched, mask, count)


def validate_step(model, criterion, heatmaper, inputs, labels, threshold=0.5, forward=None) -> ValidateResult:
    """The loop body of val_epoch_ (trainer/trainer.py:203-223): eval forward under no_grad, then ``validate_outputs``.
    The model must be in eval mode (validation must not move the BatchNorm running statistics).  `forward` replaces
    ``model(inputs)``, e.g. a ``GraphedForward`` of the model (its outputs are overwritten by its next call)."""
    if model.training:
        raise RuntimeError("validate_step runs the eval forward: call model.eval() first")
    n_classes = getattr(model, "n_classes", None)
    if n_classes is not None and n_classes != len(heatmaper.pattern):
        raise ValueError("the model has %d classes, the pattern %d maps" % (n_classes, len(heatmaper.pattern)))
    if inputs.dim() != 4 or (inputs.shape[2], inputs.shape[3]) != (heatmaper.h, heatmaper.w):
        raise ValueError("inputs must be [N, C, %d, %d] for the heat-map helper's maps" % (heatmaper.h, heatmaper.w))
    _check_labels(heatmaper, labels, inputs.shape[0])
    if not (inputs.is_cuda and labels.is_cuda):
        raise RuntimeError("validate_step runs on the GPU: this path has no CPU fallback")
    with torch.no_grad():
        outputs = forward(inputs) if forward is not None else model(inputs)
    return validate_outputs(outputs, criterion, heatmaper, labels, threshold)
