"""One training step, as the reference's loop body runs it (trainer/trainer.py:114-136).

zero_grad -> forward -> criterion on every deep-supervision head -> mean over heads -> backward ->
optimizer.step().  The loss and the optimizer are PyTorch-ROCm host code; forward and backward of the
network are the HIP path.  Unlike the reference the head outputs are not moved to the CPU for the loss.
"""
from __future__ import annotations

import os

import torch

# A/B switch (measurements only): the written-out loop over the heads instead of the fused loss launch
_FUSED_HEAD_LOSS = os.environ.get("UNETPP_NO_FUSED_HEAD_LOSS") is None
# A/B switch (measurements only): head forward, loss launch and head backward instead of one launch per head
_FUSED_HEAD_TRAIN = os.environ.get("UNETPP_NO_FUSED_HEAD_TRAIN") is None


def loss_and_backward(criterion, outputs, target):
    """criterion on every head, mean over heads, backward (the middle of the loop body) -> the mean loss.

    With this package's FocalLoss_BCE_2d on GPU heads the loop, its tensor arithmetic and the autograd walk back to the
    heads are one fused launch (``FocalLoss_BCE_2d.mean_over_heads``: same values bit for bit) and the network's backward is
    started directly from the head gradients; any other criterion runs the loop as written."""
    if isinstance(outputs, tuple):
        fused = getattr(criterion, "mean_over_heads", None)
        if _FUSED_HEAD_LOSS and fused is not None and torch.is_grad_enabled() and all(o.requires_grad for o in outputs):
            got = fused(outputs, target)
            if got is not None:
                avgloss, grads = got
                torch.autograd.backward(list(outputs), grads)
                return avgloss
        avgloss = 0
        for output in outputs:
            avgloss = avgloss + criterion(output, target)
        avgloss = 1.0 * avgloss / len(outputs)
    else:
        avgloss = criterion(outputs, target)
    avgloss.backward()
    return avgloss


def _head_train_context(model, criterion, target):
    """The engine's HeadTrainContext when the step qualifies for one launch per head (forward, loss gradient and backward
    together: ops.head_train), else None: exactly this package's FocalLoss_BCE_2d -- a subclass with a forward of its own,
    a hooked criterion or ignore_negative computes something else -- on an fp32 GPU target that needs no gradient, and a
    UNet_Nested in training mode with fp32 storage."""
    from . import engine
    from .losses import FocalLoss_BCE_2d
    from .unet import UNet_Nested
    if not (_FUSED_HEAD_TRAIN and _FUSED_HEAD_LOSS and torch.is_grad_enabled()):
        return None
    c = type(criterion)
    if not (isinstance(criterion, FocalLoss_BCE_2d) and c.forward is FocalLoss_BCE_2d.forward
            and c.mean_over_heads is FocalLoss_BCE_2d.mean_over_heads and c.__call__ is torch.nn.Module.__call__
            and not criterion._forward_hooks and not criterion._forward_pre_hooks and not criterion.ignore_negative):
        return None
    if not (type(model).forward is UNet_Nested.forward and type(model).forward_pruned is UNet_Nested.forward_pruned
            and not model._forward_hooks and not model._forward_pre_hooks
            and model.training and getattr(model, "activation_dtype", torch.float32) == torch.float32):
        return None
    if not (torch.is_tensor(target) and target.is_cuda and target.dtype == torch.float32 and not target.requires_grad
            and target.dim() == 4 and target.is_contiguous()):
        return None
    return engine.HeadTrainContext(target, criterion.gamma, criterion.size_average)


_ZERO = {}   # device -> a 0-dim zero: the stand-in for output gradients a backward does not read


def forward_loss_backward(model, criterion, inputs, target, head=None):
    """forward -> criterion on every head -> mean over heads -> backward (the loop body between zero_grad and the optimizer)
    -> (outputs, mean loss).  When the step qualifies (_head_train_context) every head's forward, loss gradient and
    backward are one launch inside the forward pass; the loss value is the fused loss launch without gradients, and the
    network's backward starts from what the forward kept.  Same bits as the written-out sequence either way."""
    ctx = _head_train_context(model, criterion, target)
    if ctx is None:
        outputs = model(inputs) if head is None else model.forward_pruned(inputs, head)
        return outputs, loss_and_backward(criterion, outputs, target)
    with ctx:
        outputs = model(inputs) if head is None else model.forward_pruned(inputs, head)
    if not ctx.used:
        return outputs, loss_and_backward(criterion, outputs, target)
    from . import ops
    with torch.no_grad():
        if len(outputs) >= 2:    # (the head counts mean_over_heads takes; the engine never runs more than MAX_HEADS)
            rows = target.numel() if criterion.size_average else target.shape[0] * target.shape[1]
            avgloss = ops.focal_bce_heads([o.detach() for o in outputs], target, rows, float(criterion.gamma),
                                          want_grad=False)[0][0]
        else:                    # one head: the loop as written
            avgloss = 0
            for output in outputs:
                avgloss = avgloss + criterion(output.detach(), target)
            avgloss = 1.0 * avgloss / len(outputs)
    zero = _ZERO.get(target.device)
    if zero is None:
        zero = _ZERO[target.device] = torch.zeros((), dtype=torch.float32, device=target.device)
    torch.autograd.backward(list(outputs), [zero.expand_as(o) for o in outputs])
    return outputs, avgloss


def train_step(model, optimizer, criterion, inputs, target, head=None):
    """head = J: the step of the network cut at deep-supervision head J (``UNet_Nested.forward_pruned``) -- the loss is the
    mean over heads 1 .. J, only the cut's nodes run and only its parameters get gradients."""
    optimizer.zero_grad()
    outputs, avgloss = forward_loss_backward(model, criterion, inputs, target, head)
    optimizer.step()
    return outputs, avgloss
