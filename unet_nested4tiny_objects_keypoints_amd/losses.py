"""Criterion of the training step.

Mirror of ``FocalLoss_BCE_2d`` (/root/reference/tools/losses/focal_loss.py:255-301) as used by the trainer
(trainer/trainer.py:426-427: gamma=3, size_average=False).  The reference moves the head outputs to the CPU for the
loss every step (trainer/trainer.py:122-135, with a "put on GPU" TODO); here GPU tensors take one fused HIP kernel
that produces the loss value and d loss / d pred together (csrc/caller.hip), so backward is a single
scaling.  CPU tensors (host-side tests of the multi-process logic) take the same arithmetic as plain torch ops.
"""
import torch
from torch import nn


class _FocalBCEIgnoreFn(torch.autograd.Function):
    """The one-head ``mean_over_heads`` value of a criterion with ignore_negative (unetpp_focal_bce_heads_ignore)."""

    @staticmethod
    def forward(ctx, pred, target, rows, gamma):
        from . import ops
        loss, grads = ops.focal_bce_heads([pred.contiguous()], target.contiguous(), rows, gamma,
                                          want_grad=ctx.needs_input_grad[0], ignore=True)
        ctx.save_for_backward(grads[0] if grads is not None else None)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None, None, None


class _FocalBCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, rows, gamma):
        from . import ops
        loss, grad = ops.focal_bce(pred.contiguous(), target.contiguous(), rows, gamma, want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None, None, None


class FocalLoss_BCE_2d(nn.Module):
    """ignore_negative: an element whose target is negative (``target < 0``: -0.0 and a NaN are not) is ignored -- its
    term and its gradient are +0.0 whatever the input holds; the divisor stays what it is without."""

    def __init__(self, gamma=3, alpha=0.25, size_average=False, ignore_negative=False):
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha  # kept for signature parity; the reference never uses it in forward
        self.size_average = size_average
        self.ignore_negative = bool(ignore_negative)

    def forward(self, input, target):
        if input.dim() > 2:
            input = input.reshape(-1, input.size(2), input.size(3))
        target = target.reshape(-1, target.size(2), target.size(3))
        samples_num = target.shape[0]
        if (input.is_cuda and target.is_cuda and input.dtype == torch.float32 and target.dtype == torch.float32
                and not target.requires_grad):
            rows = input.numel() if self.size_average else samples_num  # mean over elements / sum over N*C rows
            fn = _FocalBCEIgnoreFn if self.ignore_negative else _FocalBCEFn
            return fn.apply(input, target, rows, float(self.gamma))
        d = input - target
        if self.ignore_negative:   # (d = 0 under an ignored element as well: autograd's 0 * NaN through where is a NaN)
            d = torch.where(target < 0, torch.zeros_like(d), d)
        error = 1 - torch.abs(d) + 1e-20
        loss = -1 * (1 - error) ** self.gamma * torch.log(error)
        if self.ignore_negative:
            loss = torch.where(target < 0, torch.zeros_like(loss), loss)
        if self.size_average:
            return loss.mean()
        return loss.sum() / samples_num

    def mean_over_heads(self, outputs, target):
        """The trainer's loop over the deep-supervision heads (trainer/trainer.py:122-135) -- ``avg = 0; avg = avg +
        criterion(o, target) for o in outputs; avg = 1.0 * avg / len(outputs)`` -- in ONE launch, value and gradients
        together: -> (avg: 0-dim tensor without a graph, [d avg / d output]) or None when the heads do not qualify (CPU
        tensors, other dtypes or layouts, more than 8 heads, a target that needs a gradient): the caller then runs the loop.
        Same bits as the loop (tests/test_gpu_caller.py); about 15 launches of ~5 us fewer per step at three or four heads."""
        from . import _lib, ops
        if not (isinstance(outputs, (tuple, list)) and 2 <= len(outputs) <= _lib.MAX_HEADS):
            return None
        if not (target.is_cuda and target.dtype == torch.float32 and not target.requires_grad and target.dim() == 4):
            return None
        for o in outputs:
            if not (o.is_cuda and o.dtype == torch.float32 and o.shape == target.shape and o.is_contiguous()
                    and o.device == target.device):
                return None
        t = target.contiguous()
        rows = t.numel() if self.size_average else t.shape[0] * t.shape[1]
        loss, grads = ops.focal_bce_heads([o.detach() for o in outputs], t, rows, float(self.gamma),
                                          ignore=self.ignore_negative)
        return loss[0], grads


class _TopKFocalBCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, k, denom, gamma, ignore=False):
        from . import ops
        loss, grads, kth = ops.topk_focal_heads([pred.contiguous()], target.contiguous(), k, denom, gamma,
                                                want_grad=ctx.needs_input_grad[0], ignore=ignore)
        ctx.save_for_backward(grads[0] if grads is not None else None)
        kth = kth[0]
        ctx.mark_non_differentiable(kth)
        return loss[0], kth

    @staticmethod
    def backward(ctx, g, _g_kth):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None, None, None, None, None


class TopKFocalLoss_BCE_2d(nn.Module):
    """Hard-pixel mining for ``FocalLoss_BCE_2d``: of every (n, c) map only the ``k`` pixels with the largest
    ``|input - target|`` -- the largest loss terms, the ranking of the reference's ``BCE_loss(results, labels, topk)``
    (tools/losses/bce_loss.py:14-35) -- enter the loss; pixels equal to the k-th largest are taken in index order, so a
    step stays bit-reproducible.  Exactly one of ``k`` (pixels per map, >= 1) and ``fraction`` (of the map's P = H*W
    pixels, in (0, 1]: k = max(1, ceil(fraction * P))) is given; k >= P is ``FocalLoss_BCE_2d`` itself.
    ``size_average=False`` divides the sum by the N*C maps (the ``FocalLoss_BCE_2d`` convention), ``True`` by the number
    of selected pixels as well.  GPU fp32 tensors take one fused HIP launch (csrc/topk_loss.hip: an exact radix select,
    value and gradient together); CPU tensors the same rule as plain torch ops.  After a call ``last_threshold`` holds the
    k-th largest ``|input - target|`` of every map: [N*C] after ``forward``, [heads, N*C] after ``mean_over_heads``.

    ignore_negative: an element whose target is negative (``target < 0``: -0.0 and a NaN are not) ranks as
    ``|input - target| = 0`` -- last -- and contributes +0.0 to the loss and the gradient whether selected or not; k and
    the divisor stay what they are without.

    Deliberately not a subclass of ``FocalLoss_BCE_2d``: code that tests for that class computes the unselected loss."""

    def __init__(self, k=None, fraction=None, gamma=3, size_average=False, ignore_negative=False):
        super().__init__()
        self.ignore_negative = bool(ignore_negative)
        if (k is None) == (fraction is None):
            raise ValueError("give exactly one of k and fraction")
        if k is not None:
            if isinstance(k, bool) or int(k) != k or int(k) < 1:
                raise ValueError("k must be an integer >= 1, got %r" % (k,))
            k = int(k)
        else:
            fraction = float(fraction)
            if not 0.0 < fraction <= 1.0:
                raise ValueError("fraction must be in (0, 1], got %r" % (fraction,))
        self.k = k
        self.fraction = fraction
        self.gamma = gamma
        self.size_average = size_average
        self.last_threshold = None

    def k_for(self, pixels: int) -> int:
        """the pixels selected of a map of `pixels` pixels"""
        import math
        k = self.k if self.k is not None else max(1, math.ceil(self.fraction * pixels))
        return min(k, pixels)

    def _denom(self, rows, k_eff):
        return rows * k_eff if self.size_average else rows

    def forward(self, input, target):
        if input.dim() > 2:
            input = input.reshape(-1, input.size(-2), input.size(-1))
        target = target.reshape(-1, target.size(-2), target.size(-1))
        rows, pixels = target.shape[0], target.shape[1] * target.shape[2]
        k_eff = self.k_for(pixels)
        denom = self._denom(rows, k_eff)
        if (input.is_cuda and target.is_cuda and input.dtype == torch.float32 and target.dtype == torch.float32
                and not target.requires_grad):
            loss, kth = _TopKFocalBCEFn.apply(input, target, k_eff, denom, float(self.gamma), self.ignore_negative)
            self.last_threshold = kth
            return loss
        d = (input - target).reshape(rows, pixels)
        ignored = target.reshape(rows, pixels) < 0 if self.ignore_negative else None
        if ignored is not None:   # key 0, and no NaN reaches autograd through the where below
            d = torch.where(ignored, torch.zeros_like(d), d)
        key = d.detach().abs()
        # descending and stable: the lowest index first among equals (a NaN sorts first, as in the kernel)
        ranked, order = torch.sort(key, dim=1, descending=True, stable=True)
        selected = torch.zeros(rows, pixels, dtype=torch.bool).scatter_(1, order[:, :k_eff], True)
        self.last_threshold = ranked[:, k_eff - 1]
        error = 1 - torch.abs(d) + 1e-20
        loss = -1 * (1 - error) ** self.gamma * torch.log(error)
        if ignored is not None:
            selected = selected & ~ignored
        return torch.where(selected, loss, torch.zeros_like(loss)).sum() / denom

    def mean_over_heads(self, outputs, target):
        """``FocalLoss_BCE_2d.mean_over_heads`` for this criterion: the trainer's loop over the deep-supervision heads in
        ONE launch, the selection taken per head -> (avg: 0-dim tensor without a graph, [d avg / d output]) or None when
        the heads do not qualify; the caller then runs the loop.  Same bits as the loop (tests/test_gpu_topk.py)."""
        from . import _lib, ops
        if not (isinstance(outputs, (tuple, list)) and 2 <= len(outputs) <= _lib.MAX_HEADS):
            return None
        if not (target.is_cuda and target.dtype == torch.float32 and not target.requires_grad and target.dim() == 4):
            return None
        for o in outputs:
            if not (o.is_cuda and o.dtype == torch.float32 and o.shape == target.shape and o.is_contiguous()
                    and o.device == target.device):
                return None
        t = target.contiguous()
        rows, pixels = t.shape[0] * t.shape[1], t.shape[2] * t.shape[3]
        k_eff = self.k_for(pixels)
        loss, grads, kth = ops.topk_focal_heads([o.detach() for o in outputs], t, k_eff, self._denom(rows, k_eff),
                                                float(self.gamma), ignore=self.ignore_negative)
        self.last_threshold = kth
        return loss[0], grads


class _PRFocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, alpha, beta, eps, positive, ignore=False):
        from . import ops
        loss, grads, n_pos = ops.pr_focal_heads([pred.contiguous()], target.contiguous(), alpha, beta, eps, positive,
                                                want_grad=ctx.needs_input_grad[0], ignore=ignore)
        ctx.save_for_backward(grads[0] if grads is not None else None)
        ctx.mark_non_differentiable(n_pos)
        return loss[0], n_pos

    @staticmethod
    def backward(ctx, g, _g_n_pos):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None, None, None, None, None, None


class PenaltyReducedFocalLoss(nn.Module):
    """The penalty-reduced focal loss of CornerNet / CenterNet for heat maps of sigmoid values, normalised by the number
    of positives.  Per element of ``input`` p and ``target`` t (same shape, t in [0, 1]), in float32:

        lo = float32(eps), hi = float32(1) - lo;  q = clamp(p, lo, hi) (the gradient passes where lo <= p <= hi, as
        ``torch.clamp`` has it, and is exactly 0 elsewhere; a NaN stays a NaN and makes the loss NaN);
        t >= positive:  l = -(1 - q)^alpha log(q);   otherwise:  l = -(1 - t)^beta q^alpha log1p(-q);   0^0 = 1;
        n_pos = the elements with t >= positive, over the whole target;  loss = sum(l) * (1 / max(n_pos, 1)).

    The normaliser belongs to the call, hence to the replica under data parallel.  ``unetpp_points_target`` and
    ``create_heatmap`` write exactly 1.0 at an integer label, so ``positive=1.0`` marks the centres.  A label at a sub-pixel
    position never produces a 1.0: the largest value of ``exp(-0.5 d / radius)`` within half a pixel of it may be as low as
    ``exp(-0.5 * 0.7071 / radius)``, and ``positive=math.exp(-0.5 * 0.7071 / radius)`` takes the nearest pixel (and, close
    to a pixel centre, its neighbours) for such targets.

    GPU fp32 tensors take one fused HIP call (csrc/pr_focal.hip: value and gradient together, backward is one scaling);
    anything else the same rule as plain torch ops.  After a call ``last_num_positives`` holds n_pos as a 0-dim int64
    tensor on the device of the target; the class never reads it back.

    ignore_negative: an element whose target is negative (``target < 0``: -0.0 and a NaN are not) is ignored -- its term
    and its gradient are +0.0 whatever the input holds; n_pos is unchanged (a negative target is never >= positive).

    Deliberately not a subclass of ``FocalLoss_BCE_2d``: code that tests for that class computes another loss."""

    def __init__(self, alpha=2.0, beta=4.0, eps=1e-4, positive=1.0, ignore_negative=False):
        super().__init__()
        self.ignore_negative = bool(ignore_negative)
        alpha, beta, eps, positive = float(alpha), float(beta), float(eps), float(positive)
        if not (0.0 <= alpha < float("inf")) or not (0.0 <= beta < float("inf")):
            raise ValueError("alpha and beta must be finite and >= 0, got %r and %r" % (alpha, beta))
        lo = torch.tensor(eps, dtype=torch.float32)
        if not 0.0 < float(lo) < 0.5:
            raise ValueError("eps must be in (0, 0.5) as a float32, got %r" % (eps,))
        pos32 = float(torch.tensor(positive, dtype=torch.float32))
        if not 0.0 < pos32 <= 1.0:
            raise ValueError("positive must be in (0, 1], got %r" % (positive,))
        self.alpha, self.beta, self.eps, self.positive = alpha, beta, eps, positive
        self._lo = float(lo)
        self._hi = float(torch.tensor(1.0, dtype=torch.float32) - lo)
        self._positive32 = pos32
        self.last_num_positives = None

    def forward(self, input, target):
        if input.shape != target.shape:
            raise ValueError("input and target must have the same shape")
        if (input.is_cuda and target.is_cuda and input.dtype == torch.float32 and target.dtype == torch.float32
                and not target.requires_grad):
            loss, n_pos = _PRFocalFn.apply(input, target, self.alpha, self.beta, self.eps, self.positive,
                                           self.ignore_negative)
            self.last_num_positives = n_pos
            return loss
        q = input.clamp(self._lo, self._hi)
        if self.ignore_negative:   # (finite operands under an ignored element: autograd's 0 * NaN through where is a NaN)
            ignored = target < 0
            q = torch.where(ignored, torch.full_like(q, 0.5), q)
            target = torch.where(ignored, torch.zeros_like(target), target)
        pos = target >= self._positive32
        at_centre = -1 * (1 - q) ** self.alpha * torch.log(q)
        elsewhere = -1 * (1 - target) ** self.beta * q ** self.alpha * torch.log1p(-q)
        n_pos = pos.sum()
        self.last_num_positives = n_pos
        term = torch.where(pos, at_centre, elsewhere)
        if self.ignore_negative:
            term = torch.where(ignored, torch.zeros_like(term), term)
        total = term.sum()
        return total * (1.0 / n_pos.clamp(min=1).to(total.dtype))

    def mean_over_heads(self, outputs, target):
        """``FocalLoss_BCE_2d.mean_over_heads`` for this criterion: the trainer's loop over the deep-supervision heads in
        ONE call, the positives counted once -> (avg: 0-dim tensor without a graph, [d avg / d output]) or None when the
        heads do not qualify; the caller then runs the loop.  Same bits as the loop (tests/test_gpu_prfocal.py)."""
        from . import _lib, ops
        if not (isinstance(outputs, (tuple, list)) and 2 <= len(outputs) <= _lib.MAX_HEADS):
            return None
        if not (target.is_cuda and target.dtype == torch.float32 and not target.requires_grad and target.dim() == 4):
            return None
        for o in outputs:
            if not (o.is_cuda and o.dtype == torch.float32 and o.shape == target.shape and o.is_contiguous()
                    and o.device == target.device):
                return None
        loss, grads, n_pos = ops.pr_focal_heads([o.detach() for o in outputs], target.contiguous(), self.alpha, self.beta,
                                                self.eps, self.positive, ignore=self.ignore_negative)
        self.last_num_positives = n_pos
        return loss[0], grads
