"""Criterion of the training step.

Mirror of ``FocalLoss_BCE_2d`` (/root/reference/tools/losses/focal_loss.py:255-301) as used by the trainer
(trainer/trainer.py:426-427: gamma=3, size_average=False).  The reference moves the head outputs to the CPU for the
loss every step (trainer/trainer.py:122-135, with a "put on GPU" TODO); here GPU tensors take one fused HIP kernel
that produces the loss value and d loss / d pred together (csrc/caller.hip), so backward is a single
scaling.  CPU tensors (host-side tests of the multi-process logic) take the same arithmetic as plain torch ops.
"""
import torch
from torch import nn


class _FusedLossFn(torch.autograd.Function):
    """One map through a fused loss call: ``call(pred, target, want_grad)`` -> (the 0-dim loss, d loss / d pred or None,
    a tuple of further outputs without a gradient).  The gradient comes with the value, so backward is one scaling."""

    @staticmethod
    def forward(ctx, pred, target, call):
        loss, grad, extras = call(pred.contiguous(), target.contiguous(), ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(*extras)
        return (loss,) + tuple(extras)

    @staticmethod
    def backward(ctx, g, *_g_extras):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None, None


def _one_head(loss, grads, *extras):
    """the results of an ops.*_heads call over one head, as _FusedLossFn's call returns them"""
    return loss[0], (grads[0] if grads is not None else None), extras


def _fused_map_ok(input, target):
    """One map and its target take the fused call: GPU fp32, and the target needs no gradient."""
    return (input.is_cuda and target.is_cuda and input.dtype == torch.float32 and target.dtype == torch.float32
            and not target.requires_grad)


def _fused_heads_ok(outputs, target, min_heads=2, any_rank=False):
    """The head outputs and their target take the fused call over all heads: ``min_heads`` to ``MAX_HEADS`` contiguous
    GPU fp32 maps of the target's shape on its device, a target that needs no gradient and is [N, C, H, W] (any_rank:
    the caller has checked the rank itself)."""
    from . import _lib
    if not (isinstance(outputs, (tuple, list)) and min_heads <= len(outputs) <= _lib.MAX_HEADS):
        return False
    if not (target.is_cuda and target.dtype == torch.float32 and not target.requires_grad
            and (any_rank or target.dim() == 4)):
        return False
    return all(o.is_cuda and o.dtype == torch.float32 and o.shape == target.shape and o.is_contiguous()
               and o.device == target.device for o in outputs)


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
        if _fused_map_ok(input, target):
            from . import ops
            rows = input.numel() if self.size_average else samples_num  # mean over elements / sum over N*C rows
            gamma = float(self.gamma)
            if self.ignore_negative:   # (the one-head value of unetpp_focal_bce_heads_ignore)
                call = lambda p, t, want: _one_head(*ops.focal_bce_heads([p], t, rows, gamma, want_grad=want, ignore=True))
            else:
                call = lambda p, t, want: ops.focal_bce(p, t, rows, gamma, want_grad=want) + ((),)
            return _FusedLossFn.apply(input, target, call)[0]
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
        from . import ops
        if not _fused_heads_ok(outputs, target):
            return None
        t = target.contiguous()
        rows = t.numel() if self.size_average else t.shape[0] * t.shape[1]
        loss, grads = ops.focal_bce_heads([o.detach() for o in outputs], t, rows, float(self.gamma),
                                          ignore=self.ignore_negative)
        return loss[0], grads


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
        if _fused_map_ok(input, target):
            from . import ops
            gamma, ignore = float(self.gamma), self.ignore_negative

            def call(p, t, want):
                loss, grads, kth = ops.topk_focal_heads([p], t, k_eff, denom, gamma, want_grad=want, ignore=ignore)
                return _one_head(loss, grads, kth[0])
            loss, self.last_threshold = _FusedLossFn.apply(input, target, call)
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
        from . import ops
        if not _fused_heads_ok(outputs, target):
            return None
        t = target.contiguous()
        rows, pixels = t.shape[0] * t.shape[1], t.shape[2] * t.shape[3]
        k_eff = self.k_for(pixels)
        loss, grads, kth = ops.topk_focal_heads([o.detach() for o in outputs], t, k_eff, self._denom(rows, k_eff),
                                                float(self.gamma), ignore=self.ignore_negative)
        self.last_threshold = kth
        return loss[0], grads


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
        if _fused_map_ok(input, target):
            from . import ops
            call = lambda p, t, want: _one_head(*ops.pr_focal_heads([p], t, self.alpha, self.beta, self.eps, self.positive,
                                                                    want_grad=want, ignore=self.ignore_negative))
            loss, self.last_num_positives = _FusedLossFn.apply(input, target, call)
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
        from . import ops
        if not _fused_heads_ok(outputs, target):
            return None
        loss, grads, n_pos = ops.pr_focal_heads([o.detach() for o in outputs], target.contiguous(), self.alpha, self.beta,
                                                self.eps, self.positive, ignore=self.ignore_negative)
        self.last_num_positives = n_pos
        return loss[0], grads


class _HeadDistillFn(torch.autograd.Function):
    """``HeadDistillLoss.heads_loss``: the value and every head's gradient come from one call; backward scales them."""

    @staticmethod
    def forward(ctx, criterion, target, *outputs):
        avg, grads = criterion.mean_over_heads(tuple(o.detach() for o in outputs), target)
        ctx.save_for_backward(*grads)
        return avg.clone()

    @staticmethod
    def backward(ctx, g):
        return (None, None) + tuple(grad * g for grad in ctx.saved_tensors)


class HeadDistillLoss(nn.Module):
    """Self-distillation across the deep-supervision heads: every head is trained against the labels as
    ``FocalLoss_BCE_2d`` trains it, and every head but the deepest also against a deeper head's map -- its teacher, used
    detached: no gradient reaches a head through its role as teacher.  For heads p_1 .. p_J (a tuple, shallow to deep,
    as ``forward`` and ``forward_pruned`` of the network return them) and the target t:

        teacher="last":  T(j) = J for j < J;   teacher="next":  T(j) = j + 1 for j < J;   head J has no teacher;
        S_j = FocalLoss_BCE_2d(gamma, size_average, ignore_negative)(p_j, t);
        D_j = the FocalLoss_BCE_2d(gamma, size_average) sum of p_j against p_T(j) over the admitted elements, divided by
              S_j's divisor;  D_J = +0.0;
        L_j = S_j + weight * D_j;   loss = the trainer's mean over heads of L_j.

    gate="teacher_better" admits an element only where the teacher is closer to the target than the student,
    ``|q - t| < |p - t|`` on the float32 differences; a NaN on either side keeps the element out.  With
    ``ignore_negative`` an element with ``t < 0`` has a supervised term and gradient of +0.0 as in ``FocalLoss_BCE_2d``,
    counts as having passed the gate, and keeps its distillation term when ``distill_ignored`` (the only training signal
    inside an ignore region) or is kept out when not.

    ``weight`` (finite, >= 0) lives in a one-element float32 tensor per device, created on first use, which the kernel
    reads: ``set_weight(w)`` changes it with a ``fill_``, so a captured ``GraphedTrainStep`` follows a warm-up schedule of
    the weight without a new capture.

    ``forward(input, target)`` takes ONE map, which has no teacher: it returns ``FocalLoss_BCE_2d``'s value with the same
    bits, so a per-head loop (``validate_step``, a ``no_grad`` report) shows the supervised loss.  The distillation term
    exists only over the tuple of heads: ``mean_over_heads`` (what ``train_step`` and ``GraphedTrainStep`` call) and
    ``heads_loss``.  GPU fp32 heads take one fused HIP call (csrc/distill.hip: every map read once, value and gradients
    together); anything else the same rule as plain torch ops.  After a call over the heads ``last_supervised`` and
    ``last_distill`` hold S_j and D_j as [heads] tensors on the device of the target; the class never reads them back.

    Deliberately not a subclass of ``FocalLoss_BCE_2d``: code that tests for that class computes the loss without the
    distillation term."""

    def __init__(self, weight=0.5, teacher="last", gate="none", distill_ignored=True, gamma=3, size_average=False,
                 ignore_negative=False):
        super().__init__()
        if teacher not in ("last", "next"):
            raise ValueError("teacher must be 'last' or 'next', got %r" % (teacher,))
        if gate not in ("none", "teacher_better"):
            raise ValueError("gate must be 'none' or 'teacher_better', got %r" % (gate,))
        if not float(gamma) >= 0.0:
            raise ValueError("gamma must be >= 0, got %r" % (gamma,))
        self.teacher, self.gate = teacher, gate
        self.distill_ignored = bool(distill_ignored)
        self.gamma = gamma
        self.size_average = size_average
        self.ignore_negative = bool(ignore_negative)
        self._supervised = FocalLoss_BCE_2d(gamma=gamma, size_average=size_average, ignore_negative=ignore_negative)
        self._weight_dev = {}   # device -> the one-element float32 tensor the kernel reads
        self.weight = self._checked_weight(weight)
        self.last_supervised = None
        self.last_distill = None

    @staticmethod
    def _checked_weight(w):
        if isinstance(w, bool) or torch.is_tensor(w):
            raise TypeError("weight must be a Python number (the class keeps the device tensor itself)")
        w32 = float(torch.tensor(float(w), dtype=torch.float32))
        if not 0.0 <= w32 < float("inf"):
            raise ValueError("weight must be a finite float32 >= 0, got %r" % (w,))
        return w32

    def set_weight(self, w):
        """The weight of the distillation term from now on: a ``fill_`` of the device tensors, no host synchronisation;
        a captured step reads the new value at its next replay."""
        self.weight = self._checked_weight(w)
        for t in self._weight_dev.values():
            t.fill_(self.weight)

    def weight_tensor(self, device):
        """the one-element float32 tensor on `device` that holds the weight (created on first use)"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = self._weight_dev.get(device)
        if t is None:
            t = self._weight_dev[device] = torch.full((1,), self.weight, dtype=torch.float32, device=device)
        return t

    def forward(self, input, target):
        return self._supervised(input, target)

    def _teacher_of(self, j, heads):
        return heads - 1 if self.teacher == "last" else j + 1

    def _rule(self, outputs, target):
        """the rule as plain torch ops -> (avg with a graph, S [heads], D [heads])"""
        heads = len(outputs)
        dtype = outputs[0].dtype
        rows = target.numel() if self.size_average else target.numel() // (target.size(-2) * target.size(-1))
        w = self.weight_tensor(target.device)[0].to(dtype)
        ignored = (target < 0) if self.ignore_negative else None
        sup, dis = [], []
        avg = 0
        for j, p in enumerate(outputs):
            s = self._supervised(p, target)
            if j < heads - 1:
                q = outputs[self._teacher_of(j, heads)].detach()
                admit = torch.ones_like(target, dtype=torch.bool)
                if self.gate == "teacher_better":
                    admit = (q - target).abs() < (p.detach() - target).abs()
                if ignored is not None:
                    admit = torch.where(ignored, torch.full_like(admit, self.distill_ignored), admit)
                # (finite operands under an element that is kept out: autograd's 0 * NaN through where is a NaN)
                d = torch.where(admit, p - q, torch.full_like(p, 0.5))
                error = 1 - torch.abs(d) + 1e-20
                term = -1 * (1 - error) ** self.gamma * torch.log(error)
                dj = torch.where(admit, term, torch.zeros_like(term)).sum() / rows
            else:
                dj = torch.zeros((), dtype=dtype, device=target.device)
            sup.append(s.detach())
            dis.append(dj.detach())
            avg = avg + (s + w * dj)
        avg = 1.0 * avg / heads
        return avg, torch.stack(sup), torch.stack(dis)

    def _check_heads(self, outputs, target):
        from . import _lib
        if not isinstance(outputs, (tuple, list)) or not 1 <= len(outputs) <= _lib.MAX_HEADS:
            raise ValueError("HeadDistillLoss takes a tuple of 1 to %d heads" % _lib.MAX_HEADS)
        if target.dim() < 3:
            raise ValueError("target must be [..., H, W]")
        for o in outputs:
            if o.shape != target.shape:
                raise ValueError("every head must have the shape of the target")

    def mean_over_heads(self, outputs, target):
        """The loss over the tuple of heads and its gradients in one call -> (avg: 0-dim tensor without a graph,
        [d avg / d output]) for 1 to ``MAX_HEADS`` heads; more raise.  Fp32 contiguous GPU heads take the fused launch;
        anything else the same rule as torch ops with the gradients from ``torch.autograd.grad``.  Never None: the
        written-out loop the caller would fall back to calls ``forward`` per head and would train without the
        distillation term."""
        from . import ops
        self._check_heads(outputs, target)
        if _fused_heads_ok(outputs, target, min_heads=1, any_rank=True):
            t = target.contiguous()
            rows = t.numel() if self.size_average else t.numel() // (t.size(-2) * t.size(-1))
            loss, grads, sup, dis = ops.distill_heads([o.detach() for o in outputs], t, rows, float(self.gamma),
                                                      self.weight_tensor(t.device), self.teacher, self.gate,
                                                      ignore=self.ignore_negative, distill_ignored=self.distill_ignored)
            self.last_supervised, self.last_distill = sup, dis
            return loss[0], grads
        with torch.enable_grad():
            leaves = [o.detach().requires_grad_(True) for o in outputs]
            avg, sup, dis = self._rule(leaves, target.detach())
            grads = torch.autograd.grad(avg, leaves)
        self.last_supervised, self.last_distill = sup, dis
        return avg.detach(), list(grads)

    def heads_loss(self, outputs, target):
        """The loss over the tuple of heads as a differentiable 0-dim tensor, for callers that do not go through
        ``train_step``: one autograd node whose backward is one scaling of the gradients ``mean_over_heads`` produced."""
        self._check_heads(outputs, target)
        return _HeadDistillFn.apply(self, target, *outputs)


class TeacherDistillLoss(nn.Module):
    """Distillation from an external teacher: every head, the deepest included, is trained against the labels as
    ``FocalLoss_BCE_2d`` trains it and against ONE map from outside -- another network's output, a stitched
    ``SceneInference`` map cut by ``SceneCrops(teacher=...)``, ``infer_mc``'s mean -- set with ``set_teacher`` and read as
    data.  For heads p_1 .. p_J (a tuple, shallow to deep), the target t and the teacher's map q:

        S_j = FocalLoss_BCE_2d(gamma, size_average, ignore_negative)(p_j, t);
        D_j = the FocalLoss_BCE_2d(gamma, size_average) sum of p_j against q over the admitted elements, divided by
              S_j's divisor;
        L_j = S_j + weight * D_j;   loss = the trainer's mean over heads of L_j.

    An element is admitted where the teacher exists -- ``q < 0`` means "no teacher here" (-0.0 and a NaN are not
    negative: a NaN of the teacher reaches the loss), so the -1 that fills a cut window outside its frame keeps the term
    out -- and where the gate and the ignore rule of ``HeadDistillLoss`` admit it: gate="teacher_better" asks
    ``|q - t| < |p - t|`` on the float32 differences (a NaN on either side keeps the element out); with
    ``ignore_negative`` an element with ``t < 0`` has a supervised term and gradient of +0.0, counts as having passed
    the gate, and keeps its distillation term when ``distill_ignored`` (a frame under one whole-frame ignore rectangle
    then trains on the teacher alone) or is kept out when not.

    ``set_teacher(maps)`` copies a float32 tensor of the target's shape into a buffer the class keeps per (device,
    shape): the first call allocates it, every later call with the same device and shape is a ``copy_`` into the same
    memory without a host synchronisation, so a captured ``GraphedTrainStep`` follows the teacher of each step without a
    new capture, as it follows ``set_weight``.  A new shape or device allocates a new buffer, and a step captured before
    does not see it: capture again.  ``mean_over_heads`` raises when no teacher is set for the target's device and
    shape -- training silently without the term is what the class exists to prevent.

    ``forward(input, target)`` takes ONE map and returns ``FocalLoss_BCE_2d``'s value with the same bits, so a per-head
    loop (``validate_step``, a ``no_grad`` report) shows the supervised loss.  GPU fp32 heads take one fused HIP call
    (csrc/distill.hip: unetpp_teacher_heads, 2 + 2 J map-sized streams); anything else the same rule as plain torch ops.
    ``last_supervised`` and ``last_distill`` hold S_j and D_j as [heads] tensors on the device of the target.

    Deliberately not a subclass of ``FocalLoss_BCE_2d``: code that tests for that class computes the loss without the
    distillation term."""

    def __init__(self, weight=0.5, gate="none", distill_ignored=True, gamma=3, size_average=False, ignore_negative=False):
        super().__init__()
        if gate not in ("none", "teacher_better"):
            raise ValueError("gate must be 'none' or 'teacher_better', got %r" % (gate,))
        if not float(gamma) >= 0.0:
            raise ValueError("gamma must be >= 0, got %r" % (gamma,))
        self.gate = gate
        self.distill_ignored = bool(distill_ignored)
        self.gamma = gamma
        self.size_average = size_average
        self.ignore_negative = bool(ignore_negative)
        self._supervised = FocalLoss_BCE_2d(gamma=gamma, size_average=size_average, ignore_negative=ignore_negative)
        self._weight_dev = {}   # device -> the one-element float32 tensor the kernel reads
        self._teacher = {}      # (device, shape) -> the buffer the kernel reads
        self.weight = self._checked_weight(weight)
        self.last_supervised = None
        self.last_distill = None

    _checked_weight = staticmethod(HeadDistillLoss._checked_weight)
    set_weight = HeadDistillLoss.set_weight
    weight_tensor = HeadDistillLoss.weight_tensor

    @staticmethod
    def _device(device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return device

    def set_teacher(self, maps):
        """The teacher's maps from now on for targets of ``maps``' device and shape: float32, used detached.  The first
        call for a (device, shape) allocates a private buffer; every later one is a ``copy_`` into it (same
        ``data_ptr()``, no host synchronisation), which a captured step reads at its next replay.  A new shape or device
        allocates anew: a step captured before needs a new capture.  -> the buffer."""
        if not torch.is_tensor(maps):
            raise TypeError("the teacher's maps must be a tensor")
        if maps.dtype != torch.float32:
            raise TypeError("the teacher's maps must be torch.float32, got %s" % maps.dtype)
        if maps.dim() < 3:
            raise ValueError("the teacher's maps must be [..., H, W]")
        key = (self._device(maps.device), tuple(maps.shape))
        buf = self._teacher.get(key)
        if buf is None:
            buf = self._teacher[key] = torch.empty(key[1], dtype=torch.float32, device=key[0])
        buf.copy_(maps.detach())
        return buf

    def clear_teacher(self):
        """forget every teacher buffer"""
        self._teacher.clear()

    def teacher_tensor(self, target):
        """the buffer ``set_teacher`` filled for ``target``'s device and shape; RuntimeError when there is none"""
        buf = self._teacher.get((self._device(target.device), tuple(target.shape)))
        if buf is None:
            raise RuntimeError("TeacherDistillLoss: no teacher set for a target of shape %s on %s (set_teacher first)"
                               % (tuple(target.shape), target.device))
        return buf

    def forward(self, input, target):
        return self._supervised(input, target)

    def _rule(self, outputs, target, teacher=None):
        """the rule as plain torch ops -> (avg with a graph, S [heads], D [heads])"""
        heads = len(outputs)
        dtype = outputs[0].dtype
        rows = target.numel() if self.size_average else target.numel() // (target.size(-2) * target.size(-1))
        w = self.weight_tensor(target.device)[0].to(dtype)
        q = (self.teacher_tensor(target) if teacher is None else teacher).detach()
        exists = ~(q < 0)
        q = q.to(dtype)
        ignored = (target < 0) if self.ignore_negative else None
        sup, dis = [], []
        avg = 0
        for p in outputs:
            s = self._supervised(p, target)
            admit = torch.ones_like(target, dtype=torch.bool)
            if self.gate == "teacher_better":
                admit = (q - target).abs() < (p.detach() - target).abs()
            if ignored is not None:
                admit = torch.where(ignored, torch.full_like(admit, self.distill_ignored), admit)
            admit = admit & exists
            # (finite operands under an element that is kept out: autograd's 0 * NaN through where is a NaN)
            d = torch.where(admit, p - q, torch.full_like(p, 0.5))
            error = 1 - torch.abs(d) + 1e-20
            term = -1 * (1 - error) ** self.gamma * torch.log(error)
            dj = torch.where(admit, term, torch.zeros_like(term)).sum() / rows
            sup.append(s.detach())
            dis.append(dj.detach())
            avg = avg + (s + w * dj)
        avg = 1.0 * avg / heads
        return avg, torch.stack(sup), torch.stack(dis)

    def _check_heads(self, outputs, target):
        from . import _lib
        if not isinstance(outputs, (tuple, list)) or not 1 <= len(outputs) <= _lib.MAX_HEADS:
            raise ValueError("TeacherDistillLoss takes a tuple of 1 to %d heads" % _lib.MAX_HEADS)
        if target.dim() < 3:
            raise ValueError("target must be [..., H, W]")
        for o in outputs:
            if o.shape != target.shape:
                raise ValueError("every head must have the shape of the target")

    def mean_over_heads(self, outputs, target):
        """The loss over the tuple of heads and its gradients in one call -> (avg: 0-dim tensor without a graph,
        [d avg / d output]) for 1 to ``MAX_HEADS`` heads; more raise, and so does a target for whose device and shape no
        teacher is set.  Fp32 contiguous GPU heads take the fused launch; anything else the same rule as torch ops with
        the gradients from ``torch.autograd.grad``.  Never None: the written-out loop the caller would fall back to
        calls ``forward`` per head and would train without the distillation term."""
        from . import ops
        self._check_heads(outputs, target)
        teacher = self.teacher_tensor(target)
        if _fused_heads_ok(outputs, target, min_heads=1, any_rank=True):
            t = target.contiguous()
            rows = t.numel() if self.size_average else t.numel() // (t.size(-2) * t.size(-1))
            loss, grads, sup, dis = ops.teacher_heads([o.detach() for o in outputs], t, teacher, rows, float(self.gamma),
                                                      self.weight_tensor(t.device), self.gate,
                                                      ignore=self.ignore_negative, distill_ignored=self.distill_ignored)
            self.last_supervised, self.last_distill = sup, dis
            return loss[0], grads
        with torch.enable_grad():
            leaves = [o.detach().requires_grad_(True) for o in outputs]
            avg, sup, dis = self._rule(leaves, target.detach(), teacher)
            grads = torch.autograd.grad(avg, leaves)
        self.last_supervised, self.last_distill = sup, dis
        return avg.detach(), list(grads)

    def heads_loss(self, outputs, target):
        """The loss over the tuple of heads as a differentiable 0-dim tensor, for callers that do not go through
        ``train_step``: one autograd node whose backward is one scaling of the gradients ``mean_over_heads`` produced."""
        self._check_heads(outputs, target)
        return _HeadDistillFn.apply(self, target, *outputs)
