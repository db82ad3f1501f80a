"""The reference trainer's own optimizers with a HIP hot path: one fused launch per ``step()``.

Drop-in for tools/optimizers/{adamw,adabound,sgdw}.py of the reference (trainer/trainer.py:344-379 maps its
``--optimizer`` names adamw / adabound / sgdw to them):

    from unet_nested4tiny_objects_keypoints_amd.optim import AdamW, AdaBound, SGDW

Constructor signatures, defaults, ``ValueError`` checks, param-group keys and (in the default eager mode) the state
format are the reference's: ``state['step']`` is a Python int per parameter beside ``exp_avg`` / ``exp_avg_sq`` /
``max_exp_avg_sq`` or ``momentum_buffer``, so ``.tar`` checkpoints (checkpoint.py) move between these classes and the
reference's in both directions.  Steps are counted per parameter: a parameter whose ``grad`` is None is skipped and its
count does not advance.  ``group['lr']`` is read at every step (LR schedulers work unchanged).

What ``step()`` does on the device (csrc/optim.hip, ``unetpp_optim_step``): every parameter with a gradient is a segment
of one device table (multi_tensor.py; the format and the chunk walk are described in csrc/multi_tensor.h), and one
launch updates them all, element by element in the reference's op order.  The table is built once per set of data
pointers (parameters, their CURRENT gradients, state tensors) and cached, so a gradient buffer that moves (the
data-parallel averager swaps ``p.grad`` between two flat buffers, dp.py) gets its own table.
Eager mode: per step one small host -> device copy (the hyper-parameters and each segment's step count) and one
launch.  The update writes through raw pointers, as the reference writes through ``p.data``: ``p._version`` does not
move (the weight-image pack plan is rebuilt every pass).

``capturable=True``: ``state['step']`` is a float32 device scalar per parameter, the bias corrections and AdaBound's
bounds are formed on the device and the launch itself advances the counters -- no host sync, no host decision on device
data, so ``GraphedTrainStep(..., capture_optimizer=True)`` captures the step.  The hyper-parameters are read from a
small device block: an eager ``step()`` refreshes it, a captured one does not, so after changing ``group['lr']`` (an LR
scheduler) call ``refresh_hyperparameters()`` before the next replay.

Gradient clipping and the non-finite skip (keyword-only ``max_grad_norm=None``, ``skip_nonfinite=False``; optimizer
attributes, not param-group keys, so ``state_dict()`` keeps the reference's format): with either set, ``step()`` is two
launches over the same table.  ``unetpp_grad_norm`` leaves one float64 sum of squares per 4096-element chunk; the update
launch (``unetpp_optim_step_clip``) sums them in a fixed order in every workgroup's prologue, forms torch's
``clip_grad_norm_`` coefficient in fp32 (``c = max_norm / (norm + 1e-6)``, ``min(c, 1)``) over ALL groups' gradients and
multiplies each gradient by it as it is read -- ``p.grad`` is not written.  ``skip_nonfinite=True`` (capturable mode only:
eager mode has advanced ``state['step']`` on the host before the launch) makes a step whose gradients hold an inf or a NaN
store nothing: parameters, moments and step counters stay, ``skipped_steps`` advances.  ``last_grad_norm`` (0-dim float32,
the norm before clipping, overwritten by every step: clone it to keep it) and ``skipped_steps`` (0-dim int32) are device
tensors; reading them is the caller's sync, ``step()`` makes none.  ``opt.max_grad_norm = x`` holds from the next eager
step; a captured step reads it from the device hyper block (``refresh_hyperparameters()``, as for lr).  The defaults
leave the code path, the launch and the results exactly as they were.

``clip_grad_norm_(parameters, max_norm)`` is ``torch.nn.utils.clip_grad_norm_`` for fp32 CUDA gradients as two launches
(norm, in-place scale), for optimizers that are not the three above or for code that wants the clipped gradients.

fp32 CUDA tensors only: anything else raises (this path has no CPU fallback).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch.optim.optimizer import Optimizer, required

from . import _lib
from .multi_tensor import Table, TableCache, aligned16


class _FusedOptimizer(Optimizer):
    """Common host side of the three classes: state bookkeeping, the cached segment table, the launch."""
    _KIND = None
    _AMS_KEY = None          # group key that selects max_exp_avg_sq
    _MOMENTS = True          # exp_avg / exp_avg_sq (AdamW, AdaBound)

    def _init_fused(self, capturable: bool, max_grad_norm=None, skip_nonfinite: bool = False):
        self.capturable = bool(capturable)
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        if self.skip_nonfinite and not self.capturable:
            raise ValueError("skip_nonfinite=True needs capturable=True: eager mode advances state['step'] on the host "
                             "before the launch, and a skip decided on the device cannot take that back without a sync")
        self._clip_dev = None      # device mirror of unetpp_clip_state: total_norm, coef, skipped_steps, reserved
        self._tables = TableCache()
        self._state_epoch = 0
        self._hyper_dev = None
        self._spare_host = None

    # ---- hyper-parameters -------------------------------------------------------------------------------------------
    def _hyper_row(self, gi: int, group) -> list:
        raise NotImplementedError

    def _hyper(self) -> np.ndarray:
        rows = [self._hyper_row(gi, g) for gi, g in enumerate(self.param_groups)]
        h = np.asarray(rows, dtype=np.float64).reshape(-1)
        if self._max_grad_norm is not None:
            h[_lib.OPTIM_H_MAX_NORM] = self._max_grad_norm      # row 0; 0 = no clipping
        return h

    # ---- clipping --------------------------------------------------------------------------------------------------
    @property
    def max_grad_norm(self):
        """Largest global 2-norm of all gradients a step applies (None: no clipping)."""
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        if value is not None:
            value = float(value)
            if not value > 0.0:
                raise ValueError("Invalid max_grad_norm: {}".format(value))
        self._max_grad_norm = value

    def _clip_block(self) -> torch.Tensor:
        if self._clip_dev is None:
            dev = self._device()
            if dev is None or dev.type != "cuda":
                raise RuntimeError("%s parameters must live on the GPU: this path has no CPU fallback" % type(self).__name__)
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("capturable %s: run one eager step() before capturing it" % type(self).__name__)
            self._clip_dev = torch.zeros(4, dtype=torch.float32, device=dev)
        return self._clip_dev

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """0-dim float32 device tensor: the global gradient norm the last clipped step saw, before clipping."""
        return self._clip_block()[0]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """0-dim int32 device tensor: steps that skip_nonfinite left undone."""
        return self._clip_block()[2:3].view(torch.int32)[0]

    def refresh_hyperparameters(self):
        """capturable mode: copy the groups' current hyper-parameters (lr, betas, ...) to the device block the captured
        launch reads.  An eager step() does it itself; call it before graph replays after a scheduler changed lr."""
        if not self.capturable:
            return
        h = self._hyper()
        dev = self._device()
        if dev is None:
            return
        if self._hyper_dev is None or self._hyper_dev.numel() != h.size or self._hyper_dev.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("capturable %s: run one eager step() before capturing it" % type(self).__name__)
            self._hyper_dev = torch.zeros(h.size, dtype=torch.float64, device=dev)
        host = torch.from_numpy(h).pin_memory()
        self._hyper_dev.copy_(host, non_blocking=True)

    def _device(self):
        for g in self.param_groups:
            for p in g["params"]:
                return p.device
        return None

    # ---- state -----------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._state_epoch += 1
        self._tables.clear()
        for st in self.state.values():      # reference checkpoints carry int steps; capturable mode keeps them on the device
            if "step" not in st:
                if self.capturable and "momentum_buffer" in st:     # SGDW's reference state has no count
                    st["step"] = 1
                else:
                    continue
            s = st["step"]
            if self.capturable:
                dev = next((v.device for v in st.values() if torch.is_tensor(v) and v.is_cuda), None)
                if not torch.is_tensor(s) or s.device != dev or s.dtype != torch.float32:
                    st["step"] = torch.tensor(float(s), dtype=torch.float32, device=dev)
            elif torch.is_tensor(s):
                st["step"] = int(s.item())

    # ---- step -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        """Performs a single optimization step (the reference's semantics; see the module docstring)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        rows, ptrs, steps = [], [], []
        capturable = self.capturable
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                t = self._advance(p, group, state)
                rows.append((p, g, state, gi))
                ptrs.append(p.data_ptr())
                ptrs.append(g.data_ptr())
                steps.append(t)
        if not rows:
            return loss
        key = (self._state_epoch, tuple(ptrs))
        table = self._tables.get(key)
        if table is None:
            table = self._tables.add(key, self._build_table(rows))
        else:
            self._tables.move_to_end(key)
        L = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream(table.dev.device).cuda_stream)
        if capturable:
            if not torch.cuda.is_current_stream_capturing():
                self.refresh_hyperparameters()
            elif self._hyper_dev is None:
                raise RuntimeError("capturable %s: run one eager step() before capturing it" % type(self).__name__)
            args = table.args + (C.c_void_p(self._hyper_dev.data_ptr()), None, table.done)
            flags = self._flags() | _lib.OPTIM_CAPTURABLE
        else:
            h = self._hyper()
            if table.rows_used is not None:      # zero-element parameters have no segment, so no count in the block
                steps = [steps[i] for i in table.rows_used]
            host = torch.empty(h.size + len(steps), dtype=torch.float64, pin_memory=True)
            arr = host.numpy()
            arr[:h.size] = h
            arr[h.size:] = steps
            table.block.copy_(host, non_blocking=True)
            blk = table.block.data_ptr()
            args = table.args + (C.c_void_p(blk), C.c_void_p(blk + 8 * h.size), None)
            flags = self._flags()
        if self._max_grad_norm is None and not self.skip_nonfinite:
            _lib.check(L.unetpp_optim_step(self._KIND, flags, *args, stream), "unetpp_optim_step")
            return loss
        # clipped: the norm pass over the same table, then the update that combines its partials in its prologue
        state = self._clip_block()
        if table.partials is None:
            table.partials = torch.empty(table.n_chunks, dtype=torch.float64, device=table.dev.device)
        partials = C.c_void_p(table.partials.data_ptr())
        _lib.check(L.unetpp_grad_norm(*table.args, partials, stream), "unetpp_grad_norm")
        if self.skip_nonfinite:
            flags |= _lib.OPTIM_SKIP_NONFINITE
        _lib.check(L.unetpp_optim_step_clip(self._KIND, flags, *args, partials, C.c_void_p(state.data_ptr()), stream),
                   "unetpp_optim_step_clip")
        return loss

    def _flags(self) -> int:
        return 0

    def _advance(self, p, group, state):
        """Creates missing state and advances the count of this parameter; returns the eager count of this update."""
        raise NotImplementedError

    def _build_table(self, rows) -> Table:
        """The table of this set of tensors, with what a step needs beside it: block (eager: the device block of the
        hyper-parameters and step counts), rows_used (the rows that have a segment, when some have no elements) and
        partials (float64 [n_chunks] of the norm pass, made when a clipped step first needs it)."""
        from .ops import _need
        segs, used = [], []
        for i, (p, g, state, gi) in enumerate(rows):
            _need(p, "%s parameter" % type(self).__name__)
            _need(g, "%s gradient" % type(self).__name__)
            if g.shape != p.shape or g.device != p.device:
                raise ValueError("gradient of shape %s on %s for a parameter of shape %s on %s"
                                 % (tuple(g.shape), g.device, tuple(p.shape), p.device))
            n = p.numel()
            if n == 0:
                continue
            s = _lib.OptimSegment()
            s.param, s.grad = p.data_ptr(), g.data_ptr()
            tensors = [p, g]
            if self._MOMENTS:
                m, v = state["exp_avg"], state["exp_avg_sq"]
                s.exp_avg, s.exp_avg_sq = _need(m, "exp_avg").data_ptr(), _need(v, "exp_avg_sq").data_ptr()
                tensors += [m, v]
            aux = self._aux(state, self.param_groups[gi])
            if aux is not None:
                s.aux = _need(aux, "optimizer state").data_ptr()
                tensors.append(aux)
            if self.capturable and "step" in state:        # (SGDW without momentum keeps no state)
                st = state["step"]
                s.step = _need(st, "state['step']").data_ptr()
            for t in tensors:
                if t.numel() != n or t.device != p.device:
                    raise ValueError("optimizer state does not match its parameter's shape or device")
            s.numel, s.group, s.vec = n, gi, aligned16(*tensors)
            segs.append(s)
            used.append(i)
        if not segs:
            raise ValueError("no parameter with elements to update")
        dev = rows[0][0].device
        t = Table(segs, dev, True, self._staging)
        t.pinned = torch.cuda.is_current_stream_capturing()
        t.partials = None
        t.rows_used = None if len(used) == len(rows) else used
        t.block = None if self.capturable else torch.empty(len(self.param_groups) * _lib.OPTIM_HYPER + len(used),
                                                          dtype=torch.float64, device=dev)
        return t

    def _staging(self, nbytes: int) -> torch.Tensor:
        """The page-locked staging buffer of a new table.  No page-locked allocation inside a capture: the buffer that
        the last eager build reserved is used (the captured copy reads it at every replay: it stays with the table,
        unchanged, as long as the optimizer)."""
        if torch.cuda.is_current_stream_capturing():
            host = self._spare_host
            if host is None or host.numel() < nbytes:
                raise RuntimeError("capturable %s: run one eager step() before capturing it" % type(self).__name__)
            self._spare_host = None
            return host
        self._spare_host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)

    def _aux(self, state, group):
        return None

    def _new_step(self, p):
        return torch.zeros((), dtype=torch.float32, device=p.device) if self.capturable else 0



class AdamW(_FusedOptimizer):
    """AdamW of the reference (tools/optimizers/adamw.py): decoupled weight decay taken from the parameter BEFORE the
    update (``d = p*wd; p = p - step_size*m/denom; p = p - d``), ``step_size = lr*sqrt(1-beta2^t)/(1-beta1^t)``.

    Arguments as the reference's, plus ``capturable``, ``max_grad_norm`` and ``skip_nonfinite`` (keywords; see the module
    docstring)."""
    _KIND = _lib.OPTIM_ADAMW
    _AMS_KEY = "amsgrad"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 capturable=False, max_grad_norm=None, skip_nonfinite=False):
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults)
        self._init_fused(capturable, max_grad_norm, skip_nonfinite)
        self._check_ams()

    def _check_ams(self):
        if len({bool(g[self._AMS_KEY]) for g in self.param_groups}) > 1:
            raise ValueError("%s: %s must be the same in every parameter group of the fused step"
                             % (type(self).__name__, self._AMS_KEY))

    def _flags(self) -> int:
        return _lib.OPTIM_AMS if self.param_groups[0][self._AMS_KEY] else 0

    def _hyper_row(self, gi, group):
        b1, b2 = group["betas"]
        return [group["lr"], b1, b2, group["eps"], group["weight_decay"], 0.0, 0.0, 0.0]

    def _advance(self, p, group, state):
        if len(state) == 0:
            state["step"] = self._new_step(p)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if group[self._AMS_KEY]:
                state["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            self._state_epoch += 1
        if self.capturable:
            return 0
        state["step"] += 1
        return state["step"]

    def _aux(self, state, group):
        return state["max_exp_avg_sq"] if group[self._AMS_KEY] else None


class AdaBound(AdamW):
    """AdaBound of the reference (tools/optimizers/adabound.py): L2 weight decay into a temporary gradient
    (``p.grad`` is not modified), bounds ``final_lr*lr/base_lr * (1 -+ 1/(gamma*t (+1)))``, and
    ``p = p - clamp(step_size/denom, lo, hi)*m``.  ``base_lrs`` are the groups' lr at construction, as there."""
    _KIND = _lib.OPTIM_ADABOUND
    _AMS_KEY = "amsbound"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0,
                 amsbound=False, *, capturable=False, max_grad_norm=None, skip_nonfinite=False):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= final_lr:
            raise ValueError("Invalid final learning rate: {}".format(final_lr))
        if not 0.0 <= gamma < 1.0:
            raise ValueError("Invalid gamma parameter: {}".format(gamma))
        defaults = dict(lr=lr, betas=betas, final_lr=final_lr, gamma=gamma, eps=eps, weight_decay=weight_decay,
                        amsbound=amsbound)
        Optimizer.__init__(self, params, defaults)
        self._init_fused(capturable, max_grad_norm, skip_nonfinite)
        self._check_ams()
        self.base_lrs = list(map(lambda group: group["lr"], self.param_groups))

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsbound", False)

    def _hyper_row(self, gi, group):
        b1, b2 = group["betas"]
        final_lr = group["final_lr"] * group["lr"] / self.base_lrs[gi]
        return [group["lr"], b1, b2, group["eps"], group["weight_decay"], final_lr, group["gamma"], 0.0]


class SGDW(_FusedOptimizer):
    r"""SGDW of the reference (tools/optimizers/sgdw.py), reproduced AS IT IS: the reference never applies the gradient.
    A step updates the momentum buffer (``buf = grad`` on its first update, then ``buf = momentum*buf +
    (1-dampening)*grad``; none with momentum 0) and then only decays the weights, ``p = p - weight_decay*p``; ``lr``
    and ``nesterov`` change nothing.  The trainer's call (momentum 0) is therefore a pure weight decay.

    Arguments as the reference's, plus ``capturable``, ``max_grad_norm`` and ``skip_nonfinite`` (keywords; see the module
    docstring)."""
    _KIND = _lib.OPTIM_SGDW
    _MOMENTS = False

    def __init__(self, params, lr=required, momentum=0, dampening=0, weight_decay=0, nesterov=False, *,
                 capturable=False, max_grad_norm=None, skip_nonfinite=False):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, defaults)
        self._init_fused(capturable, max_grad_norm, skip_nonfinite)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("nesterov", False)

    def _hyper_row(self, gi, group):
        return [0.0, group["momentum"], group["dampening"], 0.0, group["weight_decay"], 0.0, 0.0, 0.0]

    def _advance(self, p, group, state):
        if group["momentum"] == 0:
            return 2
        first = "momentum_buffer" not in state
        if first:
            state["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if self.capturable:
                state["step"] = self._new_step(p)
            self._state_epoch += 1
        return 1 if first else 2

    def _aux(self, state, group):
        return state["momentum_buffer"] if group["momentum"] != 0 else None


# ---- stand-alone clipping -------------------------------------------------------------------------------------------
_CLIP_TABLES = TableCache()     # (device index, gradient data pointers and sizes) -> Table


def _clip_table(grads) -> Table:
    """The cached device table of a set of gradients: segments with grad / numel / vec only, no arrival counter."""
    dev = grads[0].device
    key = (dev.index, tuple((g.data_ptr(), g.numel()) for g in grads))
    t = _CLIP_TABLES.get(key)
    if t is not None:
        _CLIP_TABLES.move_to_end(key)
        return t
    segs = []
    for g in grads:
        s = _lib.OptimSegment()
        s.grad, s.numel, s.group, s.vec = g.data_ptr(), g.numel(), 0, aligned16(g)
        segs.append(s)
    t = Table(segs, dev, False)
    t.partials = torch.empty(t.n_chunks, dtype=torch.float64, device=dev)
    return _CLIP_TABLES.add(key, t)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` for fp32 CUDA gradients as two launches: the norm pass over a cached table of
    the gradients (float64 sums, one fp32 rounding), then ``grad *= min(max_norm / (norm + 1e-6), 1)`` in place (nothing
    is written when the coefficient is 1).  Returns the norm before clipping as a 0-dim device tensor without a host
    sync; ``error_if_nonfinite=True`` reads it on the host before anything is scaled.  Parameters whose ``grad`` is None
    are skipped.  2-norm only; CPU tensors and other dtypes raise (no fallback)."""
    from .ops import _need
    if torch.is_tensor(parameters):
        parameters = [parameters]
    if float(norm_type) != 2.0:
        raise ValueError("clip_grad_norm_: only norm_type=2 is implemented, got %r" % (norm_type,))
    max_norm = float(max_norm)
    if not max_norm > 0.0:
        raise ValueError("Invalid max_norm: {}".format(max_norm))
    grads = [_need(p.grad, "clip_grad_norm_ gradient") for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    if any(g.device != grads[0].device for g in grads):
        raise ValueError("clip_grad_norm_: all gradients must live on one device")
    dev = grads[0].device
    grads = [g for g in grads if g.numel() > 0]
    if not grads:
        return torch.zeros((), dtype=torch.float32, device=dev)
    table = _clip_table(grads)
    L = _lib.lib()
    state = torch.empty(4, dtype=torch.float32, device=dev)      # this call's own: the returned norm is not overwritten
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = table.args + (C.c_void_p(table.partials.data_ptr()),)
    _lib.check(L.unetpp_grad_norm(*args, stream), "unetpp_grad_norm")
    if error_if_nonfinite:
        total = torch.sqrt(table.partials.sum())
        if not bool(torch.isfinite(total)):
            raise RuntimeError("The total norm of order 2.0 for gradients from `parameters` is non-finite, so it cannot "
                               "be clipped. To disable this error and scale the gradients by the non-finite norm "
                               "anyway, set `error_if_nonfinite=False`")
    _lib.check(L.unetpp_grad_scale(*args, max_norm, C.c_void_p(state.data_ptr()), stream), "unetpp_grad_scale")
    return state[0]


__all__ = ["AdamW", "AdaBound", "SGDW", "clip_grad_norm_"]
