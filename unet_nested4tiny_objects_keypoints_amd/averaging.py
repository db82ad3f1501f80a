"""Averaged weights on the device: the reference trainer's ``model_save == "average"`` strategy, which it names and
leaves unimplemented (trainer/trainer.py:243-252).

    avg = WeightAverager(model, kind="mean")        # "mean": equal weights (SWA); "ema": avg += (1 - decay) * (p - avg)
    for epoch ...:
        train ...
        avg.update()                                 # ONE launch over every parameter and floating buffer
    avg.update_bn(loader)                            # BatchNorm statistics OF the averaged weights (encoder column only)
    with avg.applied():                              # the model holds the averaged weights; back bit for bit on exit
        validate_step(model, ...)
    checkpoint.save_average(avg, save_dir, epoch, heatmap_loss, landmark_loss)

The averager owns one flat fp32 buffer that shadows every floating ``state_dict`` entry of the model (parameters and the
BatchNorm running statistics; every entry starts on a 16-byte boundary); the int64 ``num_batches_tracked`` counters are
shadowed by plain torch copies.  Construction fills the shadow with the model's current state (that does not count as
an update).  ``update()`` (csrc/average.hip, ``unetpp_avg_update``): with n updates made before, the first one copies,
later ones compute ``d = p - avg; avg = avg + w*d`` with ``w = 1/(n+1)`` (mean) or ``1 - decay`` (ema), each operation
rounded once.  Floating buffers are copied at every update unless ``average_buffers=True``.  ``applied()`` is one swap
launch in and one out, so nothing is allocated and the model's own weights survive in the shadow meanwhile.  The launches
write through raw pointers: ``p._version`` does not move (the weight-image pack plan is rebuilt every pass, DESIGN.md
section 4; a model with frozen weight images is invalidated by every swap).

The segment table (multi_tensor.py; the format and the chunk walk are described in csrc/multi_tensor.h) is built once per
set of data pointers and cached.

``capturable=True``: ``n_averaged`` is a float32 device scalar, the decay lives in a one-double device block, ``w`` and the
first-update decision are formed on the device and the launch itself advances the count -- no host sync, no host decision
on device data, so ``update()`` can be captured in a ``torch.cuda.graph`` after one eager ``update()``.  (The count is
exact up to 2^24 updates.)

fp32 CUDA tensors only: anything else raises (this path has no CPU fallback).
"""
from __future__ import annotations

import contextlib
import ctypes as C

import torch

from . import _lib
from .checkpoint import _unwrap
from .multi_tensor import Table, TableCache, aligned16

_KINDS = {"mean": _lib.AVG_MEAN, "ema": _lib.AVG_EMA}
_ALIGN = 4          # floats: every shadow entry starts on a 16-byte boundary


class SegmentTable(Table):
    """A device table of {avg, src} segments with the arrival counter of capturable launches.
    pairs: (avg tensor, src tensor, copy flag) -- fp32, contiguous, on one GPU, the same number of elements each."""

    def __init__(self, pairs):
        from .ops import _need
        segs, dev = [], None
        for avg, src, copy in pairs:
            _need(avg, "average")
            _need(src, "averaged tensor")
            if avg.numel() != src.numel() or avg.device != src.device:
                raise ValueError("an average does not match its tensor's size or device")
            if dev is None:
                dev = src.device
            elif src.device != dev:
                raise ValueError("every averaged tensor must live on the same device")
            n = src.numel()
            if n == 0:
                continue
            a0, s0 = avg.data_ptr(), src.data_ptr()
            if a0 < s0 + 4 * n and s0 < a0 + 4 * n:
                raise ValueError("an average overlaps its tensor")
            s = _lib.AvgSegment()
            s.avg, s.src, s.numel = a0, s0, n
            s.vec, s.copy = aligned16(avg, src), int(bool(copy))
            segs.append(s)
        if not segs:
            raise ValueError("no tensor with elements to average")
        super().__init__(segs, dev, True)

    def launch(self, kind: int, count: int = 0, decay: float = 0.0, count_dev=None, hyper_dev=None) -> None:
        """One unetpp_avg_update over the table on the current stream.  count_dev (float32 device scalar) selects the
        capturable form; hyper_dev is its one-double decay block."""
        capturable = count_dev is not None
        status = _lib.lib().unetpp_avg_update(
            kind, _lib.AVG_CAPTURABLE if capturable else 0, *self.args, int(count), float(decay),
            C.c_void_p(count_dev.data_ptr()) if capturable else None,
            C.c_void_p(hyper_dev.data_ptr()) if (capturable and hyper_dev is not None) else None,
            self.done if capturable else None,
            C.c_void_p(torch.cuda.current_stream(self.dev.device).cuda_stream))
        _lib.check(status, "unetpp_avg_update")


def _batchnorm_layers(module):
    from .unet import BatchNormParams
    return [m for m in module.modules() if isinstance(m, (BatchNormParams, torch.nn.modules.batchnorm._BatchNorm))]


class WeightAverager:
    """Running average of a model's weights, kept and updated on the device (see the module docstring).

    model: a module whose floating parameters and buffers are fp32 CUDA tensors (``UNet_Nested``, ``UNet``, or a
    DataParallel wrapper of one, which is unwrapped).  kind: "mean" or "ema"; decay in [0, 1) (ema only)."""

    def __init__(self, model, kind="mean", decay=0.999, average_buffers=False, capturable=False):
        if kind not in _KINDS:
            raise ValueError("kind must be 'mean' or 'ema', got %r" % (kind,))
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
            raise ValueError("decay must be in [0, 1), got %r" % (decay,))
        from .ops import _need
        self.kind, self.decay = kind, float(decay)
        self.average_buffers, self.capturable = bool(average_buffers), bool(capturable)
        self.model = _unwrap(model)
        self._names, self._float_names, self._int_names = [], [], []
        self._offsets = {}
        total, dev = 0, None
        params = {k for k, _ in self.model.named_parameters()}
        self._is_param = {}
        for k, t in self._entries().items():
            self._names.append(k)
            if not t.is_floating_point():
                self._int_names.append(k)
                continue
            _need(t, "WeightAverager: %s" % k)
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise ValueError("WeightAverager: every tensor of the model must live on the same device")
            self._float_names.append(k)
            self._is_param[k] = k in params
            self._offsets[k] = total
            total += (t.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        if not self._float_names:
            raise ValueError("WeightAverager: the model has no floating-point state")
        for k in self._int_names:
            if self._entries()[k].device != dev:
                raise RuntimeError("WeightAverager: %s must live on the GPU: this path has no CPU fallback" % k)
        self.device = dev
        self._flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self._ints = {k: self._entries()[k].detach().clone() for k in self._int_names}
        self._int_tmp = [t.clone() for t in self._ints.values()]   # scratch of a swap
        # where every entry lives: (the owning module's _parameters / _buffers dict, leaf name).  update() reads the
        # tensors through these instead of building a state_dict per call (a hundred entries: ~0.1 ms of host time);
        # a buffer replaced by .to() or an assignment is still found, under its owner's name
        self._slots = {}
        for k in self._names:
            owner, _, leaf = k.rpartition(".")
            mod = self.model.get_submodule(owner)
            held = mod._parameters if leaf in mod._parameters else mod._buffers
            if held.get(leaf) is None:
                raise ValueError("WeightAverager: cannot find %s on the model" % k)
            self._slots[k] = (held, leaf)
        self._tables = TableCache()
        self._applied = False
        self._n = 0
        self._count_dev = torch.zeros((), dtype=torch.float32, device=dev) if self.capturable else None
        self._hyper_dev = torch.tensor([self.decay], dtype=torch.float64, device=dev) if self.capturable else None
        self._eager_updates = 0
        self._table().launch(_lib.AVG_MEAN, count=0)     # the shadow starts as the model's state (not an update)

    # ---- storage ----------------------------------------------------------------------------------------------------
    def _entries(self):
        return self.model.state_dict(keep_vars=True)

    def _view(self, k, like):
        off = self._offsets[k]
        return self._flat[off:off + like.numel()].view(like.shape)

    def _tensor(self, k):
        held, leaf = self._slots[k]
        t = held.get(leaf)
        if t is None:
            raise RuntimeError("WeightAverager: %s is gone from the model since the averager was built" % k)
        return t

    def _table(self) -> SegmentTable:
        ent = {k: self._tensor(k) for k in self._float_names}
        key = tuple(t.data_ptr() for t in ent.values())
        table = self._tables.get(key)
        if table is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("capturable WeightAverager: run one eager update() before capturing it")
            pairs = []
            for k in self._float_names:
                t = ent[k].detach()
                if t.dtype != torch.float32 or not t.is_cuda:
                    raise RuntimeError("WeightAverager: %s must be a float32 tensor on the GPU: this path has no CPU "
                                       "fallback" % k)
                pairs.append((self._view(k, t).view(-1), t, not (self._is_param[k] or self.average_buffers)))
            table = self._tables.add(key, SegmentTable(pairs))
        else:
            self._tables.move_to_end(key)
        return table

    # ---- update -----------------------------------------------------------------------------------------------------
    @property
    def n_averaged(self):
        """Updates made so far: an int, or the float32 device scalar of a capturable averager."""
        return self._count_dev if self.capturable else self._n

    @torch.no_grad()
    def update(self) -> None:
        """Takes the model's current state into the average: one launch."""
        if self._applied:
            raise RuntimeError("WeightAverager.update() inside applied(): the model holds the averaged weights")
        kind = _KINDS[self.kind]
        if self.capturable:
            if torch.cuda.is_current_stream_capturing() and not self._eager_updates:
                raise RuntimeError("capturable WeightAverager: run one eager update() before capturing it")
            self._table().launch(kind, count_dev=self._count_dev, hyper_dev=self._hyper_dev)
            if not torch.cuda.is_current_stream_capturing():
                self._eager_updates += 1
        else:
            self._table().launch(kind, count=self._n, decay=self.decay)
            self._n += 1
        if self._ints:
            torch._foreach_copy_([self._ints[k] for k in self._int_names],
                                 [self._tensor(k).detach() for k in self._int_names])

    # ---- the averaged weights in the model -----------------------------------------------------------------------------
    def _swap(self) -> None:
        self._table().launch(_lib.AVG_SWAP)
        if self._ints:
            mine = [self._ints[k] for k in self._int_names]
            theirs = [self._tensor(k).detach() for k in self._int_names]
            torch._foreach_copy_(self._int_tmp, theirs)      # three launches, whatever the number of counters
            torch._foreach_copy_(theirs, mine)
            torch._foreach_copy_(mine, self._int_tmp)
        inval = getattr(self.model, "invalidate_weight_images", None)
        if inval is not None:
            inval()

    @contextlib.contextmanager
    def applied(self):
        """While the block runs the model holds the averaged weights and the averager's BatchNorm statistics (one swap
        launch in, one out; the model's own state waits in the shadow).  On exit everything is back bit for bit, except
        that whatever the block wrote into the model -- update_bn's statistics -- stays with the averager."""
        if self._applied:
            raise RuntimeError("WeightAverager.applied() is already active: it does not nest")
        with torch.no_grad():
            self._swap()
        self._applied = True
        try:
            yield self.model
        finally:
            with torch.no_grad():
                self._swap()
            self._applied = False

    # ---- BatchNorm statistics of the averaged weights ----------------------------------------------------------------
    @torch.no_grad()
    def update_bn(self, batches) -> None:
        """torch.optim.swa_utils.update_bn for the averaged weights: under applied(), the running statistics are reset
        and every batch k (0-based; a tensor, or a list / tuple whose first item is the input) goes through a statistics
        pass with every BatchNorm layer in training mode and momentum 1 / (k + 1) -- the cumulative average.  The fresh
        statistics end up in the averager; the model's own statistics, momenta and training flags are untouched.
        UNet_Nested runs only its encoder column (engine.stats_pass); other modules take a whole training-mode forward
        under no_grad.  A model without BatchNorm returns at once."""
        from . import engine
        from .unet import UNet_Nested
        layers = _batchnorm_layers(self.model)
        if not layers:
            return
        nested = isinstance(self.model, UNet_Nested)
        with self.applied():
            modes = [(m, m.training) for m in self.model.modules()]
            momenta = [bn.momentum for bn in layers]
            try:
                for bn in layers:
                    bn.running_mean.zero_()
                    bn.running_var.fill_(1.0)
                    bn.num_batches_tracked.zero_()
                if nested:
                    for bn in layers:
                        torch.nn.Module.train(bn, True)
                else:
                    self.model.train()
                for k, batch in enumerate(batches):
                    x = batch[0] if isinstance(batch, (list, tuple)) else batch
                    x = x.to(self.device, non_blocking=True)
                    for bn in layers:
                        bn.momentum = 1.0 / (k + 1)
                    if nested:
                        engine.stats_pass(self.model, x)
                    else:
                        self.model(x)
            finally:
                for bn, mom in zip(layers, momenta):
                    bn.momentum = mom
                for m, mode in modes:
                    m.training = mode

    # ---- state ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def averaged_state_dict(self):
        """Clones of the averaged entries under the model's (= the reference's) key names, in its order: loads into this
        package's model and into the reference's."""
        if self._applied:
            raise RuntimeError("WeightAverager.averaged_state_dict() inside applied(): the shadow holds the model's own "
                               "weights; read model.state_dict() instead")
        ent = self.model.state_dict()
        out = type(ent)()
        for k in self._names:
            out[k] = self._ints[k].clone() if k in self._ints else self._view(k, ent[k]).clone()
        if hasattr(ent, "_metadata"):
            out._metadata = ent._metadata
        return out

    def state_dict(self):
        """What a resume needs: kind, decay, n_averaged (an int) and the averaged entries."""
        n = int(self._count_dev.item()) if self.capturable else self._n
        return {"kind": self.kind, "decay": self.decay, "average_buffers": self.average_buffers, "n_averaged": n,
                "averaged": self.averaged_state_dict()}

    @torch.no_grad()
    def load_state_dict(self, state) -> None:
        if self._applied:
            raise RuntimeError("WeightAverager.load_state_dict() inside applied()")
        if state["kind"] != self.kind:
            raise ValueError("the saved average is of kind %r, this averager of kind %r" % (state["kind"], self.kind))
        decay = float(state["decay"])
        if not 0.0 <= decay < 1.0:
            raise ValueError("decay must be in [0, 1), got %r" % (decay,))
        saved = state["averaged"]
        if list(saved) != self._names:
            missing, extra = [k for k in self._names if k not in saved], [k for k in saved if k not in self._names]
            raise RuntimeError("the saved average does not fit this model: missing keys %s, unexpected keys %s (or another "
                               "order)" % (missing, extra))
        ent = self._entries()
        for k in self._names:
            if tuple(saved[k].shape) != tuple(ent[k].shape):
                raise RuntimeError("the saved average of %s has shape %s, the model's tensor %s"
                                   % (k, tuple(saved[k].shape), tuple(ent[k].shape)))
        for k in self._names:
            dst = self._ints[k] if k in self._ints else self._view(k, ent[k])
            dst.copy_(saved[k].to(dtype=dst.dtype))
        self.decay = decay
        n = int(state["n_averaged"])
        if self.capturable:
            self._count_dev.fill_(float(n))
            self._hyper_dev.fill_(self.decay)
        else:
            self._n = n


__all__ = ["WeightAverager", "SegmentTable"]
