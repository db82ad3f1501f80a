"""Tensor-facing wrappers over the C ABI (include/unetpp_hip.h).

Every function takes CUDA(HIP) fp32 tensors owned by PyTorch, hands raw pointers, sizes and the
current HIP stream to the library, and returns immediately (asynchronous on that stream).  PyTorch
here is plumbing only: device memory and the stream.  Activations are NHWC ``[N, H, W, C]``.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import MAX_VIEWS, GemmDesc, PackJob, View, WeightSrc, WgradDesc, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class LaunchTimer:
    """Optional per-launch timing with HIP events on the launching stream (used by bench.py for the
    roofline line).  Records (kind, flops, bytes, start_event, end_event) for every MFMA-kernel launch
    and (name, start, end) for named regions; read the times after a device synchronise.  An event pair costs the
    stream about 6 us, so a caller that wants honest region times samples launches and regions on DIFFERENT steps
    (want_launches / want_regions)."""

    def __init__(self):
        self.launches = []
        self.regions = []
        self.want_launches = True
        self.want_regions = True

    def _pair(self):
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def summary(self):
        out = {}
        for kind, flops, nbytes, s, e in self.launches:
            d = out.setdefault(kind, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += flops
            d["bytes"] += nbytes
        reg = {}
        for name, s, e in self.regions:
            d = reg.setdefault(name, {"count": 0, "ms": 0.0})
            d["count"] += 1
            d["ms"] += s.elapsed_time(e)
        return out, reg


_TIMER: Optional[LaunchTimer] = None


def set_timer(t: Optional[LaunchTimer]) -> None:
    global _TIMER
    _TIMER = t


class region:
    """with ops.region("X00.fwd"): ...  -- a named span on the current stream when a LaunchTimer is set."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = _TIMER is not None and _TIMER.want_regions
        if self.on:
            self.s, self.e = _TIMER._pair()
            self.s.record()
        return self

    def __exit__(self, *exc):
        if self.on and _TIMER is not None:
            self.e.record()
            _TIMER.regions.append((self.name, self.s, self.e))
        return False


def _timed_call(kind, flops, fn, nbytes=0.0):
    """kind = label of the launch, or None to ask the library which kernel it picked (unetpp_last_kernel_name).
    flops / nbytes: ALGORITHMIC work of the launch (every operand element read or written once)."""
    if _TIMER is None or not _TIMER.want_launches:
        return fn()
    s, e = _TIMER._pair()
    s.record()
    r = fn()
    e.record()
    if kind is None:
        kind = _lib.lib().unetpp_last_kernel_name().decode()
    _TIMER.launches.append((kind, flops, nbytes, s, e))
    return r


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need(t: torch.Tensor, what: str, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU: this path has no CPU fallback" % what)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (what, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    return t


def _window_rows(index: torch.Tensor, params: torch.Tensor, n: Optional[int] = None) -> int:
    """N of index [N] / params [N, 16], the rows of a warp; n: the N they must have (a target's)."""
    rows = int(index.numel())
    if index.dim() != 1 or (n is not None and rows != n) or tuple(params.shape) != (rows, _lib.WARP_PARAMS):
        raise ValueError("index [N] and params [N, %d]" % _lib.WARP_PARAMS
                         + ("" if n is None else " for a target of N = %d samples" % n))
    return rows


def _frame_store(store: torch.Tensor, shape_error: str = "store must be a contiguous 4-d tensor"):
    """store -> (u8, M, Hs, Ws, C): the frames as uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws]."""
    if not store.is_cuda:
        raise RuntimeError("store must live on the GPU: this path has no CPU fallback")
    if store.dtype not in (torch.uint8, torch.float32):
        raise TypeError("store must be uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws], got %s" % store.dtype)
    if store.dim() != 4 or not store.is_contiguous():
        raise ValueError(shape_error)
    u8 = store.dtype == torch.uint8
    hs, ws, c = store.shape[1:] if u8 else (store.shape[2], store.shape[3], store.shape[1])
    return u8, int(store.shape[0]), int(hs), int(ws), int(c)


def _label_table(labels: torch.Tensor, label_class: torch.Tensor):   # -> (M, L)
    if labels.dim() != 3 or labels.shape[2] != 2 or tuple(label_class.shape) != tuple(labels.shape[:2]):
        raise ValueError("labels must be [M, L, 2] and label_class [M, L]")
    return int(labels.shape[0]), int(labels.shape[1])


_ACT_DTYPES = (torch.float32, torch.bfloat16)  # storage types of activations (bf16: UNETPP_GEMM_BF16 launches)


def _storage_flag(outs, ins):
    """UNETPP_GEMM_BF16 when the launch's activations are bf16.  All views of a launch share the storage type, except
    that the 1..4-channel network input of the first convolution stays fp32."""
    bf = outs[0].t.dtype == torch.bfloat16
    for v in outs:
        if (v.t.dtype == torch.bfloat16) != bf:
            raise TypeError("mixed fp32 / bf16 output views in one launch")
    for v in ins:
        if (v.t.dtype == torch.bfloat16) != bf and not (bf and len(ins) == 1 and v.t.shape[3] <= 4):
            raise TypeError("mixed fp32 / bf16 views in one launch")
    return _lib.GEMM_BF16 if bf else 0


@dataclass
class V:
    """A channel slice of an NHWC tensor (fp32 or bf16 storage), optionally on a strided pixel grid (struct unetpp_view)."""
    t: torch.Tensor
    c_off: int = 0
    c_len: Optional[int] = None
    sy: int = 1
    sx: int = 1
    oy: int = 0
    ox: int = 0
    scale: Optional[torch.Tensor] = None
    shift: Optional[torch.Tensor] = None
    gate: Optional[torch.Tensor] = None
    relu: bool = False
    accumulate: bool = False
    gate_sum: bool = False

    def fill(self, dst: View) -> int:
        t = _need(self.t, "view tensor", self.t.dtype if self.t.dtype in _ACT_DTYPES else torch.float32)
        if t.dim() != 4:
            raise ValueError("view tensor must be NHWC [N,H,W,C]")
        c = t.shape[3]
        n = c - self.c_off if self.c_len is None else self.c_len
        dst.ptr = t.data_ptr()
        dst.C, dst.c_off, dst.c_len = c, self.c_off, n
        dst.Hs, dst.Ws = t.shape[1], t.shape[2]
        dst.sy, dst.sx, dst.oy, dst.ox = self.sy, self.sx, self.oy, self.ox
        dst.scale = None if self.scale is None else _need(self.scale, "scale").data_ptr()
        dst.shift = None if self.shift is None else _need(self.shift, "shift").data_ptr()
        if self.gate is not None:
            g = _need(self.gate, "gate", t.dtype)
            if g.shape != t.shape:
                raise ValueError("gate must have the geometry of the gated tensor")
            dst.gate = g.data_ptr()
        else:
            dst.gate = None
        dst.relu = int(self.relu)
        dst.accumulate = int(self.accumulate)
        dst.gate_sum = int(self.gate_sum)
        return n


USE_FAST_GEMM = True  # tests flip this to exercise the generic kernel on the same shapes
USE_WINOGRAD = os.environ.get("UNETPP_NO_WINOGRAD") is None  # 3x3 fast path: Winograd F(2x2,3x3) unless disabled


@dataclass
class WSrc:
    """A GEMM weight [taps][K][N] given by a parameter in its torch layout (struct unetpp_weight_src): element
    (tap, k, n) sits at tap' * s_t + (k % k_inner) * s_k + (k // k_inner) * s_ko + (n % n_inner) * s_n +
    (n // n_inner) * s_no, tap' = taps-1-tap when flip.  The fast kernels build their LDS image straight from it;
    `packed()` materialises the [taps][K][N] operand for the generic kernel."""
    t: torch.Tensor
    taps: int
    k: int
    n: int
    s_t: int
    s_k: int
    s_n: int
    s_ko: int = 0
    s_no: int = 0
    k_inner: int = 0
    n_inner: int = 0
    flip: bool = False
    pack: Optional[callable] = None  # () -> packed tensor

    def numel(self) -> int:
        return self.taps * self.k * self.n

    @property
    def device(self):
        return self.t.device

    def fill(self, dst: WeightSrc) -> None:
        dst.src = _need(self.t, "weight").data_ptr()
        dst.s_t, dst.s_k, dst.s_ko, dst.s_n, dst.s_no = self.s_t, self.s_k, self.s_ko, self.s_n, self.s_no
        dst.k_inner, dst.n_inner, dst.flip = self.k_inner, self.n_inner, int(self.flip)

    def packed(self) -> torch.Tensor:
        if self.pack is None:
            raise ValueError("this weight source has no packed form")
        return self.pack()


class PackPlan:
    """All weight images of a forward (or backward) pass in ONE launch (unetpp_gemm_pack_weight_images).

    The first time a launch is seen (engine pass `phase`, weight source, channel structure) its image is packed by
    itself into a persistent buffer and a job is recorded; from then on `begin(phase)` packs every recorded image of
    that pass with a single kernel before the pass starts and the launches just pick their buffer.

    The images are rebuilt on EVERY pass: nothing observable from Python says that a parameter's storage kept its
    contents (the reference's own optimizers update through ``p.data`` -- tools/optimizers/adamw.py:95-98,
    sgdw.py:108, adabound.py:120 -- which leaves ``p._version`` untouched, as do ``init.*_(m.weight.data)``,
    ``dist.broadcast(p.data)`` or EMA/clipping through ``.data``).  Skipping is an explicit opt-in for serving:
    ``frozen = True`` (UNet_Nested.freeze_weight_images) keeps the images until ``invalidate()``, which the module
    calls from ``load_state_dict``, ``_apply`` (.to()/.float()/.cuda()) and ``train()``.  Entries keep their source
    tensor alive and are dropped when unused for a few passes."""

    class _Entry:  # one weight image; like _Copy: jobs, size (of the largest job: sizes the grid) and device feed _run_jobs
        __slots__ = ("image", "n_img", "jobs", "size", "device", "src", "phase", "fresh", "used")

    class _Copy:  # a group of strided copies into one destination buffer (unetpp_copy_jobs), redone with the images
        __slots__ = ("dst", "jobs", "size", "device", "srcs", "srcsig", "phase", "fresh", "used")

    def __init__(self):
        self.entries = {}
        self.copies = {}     # key -> _Copy
        self._copy_tables = {}  # phase -> (keys, device table, jobs, max elements)
        self.copy_launches = 0  # batched copy launches issued (tests)
        self._tables = {}    # phase -> (signatures, device table, jobs, max floats)
        self._packed = set()  # phases whose images are current (only consulted while frozen)
        self.frozen = False
        self.phase = None
        self.pass_id = 0
        self.launches = 0     # batched pack launches issued (tests)
        self.pinned = 0       # > 0 while a captured HIP graph holds raw pointers into this plan (serving.GraphedForward)
        self._retired = []    # job tables replaced while pinned: a captured pack launch may still read them

    def pin(self) -> None:
        """A captured graph bakes in the addresses of the weight images and of the device job table of its pack launch:
        while pinned, entries are not evicted and a replaced job table is kept alive instead of freed."""
        self.pinned += 1

    def unpin(self) -> None:
        self.pinned = max(0, self.pinned - 1)
        if not self.pinned:
            self._retired.clear()

    def invalidate(self) -> None:
        """The parameters may have changed: the next pass of every phase rebuilds its images."""
        self._packed.clear()

    def __deepcopy__(self, memo):  # copies / pickles of a model start with an empty plan
        return PackPlan()

    def __reduce__(self):
        return (PackPlan, ())

    def begin(self, phase: str) -> None:
        self.phase = phase
        self.pass_id += 1
        if not self.pinned:
            self._evict(self.entries, self._tables)
            self._evict(self.copies, self._copy_tables)
        # (copies first: weight images of this pass may be packed FROM a copied buffer)
        self.copy_launches += self._run_jobs(phase, self.copies, self._copy_tables, _lib.CopyJob, "unetpp_copy_jobs")
        if self._run_jobs(phase, self.entries, self._tables, PackJob, "unetpp_gemm_pack_weight_images"):
            self.launches += 1
            self._packed.add(phase)

    def _evict(self, items, tables) -> None:
        """Drop what no pass used for 16 passes.  An evicted record takes its phase's job table with it: the table's rows
        hold the address of the entry's image (of the copy's destination), and a pass that records the same launches again
        gets the same keys -- a table kept by key alone would make the batched launch write into the freed buffers."""
        for k in [k for k, x in items.items() if self.pass_id - x.used > 16]:
            tables.pop(items[k].phase, None)
            del items[k]

    def _run_jobs(self, phase: str, items, tables, job_type, entry_point: str) -> bool:
        """ONE launch of `entry_point` (job table in device memory, jobs, size of the largest) for all that `items` holds
        under `phase`; -> launched.  The table is rebuilt when the phase's keys changed (the replaced one is kept while
        pinned); while frozen, a phase whose images are current launches nothing."""
        keys = tuple(k for k, x in items.items() if x.phase == phase)
        if not keys:
            return False
        recs = [items[k] for k in keys]
        tab = tables.get(phase)
        if tab is None or tab[0] != keys:
            if self.pinned and tab is not None:
                self._retired.append(tab)
            jobs = [j for x in recs for j in x.jobs]
            dev = torch.frombuffer(bytearray(bytes((job_type * len(jobs))(*jobs))), dtype=torch.uint8).to(recs[0].device)
            tab = tables[phase] = (keys, dev, len(jobs), max(x.size for x in recs))
            self._packed.discard(phase)
        launched = not (self.frozen and phase in self._packed)
        if launched:
            check(getattr(_lib.lib(), entry_point)(_ptr(tab[1]), tab[2], tab[3], _stream()), entry_point)
        for x in recs:
            x.fresh = self.pass_id
        return launched

    def copy_for(self, key, phase: str, srcsig, make):
        """A destination buffer filled by strided copies that ``begin(phase)`` redoes in ONE launch from the second pass on.
        -> (dst, ready): ready = the buffer already holds this pass's contents.  The first time `key` is seen -- or when
        `srcsig` (whatever identifies the sources: their addresses) changed -- ``make()`` -> (dst tensor, source tensors
        kept alive, [(src tensor, src offset, dst offset, n_outer, n_inner, src_stride, dst_stride) in floats]) builds the
        job list; the caller fills the buffer itself for that pass (ready = False)."""
        c = self.copies.get(key)
        if c is None or c.srcsig != srcsig or c.phase != phase:
            dst, srcs, items = make()
            c = PackPlan._Copy()
            c.dst, c.device, c.srcs, c.srcsig, c.phase, c.fresh = dst, dst.device, srcs, srcsig, phase, -1
            c.jobs, c.size = [], 1
            for (src, s_off, d_off, n_outer, n_inner, s_stride, d_stride) in items:
                j = _lib.CopyJob()
                j.src, j.dst = src.data_ptr() + 4 * s_off, dst.data_ptr() + 4 * d_off
                j.n_outer, j.n_inner, j.src_stride, j.dst_stride = n_outer, n_inner, s_stride, d_stride
                if n_outer * n_inner >= 2 ** 31:
                    raise ValueError("copy job too large")
                c.jobs.append(j)
                c.size = max(c.size, n_outer * n_inner)
            self.copies[key] = c
            old_tab = self._copy_tables.pop(phase, None)   # same keys, other jobs: the table is rebuilt by the next begin()
            if old_tab is not None and self.pinned:
                self._retired.append(old_tab)
        c.used = self.pass_id
        return c.dst, c.fresh == self.pass_id

    def knows_copy(self, key, phase: str, srcsig) -> bool:
        """begin(phase) will fill this buffer (callers that run BEFORE begin: the grouped input-gradient weights)"""
        c = self.copies.get(key)
        return c is not None and c.srcsig == srcsig and c.phase == phase

    def image_for(self, sig, n_img: int, weight: "WSrc", d: GemmDesc):
        """-> (image tensor, already packed for this pass)"""
        e = self.entries.get(sig)
        if e is None:
            e = PackPlan._Entry()
            e.image = torch.empty(n_img, dtype=torch.float32, device=weight.device)
            e.n_img, e.size, e.device, e.src, e.phase, e.fresh = n_img, n_img, weight.device, weight.t, self.phase, -1
            job = PackJob()
            weight.fill(job.src)
            job.image = e.image.data_ptr()
            job.taps, job.flags, job.n_in, job.n_out = d.taps, d.flags, d.n_in, d.n_out
            for i in range(d.n_in):
                job.in_len[i] = d.inp[i].c_len
            for i in range(d.n_out):
                job.out_len[i] = d.out[i].c_len
            e.jobs = [job]
            self.entries[sig] = e
        e.used = self.pass_id
        return e.image, e.fresh == self.pass_id


_PLAN: Optional[PackPlan] = None
_NO_IMAGE_YET = 16  # d.weight_image while a launch is planned: "an image will be there" (never dereferenced)


def set_pack_plan(plan: Optional[PackPlan]) -> None:
    global _PLAN
    _PLAN = plan


def current_plan() -> Optional[PackPlan]:
    """the plan of the engine pass that is running, if any"""
    return _PLAN if (_PLAN is not None and _PLAN.phase is not None) else None


def phase_tag(phase) -> tuple:
    """() for the two whole-network passes, (phase,) for a pruned pass ("fwd/J", "bwd/J": engine.plan_phase): part of the key
    of whatever a plan records, so that a pruned pass owns its images and its copies -- its ``begin`` packs the weights of
    the nodes it runs and nothing else, and the entries of the whole-network passes stay exactly what they were."""
    return () if phase in ("fwd", "bwd") else (phase,)


def gemm_pixel_blocks(n: int, h: int, w: int) -> int:
    return int(_lib.lib().unetpp_gemm_pixel_blocks(n, h, w))


@dataclass
class BatchNormFinish:
    """BatchNorm finalize attached to the convolution call that takes the statistics (struct unetpp_bn_fused): the call
    leaves mean / invstd / scale / shift and the updated running statistics behind; the persistent kernels write one
    row of sums per workgroup and the library finishes those few rows itself."""
    gamma: torch.Tensor
    beta: torch.Tensor
    running_mean: Optional[torch.Tensor]
    running_var: Optional[torch.Tensor]
    eps: float
    momentum: float
    count: int

    def outputs(self, c: int):
        dev = self.gamma.device
        self.mean, self.invstd, self.scale, self.shift = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(4))
        return self.mean, self.invstd, self.scale, self.shift


def gemm_stats_rows(n: int, h: int, w: int) -> int:
    return int(_lib.lib().unetpp_gemm_stats_rows(n, h, w))


def gemm_fwd(n: int, h: int, w: int, taps: int, ins: Sequence[V], outs: Sequence[V], weight: torch.Tensor,
             bias: Optional[torch.Tensor] = None, stats_partial: Optional[torch.Tensor] = None,
             direct: bool = False, bn: Optional[BatchNormFinish] = None) -> _lib.GemmSizes:
    """direct=True forbids the Winograd form of the 3x3 fast path (bit-exact direct summation).
    bn: finalize the BatchNorm statistics inside this call (stats_partial then is workspace of gemm_stats_rows() rows).
    Returns the library's plan of the launch (kernel label, grid, image size, finalize rows: unetpp_gemm_plan)."""
    if len(ins) > MAX_VIEWS or len(outs) > MAX_VIEWS:
        raise ValueError("too many views")
    d = GemmDesc()
    d.N, d.H, d.W, d.taps = n, h, w, taps
    d.flags = (_lib.GEMM_DIRECT if (direct or not USE_WINOGRAD) else 0) | _storage_flag(outs, ins)
    d.n_in, d.n_out = len(ins), len(outs)
    k = sum(v.fill(d.inp[i]) for i, v in enumerate(ins))
    nc = sum(v.fill(d.out[i]) for i, v in enumerate(outs))
    from_src = isinstance(weight, WSrc)  # parameter in torch layout, or the packed [taps][K][N] operand
    if not from_src:
        _need(weight, "packed weight")
    if weight.numel() != taps * k * nc or (from_src and (weight.taps, weight.k, weight.n) != (taps, k, nc)):
        raise ValueError("weight has %d elements, expected %d*%d*%d" % (weight.numel(), taps, k, nc))
    if bias is not None and _need(bias, "bias").numel() != nc:
        raise ValueError("bias length mismatch")
    rows = gemm_pixel_blocks(n, h, w) if bn is None else gemm_stats_rows(n, h, w)
    if stats_partial is not None and _need(stats_partial, "stats").numel() != rows * nc * 2:
        raise ValueError("stats_partial size mismatch")
    if bn is not None:
        if stats_partial is None or len(outs) != 1:
            raise ValueError("a fused BatchNorm finalize needs stats_partial and a single output view")
        mean, invstd, scale, shift = bn.outputs(nc)
        for t, what in ((bn.gamma, "gamma"), (bn.beta, "beta")):
            if _need(t, what).numel() != nc:
                raise ValueError("BatchNorm %s length mismatch" % what)
        d.bn.gamma, d.bn.beta = bn.gamma.data_ptr(), bn.beta.data_ptr()
        d.bn.running_mean = None if bn.running_mean is None else _need(bn.running_mean, "running_mean").data_ptr()
        d.bn.running_var = None if bn.running_var is None else _need(bn.running_var, "running_var").data_ptr()
        d.bn.mean, d.bn.invstd, d.bn.scale, d.bn.shift = mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr()
        d.bn.count, d.bn.eps, d.bn.momentum = int(bn.count), float(bn.eps), float(bn.momentum)

    d.weight = None if from_src else weight.data_ptr()
    d.bias = None if bias is None else bias.data_ptr()
    d.stats_partial = None if stats_partial is None else stats_partial.data_ptr()
    # One look at the descriptor (unetpp_gemm_plan) for the launch as it will run with a weight image: only whether
    # d.weight_image is NULL counts for the plan, so the image is allocated from the plan's own image_floats.  A refusal
    # means no image kernel takes these views: the launch then reads the packed operand and is planned as that.
    lib = _lib.lib()
    plan = _lib.GemmSizes()
    d.weight_image = _NO_IMAGE_YET if USE_FAST_GEMM else None
    if USE_FAST_GEMM and lib.unetpp_gemm_plan(C.byref(d), 0, C.byref(plan)) != 0:
        d.weight_image = None
    if d.weight_image is not None:  # aligned views: a fast kernel applies; its weight image is built in one launch
        n_img = int(plan.image_floats)
        ready = False
        if from_src and _PLAN is not None and _PLAN.phase is not None:
            sig = (weight.t.data_ptr(), weight.s_t, weight.s_k, weight.s_ko, weight.s_n, weight.s_no, weight.k_inner,
                   weight.n_inner, weight.flip, taps, d.flags, tuple(v.c_len for v in d.inp[:d.n_in]),
                   tuple(v.c_len for v in d.out[:d.n_out])) + phase_tag(_PLAN.phase)
            image, ready = _PLAN.image_for(sig, n_img, weight, d)
        else:
            image = torch.empty(n_img, dtype=torch.float32, device=weight.device)
        if ready:
            pass  # packed by PackPlan.begin() together with the other images of this pass
        elif from_src:
            ws = WeightSrc()
            weight.fill(ws)
            check(lib.unetpp_gemm_pack_weight_image_from(C.byref(d), C.byref(ws), _ptr(image), _stream()),
                  "unetpp_gemm_pack_weight_image_from")
        else:
            check(lib.unetpp_gemm_pack_weight_image(C.byref(d), _ptr(image), _stream()),
                  "unetpp_gemm_pack_weight_image")
        d.weight_image = image.data_ptr()
    if d.weight_image is None:
        if from_src:  # generic kernel: it reads the packed operand
            packed = weight.packed()
            d.weight = packed.data_ptr()
        check(lib.unetpp_gemm_plan(C.byref(d), 0, C.byref(plan)), "unetpp_gemm_plan")
    # operands the launch has to read besides its inputs: accumulated outputs and ReLU gates of the output views
    acc = sum(v.c_len for v in d.out[:d.n_out] if v.accumulate) + sum(v.c_len for v in d.out[:d.n_out] if v.gate)
    _timed_call(None, 2.0 * n * h * w * taps * k * nc,
                lambda: check(lib.unetpp_gemm_fwd(C.byref(d), _stream()), "unetpp_gemm_fwd"),
                (2.0 if d.flags & _lib.GEMM_BF16 else 4.0) * n * h * w * (k + nc + acc))
    return plan


def first_layer_dgrad_bf16(dy: torch.Tensor, weight: torch.Tensor, dx: torch.Tensor) -> None:
    """dx fp32 [N,H,W,Cin<=4] = input gradient of the first 3x3 convolution from a bf16 dy [N,H,W,Cout]"""
    n, h, w, co = dy.shape
    ci = dx.shape[3]
    _need(dy, "dy", torch.bfloat16)
    _need(weight, "weight")
    _need(dx, "dx")
    if tuple(weight.shape) != (co, ci, 3, 3) or tuple(dx.shape[:3]) != (n, h, w):
        raise ValueError("shape mismatch")
    check(_lib.lib().unetpp_first_layer_dgrad_bf16(_ptr(dy), _ptr(weight), n, h, w, ci, co, _ptr(dx), _stream()),
          "unetpp_first_layer_dgrad_bf16")


def pack_weight(dst: torch.Tensor, src: torch.Tensor, t: int, k: int, n: int, dstr, sstr, flip: bool = False) -> None:
    _need(dst, "pack dst")
    _need(src, "pack src")
    check(_lib.lib().unetpp_pack_weight(_ptr(dst), _ptr(src), t, k, n, dstr[0], dstr[1], dstr[2],
                                        sstr[0], sstr[1], sstr[2], int(flip), _stream()), "unetpp_pack_weight")


def wgrad(n: int, h: int, w: int, taps: int, xs: Sequence[V], dys: Sequence[V], dw: Optional[torch.Tensor],
          dw_strides, db: Optional[torch.Tensor], n_inner: Optional[int] = None, target_blocks: int = 256,
          direct: bool = False) -> _lib.WgradSizes:
    """dw / db are written (not accumulated).  dw_strides = (d_t, d_k, d_n, d_o) into the torch-layout gradient.
    direct=True forbids the Winograd form of the 3x3 kernel.  Returns the library's plan of the launch (kernel label,
    n_split, slab layout: unetpp_wgrad_plan)."""
    lib = _lib.lib()
    d = WgradDesc()
    d.N, d.H, d.W, d.taps = n, h, w, taps
    d.n_x, d.n_dy = len(xs), len(dys)
    k = sum(v.fill(d.x[i]) for i, v in enumerate(xs))
    nc = sum(v.fill(d.dy[i]) for i, v in enumerate(dys))
    d.flags = (_lib.GEMM_DIRECT if (direct or not USE_WINOGRAD) else 0) | _storage_flag(dys, xs)
    plan = _lib.WgradSizes()
    check(lib.unetpp_wgrad_plan(C.byref(d), target_blocks, C.byref(plan)), "unetpp_wgrad_plan")
    slabs = torch.empty(plan.slab_floats, dtype=torch.float32, device=xs[0].t.device)
    d.n_split, d.slabs = plan.n_split, slabs.data_ptr()
    _timed_call(None, 2.0 * n * h * w * taps * k * nc,
                lambda: check(lib.unetpp_wgrad(C.byref(d), _stream()), "unetpp_wgrad"),
                (2.0 if d.flags & _lib.GEMM_BF16 else 4.0) * n * h * w * (k + nc))
    if n_inner is None:
        n_inner = nc
    check(lib.unetpp_wgrad_finish(_ptr(slabs), plan.n_split, plan.planes, k, nc, n_inner, _ptr(dw), dw_strides[0],
                                  dw_strides[1], dw_strides[2], dw_strides[3], _ptr(db), _stream()), "unetpp_wgrad_finish")
    return plan


def bn_finalize(partial, n_blocks, c, count, gamma, beta, eps, momentum, running_mean, running_var):
    dev = partial.device
    mean, invstd, scale, shift = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(4))
    check(_lib.lib().unetpp_bn_finalize(_ptr(partial), n_blocks, c, count, _ptr(gamma), _ptr(beta), eps, momentum,
                                        _ptr(running_mean), _ptr(running_var), _ptr(mean), _ptr(invstd), _ptr(scale),
                                        _ptr(shift), _stream()), "unetpp_bn_finalize")
    return mean, invstd, scale, shift


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps):
    c = gamma.numel()
    scale, shift = (torch.empty(c, dtype=torch.float32, device=gamma.device) for _ in range(2))
    check(_lib.lib().unetpp_bn_eval_coeffs(_ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), eps, c,
                                           _ptr(scale), _ptr(shift), _stream()), "unetpp_bn_eval_coeffs")
    return scale, shift


def bn_eval_coeffs_stats(gamma, beta, running_mean, running_var, eps):
    """(mean, invstd, scale, shift) of a frozen layer: bn_eval_coeffs' scale / shift (same kernel, same bits) plus the
    snapshot of running_mean and 1/sqrt(running_var + eps) that bn_frozen_backward's sums read."""
    c = gamma.numel()
    mean, invstd, scale, shift = (torch.empty(c, dtype=torch.float32, device=gamma.device) for _ in range(4))
    check(_lib.lib().unetpp_bn_eval_coeffs_stats(_ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), eps, c,
                                                 _ptr(scale), _ptr(shift), _ptr(mean), _ptr(invstd), _stream()),
          "unetpp_bn_eval_coeffs_stats")
    return mean, invstd, scale, shift


def _is_bf16(t):
    return t.dtype == torch.bfloat16


def affine_relu_pool(y, scale, shift, relu, act, pooled, pool_idx):
    n, h, w, c = y.shape
    if _is_bf16(y):
        check(_lib.lib().unetpp_affine_relu_pool_bf16(_ptr(y), _ptr(scale), _ptr(shift), int(relu), n, h, w, c, _ptr(act),
                                                      _ptr(pooled), _ptr(pool_idx), _stream()),
              "unetpp_affine_relu_pool_bf16")
        return
    check(_lib.lib().unetpp_affine_relu_pool(_ptr(y), _ptr(scale), _ptr(shift), int(relu), n, h, w, c, _ptr(act),
                                             _ptr(pooled), _ptr(pool_idx), _stream()), "unetpp_affine_relu_pool")


def maxpool_bwd(d_pooled, pool_idx, d_act, gate=None):
    """d_act[window argmax] += d_pooled; bf16 storage: optionally followed by d_act *= (gate > 0) (the node's ReLU mask)"""
    n, h, w, c = d_act.shape
    if _is_bf16(d_act):
        check(_lib.lib().unetpp_maxpool_bwd_bf16(_ptr(d_pooled), _ptr(pool_idx), n, h, w, c, _ptr(d_act), _ptr(gate), _stream()),
              "unetpp_maxpool_bwd_bf16")
        return
    if gate is not None:
        raise ValueError("the fused ReLU mask is a bf16-storage option")
    check(_lib.lib().unetpp_maxpool_bwd(_ptr(d_pooled), _ptr(pool_idx), n, h, w, c, _ptr(d_act), _stream()),
          "unetpp_maxpool_bwd")


def _bn_backward(frozen, d_act, y, scale, shift, mean, invstd, gamma, dy_out, dgamma, dbeta, pool, want_sums):
    """The one body of bn_backward and bn_frozen_backward.  unetpp_bn_bwd_plan says how the pool gradient travels (inside
    the passes, or by a maxpool_bwd pass into d_act first) and how large the partial buffer is; then the pass or passes
    and the finalize."""
    lib = _lib.lib()
    n, h, w, c = y.shape
    bf16 = _is_bf16(y)
    if want_sums and dgamma is None:
        dgamma = torch.empty(c, dtype=torch.float32, device=y.device)
    if want_sums and dbeta is None:
        dbeta = torch.empty(c, dtype=torch.float32, device=y.device)
    d_pooled, pool_idx = (None, None) if pool is None else pool
    # every address once, in BnBwdQuery.POINTERS order: the plan looks at them, the launches get the same ones
    addr = [None if t is None else t.data_ptr()
            for t in (d_act, y, dy_out, scale, shift, mean, invstd, gamma, dgamma, dbeta, d_pooled, pool_idx)]
    plan = _lib.BnBwdSizes()
    rc = lib.unetpp_bn_bwd_plan(_lib.BnBwdQuery(frozen, bf16, want_sums, n, h, w, c, 0, *addr), plan)
    rows = plan.partial_rows
    if rows < 1 and (bf16 or frozen):
        raise ValueError("bf16 BatchNorm backward needs C = 8 * 2^k channels, got %d" % c)
    if rc != 0:  # a refused plan is reported under the name of the launch that used to refuse
        check(rc, "unetpp_maxpool_bwd" if pool is not None and not bf16 else
              "unetpp_bn_frozen_bwd" if frozen else "unetpp_bn_bwd_reduce" + ("_bf16" if bf16 else ""))
    a_dact, a_y, a_dy, a_scale, a_shift, a_mean, a_invstd, a_gamma, a_dgamma, a_dbeta, a_pooled, a_idx = addr
    route = plan.route
    if route == 2:
        maxpool_bwd(d_pooled, pool_idx, d_act)
        a_pooled = a_idx = None
    elif route == 1:
        _need(d_pooled, "d_pooled", y.dtype), _need(pool_idx, "pool_idx", torch.uint8)
    a_partial = None
    if want_sums:
        partial = torch.empty(plan.partial_floats, dtype=torch.float32, device=y.device)
        a_partial = partial.data_ptr()
    st = _stream()
    if frozen:
        fn = lib.unetpp_bn_frozen_bwd_bf16 if bf16 else lib.unetpp_bn_frozen_bwd
        _timed_call(None, 0.0, lambda: check(fn(a_dact, a_y, a_scale, a_shift, a_mean, a_invstd, a_pooled, a_idx, n, h, w, c,
                                                a_dy, a_partial, st), "unetpp_bn_frozen_bwd"),
                    (2.0 if bf16 else 4.0) * n * h * w * c * 3)
        if want_sums:
            check(lib.unetpp_bn_bwd_finalize(a_partial, rows, c, a_dgamma, a_dbeta, st), "unetpp_bn_bwd_finalize")
        return (dgamma, dbeta) if want_sums else (None, None)
    # the plain fp32 passes take a pixel count, the routing and the bf16 ones the pool pair (NULL: none) and the shape
    suffix = "_bf16" if bf16 else "_pool" if route == 1 else ""
    shape = (a_pooled, a_idx, n, h, w, c) if suffix else (n * h * w, c)
    check(getattr(lib, "unetpp_bn_bwd_reduce" + suffix)(a_dact, a_y, a_scale, a_shift, a_mean, a_invstd, *shape, a_partial, st),
          "unetpp_bn_bwd_reduce" + suffix)
    check(lib.unetpp_bn_bwd_finalize(a_partial, rows, c, a_dgamma, a_dbeta, st), "unetpp_bn_bwd_finalize")
    check(getattr(lib, "unetpp_bn_bwd_apply" + suffix)(a_dact, a_y, a_scale, a_shift, a_mean, a_invstd, a_gamma, a_dgamma, a_dbeta,
                                                       *shape, a_dy, st), "unetpp_bn_bwd_apply" + suffix)
    return dgamma, dbeta


def _bn_backward_bf16(d_act, y, scale, shift, mean, invstd, gamma, dy_out, dgamma, dbeta, pool):
    return _bn_backward(False, d_act, y, scale, shift, mean, invstd, gamma, dy_out, dgamma, dbeta, pool, True)


def bn_backward(d_act, y, scale, shift, mean, invstd, gamma, dy_out, dgamma=None, dbeta=None, pool=None):
    """Training-mode BatchNorm+ReLU backward.  Returns (dgamma, dbeta); dy_out may alias d_act.
    pool = (d_pooled, pool_idx): the gradient of the 2x2 max-pool of this activation, routed to the argmax while
    d_act is read (both passes) when the shape allows, else by a maxpool_bwd pass into d_act first."""
    return _bn_backward(False, d_act, y, scale, shift, mean, invstd, gamma, dy_out, dgamma, dbeta, pool, True)


def bn_frozen_backward(d_act, y, scale, shift, mean, invstd, dy_out, dgamma=None, dbeta=None, pool=None, want_sums=True):
    """BatchNorm+ReLU backward of a layer that normalised with its running statistics: dy = (y*scale+shift > 0) * g * scale
    in ONE streaming launch (g = d_act plus the routed pool gradient); dy_out may alias d_act.  want_sums: also dgamma =
    sum gg*xhat and dbeta = sum gg (per-workgroup rows + bn_bwd_finalize); returns (dgamma, dbeta), or (None, None) without
    sums (gamma and beta frozen too: mean / invstd may then be None).  pool = (d_pooled, pool_idx) as in bn_backward."""
    adt = torch.bfloat16 if _is_bf16(y) else torch.float32
    _need(d_act, "d_act", adt), _need(y, "y", adt), _need(dy_out, "dy", adt)
    if tuple(d_act.shape) != tuple(y.shape) or tuple(dy_out.shape) != tuple(y.shape):
        raise ValueError("d_act, y and dy must have one shape")
    if want_sums and (mean is None or invstd is None):
        raise ValueError("the gamma / beta sums need the running mean snapshot and invstd")
    return _bn_backward(True, d_act, y, scale, shift, mean, invstd, None, dy_out, dgamma, dbeta, pool, want_sums)


def head_fwd(x, weight, bias, p_drop, seed, mask, out_nchw, seed_dev=None):
    """seed_dev: optional one-element int64 device tensor added to `seed` when the kernel runs (graph-captured steps)"""
    n, h, w, c = x.shape
    n_cls = weight.shape[0]
    fn = _lib.lib().unetpp_head_fwd_bf16 if _is_bf16(x) else _lib.lib().unetpp_head_fwd
    check(fn(_ptr(x), _ptr(weight), _ptr(bias), n, h, w, c, n_cls, float(p_drop), C.c_uint64(seed), _ptr(mask),
             _ptr(seed_dev), _ptr(out_nchw), _stream()), "unetpp_head_fwd")


# A/B switch (measurements only): the composition of head_fwd launches and torch reductions instead of unetpp_head_mc
_FUSED_HEAD_MC = os.environ.get("UNETPP_NO_FUSED_HEAD_MC") is None


def mc_sample_seeds(seed: int, samples: int):
    """The seeds of the `samples` dropout draws of head_mc: seed + MC_SEED_STEP * k (mod 2^64), k = 0 .. samples-1."""
    return [(int(seed) + _lib.MC_SEED_STEP * k) & 0xFFFFFFFFFFFFFFFF for k in range(samples)]


def head_mc(x, weight, bias, p_drop, seed, samples, mean_out, var_out, seed_dev=None):
    """Monte-Carlo dropout at one head: mean_out and var_out (fp32 [N, n_cls, H, W]) over `samples` = K draws of the head's
    dropout, sample k being head_fwd(x, weight, bias, p_drop, mc_sample_seeds(seed, K)[k], None, ..., seed_dev):
        mean = (((s_0 + s_1) + ...) + s_{K-1}) / float(K)
        var  = (((d_0 d_0 + d_1 d_1) + ...) + d_{K-1} d_{K-1}) / float(K - 1),   d_k = s_k - mean   (unbiased)
    every operation rounded on its own, both quotients true divisions.  ONE launch that reads x once where the library
    takes the call (unetpp_head_mc: fp32 features on the streaming forward's shapes); otherwise -- other channel counts,
    bf16 features, UNETPP_NO_FUSED_HEAD_MC set -- K head_fwd launches and the same fold in torch elementwise ops, with the
    same bits wherever head_fwd runs the same kernel.  ValueError for samples outside 2..32 or p_drop outside (0, 1)."""
    if isinstance(samples, bool) or not isinstance(samples, int) or not 2 <= samples <= _lib.MC_MAX_SAMPLES:
        raise ValueError("samples must be an int in 2..%d, got %r" % (_lib.MC_MAX_SAMPLES, samples))
    p_drop = float(p_drop)
    if not 0.0 < p_drop < 1.0:
        raise ValueError("p_drop must lie in (0, 1): without dropout every sample is the same map, got %r" % p_drop)
    if x.dtype not in _ACT_DTYPES:
        raise TypeError("features must be float32 or bfloat16, got %s" % x.dtype)
    _need(x, "head features", x.dtype)
    n, h, w, c = x.shape
    n_cls = weight.shape[0]
    if tuple(_need(weight, "head weight").shape) != (n_cls, c) or _need(bias, "head bias").numel() != n_cls:
        raise ValueError("head weight must be [n_cls, C] and bias [n_cls]")
    for t, what in ((mean_out, "mean map"), (var_out, "variance map")):
        if tuple(_need(t, what).shape) != (n, n_cls, h, w):
            raise ValueError("mean and variance maps must be [N, n_cls, H, W]")
    if _FUSED_HEAD_MC and not _is_bf16(x):
        status = _lib.lib().unetpp_head_mc(_ptr(x), _ptr(weight), _ptr(bias), n, h, w, c, n_cls, p_drop, C.c_uint64(seed),
                                           _ptr(seed_dev), samples, _ptr(mean_out), _ptr(var_out), _stream())
        if status != -1:   # UNETPP_EINVAL: a refusal for the shape or an alignment, before anything ran
            check(status, "unetpp_head_mc")
            return
    # the composition: K maps, then the fold in the kernel's order.  (On the GPU torch divides by a Python scalar through
    # a multiplication with its reciprocal: the divisors are device tensors, so that both quotients are true divisions.)
    maps = torch.empty((samples, n, n_cls, h, w), dtype=torch.float32, device=x.device)
    for k, seed_k in enumerate(mc_sample_seeds(seed, samples)):
        head_fwd(x, weight, bias, p_drop, seed_k, None, maps[k], seed_dev=seed_dev)
    total = maps[0].clone()
    for k in range(1, samples):
        total.add_(maps[k])
    torch.div(total, torch.full((), float(samples), dtype=torch.float32, device=x.device), out=mean_out)
    d = torch.sub(maps[0], mean_out, out=total)
    squares = torch.mul(d, d)
    for k in range(1, samples):
        torch.sub(maps[k], mean_out, out=d)
        squares.add_(torch.mul(d, d, out=d))
    torch.div(squares, torch.full((), float(samples - 1), dtype=torch.float32, device=x.device), out=var_out)


def heads_mean_fwd(xs, weights, biases, out_nchw):
    """out_nchw [N, n_cls, H, W] fp32 = (((s_1 + s_2) + ...) + s_n) / float(n), s_h = sigmoid(bias_h + x_h . weight_h): the
    mean of n = len(xs) <= 8 sigmoid heads in ONE launch that reads every NHWC feature tensor xs[h] (all fp32, or all
    bf16) once and never writes the individual head maps.  weights[h] [n_cls, C], biases[h] [n_cls]; no dropout."""
    n_heads = len(xs)
    if not (1 <= n_heads <= _lib.MAX_HEADS) or len(weights) != n_heads or len(biases) != n_heads:
        raise ValueError("heads_mean_fwd takes 1..%d heads with one weight and one bias each" % _lib.MAX_HEADS)
    adt = xs[0].dtype
    if adt not in _ACT_DTYPES:
        raise TypeError("features must be float32 or bfloat16, got %s" % adt)
    n, h, w, c = xs[0].shape
    n_cls = weights[0].shape[0]
    d = _lib.HeadsMean()
    d.n_heads = n_heads
    for i, (x, wt, b) in enumerate(zip(xs, weights, biases)):
        if tuple(_need(x, "head features", adt).shape) != (n, h, w, c):
            raise ValueError("every head reads a feature tensor of the same shape")
        if tuple(_need(wt, "head weight").shape) != (n_cls, c) or _need(b, "head bias").numel() != n_cls:
            raise ValueError("head weight must be [n_cls, C] and bias [n_cls]")
        d.head[i].x, d.head[i].weight, d.head[i].bias = x.data_ptr(), wt.data_ptr(), b.data_ptr()
    if tuple(_need(out_nchw, "output").shape) != (n, n_cls, h, w):
        raise ValueError("output must be [N, n_cls, H, W]")
    fn = _lib.lib().unetpp_heads_mean_fwd_bf16 if adt == torch.bfloat16 else _lib.lib().unetpp_heads_mean_fwd
    check(fn(C.byref(d), n, h, w, c, n_cls, _ptr(out_nchw), _stream()), "unetpp_heads_mean_fwd")


def heads_mean_bwd(xs, weights, biases, d_out, dxs, accumulates, gates):
    """Backward of heads_mean_fwd: d_out [N, n_cls, H, W] fp32 is the gradient of the mean.  For every head h the kernel
    recomputes s_h = sigmoid(bias_h + x_h . weight_h) from the features (the forward never wrote the head maps), forms
    dl = (d_out * (1 / n)) * (s_h * (1 - s_h)) and writes dxs[h] = W_h^T dl (added to dxs[h] when accumulates[h]; then
    multiplied by (x_h > 0) when gates[h]).  Returns [(dW_h [n_cls, C, 1, 1], db_h [n_cls])], summed in a fixed order."""
    lib = _lib.lib()
    n_heads = len(xs)
    if not (1 <= n_heads <= _lib.MAX_HEADS) or not all(len(v) == n_heads for v in (weights, biases, dxs, accumulates, gates)):
        raise ValueError("heads_mean_bwd takes 1..%d heads with one weight, bias, dx, accumulate and gate each" % _lib.MAX_HEADS)
    adt = xs[0].dtype
    if adt not in _ACT_DTYPES:
        raise TypeError("features must be float32 or bfloat16, got %s" % adt)
    n, h, w, c = xs[0].shape
    n_cls = weights[0].shape[0]
    if tuple(_need(d_out, "gradient of the mean").shape) != (n, n_cls, h, w):
        raise ValueError("d_out must be [N, n_cls, H, W]")
    blocks = int(lib.unetpp_head_bwd_blocks(n * h * w))
    ln = n_cls * c + n_cls
    partial = torch.empty((n_heads, blocks * ln), dtype=torch.float32, device=d_out.device)
    sums = torch.empty((n_heads, ln), dtype=torch.float32, device=d_out.device)
    d, g = _lib.HeadsMean(), _lib.HeadsMeanGrad()
    d.n_heads = g.n_heads = n_heads
    for i, (x, wt, b, dx) in enumerate(zip(xs, weights, biases, dxs)):
        if tuple(_need(x, "head features", adt).shape) != (n, h, w, c) or tuple(_need(dx, "feature gradient", adt).shape) != (n, h, w, c):
            raise ValueError("every head reads a feature tensor and writes a gradient of the same shape")
        if tuple(_need(wt, "head weight").shape) != (n_cls, c) or _need(b, "head bias").numel() != n_cls:
            raise ValueError("head weight must be [n_cls, C] and bias [n_cls]")
        d.head[i].x, d.head[i].weight, d.head[i].bias = x.data_ptr(), wt.data_ptr(), b.data_ptr()
        g.head[i].dx, g.head[i].partial = dx.data_ptr(), partial[i].data_ptr()
        g.head[i].accumulate, g.head[i].gate_x = int(bool(accumulates[i])), int(bool(gates[i]))
    st = _stream()
    fn = lib.unetpp_heads_mean_bwd_bf16 if adt == torch.bfloat16 else lib.unetpp_heads_mean_bwd
    check(fn(C.byref(d), C.byref(g), _ptr(d_out), n, h, w, c, n_cls, st), "unetpp_heads_mean_bwd")
    out = []
    for i in range(n_heads):
        check(lib.unetpp_sum_partials(_ptr(partial[i]), blocks, ln, _ptr(sums[i]), st), "unetpp_sum_partials")
        out.append((sums[i, :n_cls * c].view(n_cls, c, 1, 1), sums[i, n_cls * c:]))
    return out


def head_bwd(d_out, out, x, weight, p_drop, seed, mask, dx, accumulate, gate_x=False, seed_dev=None):
    """Returns (dW [n_cls, C, 1, 1], db [n_cls]); dx is written or accumulated in place."""
    lib = _lib.lib()
    n, h, w, c = x.shape
    n_cls = weight.shape[0]
    blocks = int(lib.unetpp_head_bwd_blocks(n * h * w))
    ln = n_cls * c + n_cls
    partial = torch.empty(blocks * ln, dtype=torch.float32, device=x.device)
    sums = torch.empty(ln, dtype=torch.float32, device=x.device)
    st = _stream()
    fn = lib.unetpp_head_bwd_bf16 if _is_bf16(x) else lib.unetpp_head_bwd
    check(fn(_ptr(d_out), _ptr(out), _ptr(x), _ptr(weight), n, h, w, c, n_cls, float(p_drop), C.c_uint64(seed), _ptr(mask),
             _ptr(seed_dev), _ptr(dx), int(accumulate), int(gate_x), _ptr(partial), st), "unetpp_head_bwd")
    check(lib.unetpp_sum_partials(_ptr(partial), blocks, ln, _ptr(sums), st), "unetpp_sum_partials")
    return sums[:n_cls * c].view(n_cls, c, 1, 1), sums[n_cls * c:]


def head_train(x, weight, bias, target, rows, gamma, n_heads, p_drop, seed, mask, out_nchw, dx, gate_x=False,
               seed_dev=None, partial=None):
    """One head of a training step in ONE launch: head_fwd, this head's gradient of focal_bce_heads (the mean over
    `n_heads` against `target`) and head_bwd (accumulate = 0), bit for bit.  out_nchw and dx are written.
    -> (dW [n_cls, C, 1, 1], db [n_cls]), or None when the library refuses the call (anything but the fp32 power-of-two
    channel-quad form): nothing was launched and the caller runs the three launches.
    partial: the caller's unetpp_head_bwd_blocks(N*H*W) * (n_cls*C + n_cls) floats (tests read the rows)."""
    lib = _lib.lib()
    n, h, w, c = x.shape
    n_cls = weight.shape[0]
    if _is_bf16(x):
        return None
    _need(x, "head features"), _need(dx, "feature gradient"), _need(target, "target"), _need(out_nchw, "output")
    if tuple(dx.shape) != (n, h, w, c) or tuple(target.shape) != (n, n_cls, h, w) or tuple(out_nchw.shape) != (n, n_cls, h, w):
        raise ValueError("dx must be [N, H, W, C], target and output [N, n_cls, H, W]")
    blocks = int(lib.unetpp_head_bwd_blocks(n * h * w))
    ln = n_cls * c + n_cls
    if partial is None:
        partial = torch.empty(blocks * ln, dtype=torch.float32, device=x.device)
    elif _need(partial, "partial rows").numel() != blocks * ln:
        raise ValueError("partial must hold %d rows of %d floats" % (blocks, ln))
    st = _stream()
    status = lib.unetpp_head_train(_ptr(x), _ptr(weight), _ptr(bias), _ptr(target), n, h, w, c, n_cls, float(p_drop),
                                   C.c_uint64(seed), _ptr(mask), _ptr(seed_dev), int(rows), float(gamma), int(n_heads),
                                   _ptr(out_nchw), _ptr(dx), int(bool(gate_x)), _ptr(partial), st)
    if status == -1:   # UNETPP_EINVAL: a refusal, before anything ran
        return None
    check(status, "unetpp_head_train")
    sums = torch.empty(ln, dtype=torch.float32, device=x.device)
    check(lib.unetpp_sum_partials(_ptr(partial), blocks, ln, _ptr(sums), st), "unetpp_sum_partials")
    return sums[:n_cls * c].view(n_cls, c, 1, 1), sums[n_cls * c:]


def bilinear2x_fwd(x, y):
    n, h, w, c = x.shape
    if _is_bf16(x):
        check(_lib.lib().unetpp_bilinear2x_fwd_bf16(_ptr(x), n, h, w, c, _ptr(y), _stream()), "unetpp_bilinear2x_fwd_bf16")
        return
    check(_lib.lib().unetpp_bilinear2x_fwd(_ptr(x), n, h, w, c, _ptr(y), _stream()), "unetpp_bilinear2x_fwd")


def bilinear2x_bwd(dy, dx, accumulate, gate=None):
    """dx (+)= stencil^T(dy); bf16 storage: optionally followed by dx *= (gate > 0) (the node's ReLU mask)"""
    n, h, w, c = dx.shape
    if _is_bf16(dx):
        check(_lib.lib().unetpp_bilinear2x_bwd_bf16(_ptr(dy), n, h, w, c, _ptr(dx), int(accumulate), _ptr(gate), _stream()),
              "unetpp_bilinear2x_bwd_bf16")
        return
    if gate is not None:
        raise ValueError("the fused ReLU mask is a bf16-storage option")
    check(_lib.lib().unetpp_bilinear2x_bwd(_ptr(dy), n, h, w, c, _ptr(dx), int(accumulate), _stream()),
          "unetpp_bilinear2x_bwd")


def nchw_to_nhwc(src):
    n, c, h, w = src.shape
    _need(src, "input")
    if c == 1:
        return src.view(n, h, w, 1)  # same bytes
    dst = torch.empty((n, h, w, c), dtype=torch.float32, device=src.device)
    check(_lib.lib().unetpp_nchw_to_nhwc(_ptr(src), n, c, h, w, _ptr(dst), _stream()), "unetpp_nchw_to_nhwc")
    return dst


def nhwc_to_nchw(src):
    n, h, w, c = src.shape
    if c == 1:
        return src.view(n, 1, h, w)
    dst = torch.empty((n, c, h, w), dtype=torch.float32, device=src.device)
    check(_lib.lib().unetpp_nhwc_to_nchw(_ptr(src), n, c, h, w, _ptr(dst), _stream()), "unetpp_nhwc_to_nchw")
    return dst


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """The loss kernels read float4: a contiguous view whose storage offset leaves it off a 16-byte boundary is copied
    (the C ABI's alignment contract stays)."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def _loss_maps(preds, target: torch.Tensor):
    """The checks every loss makes on its maps -> (preds, target) on 16-byte boundaries."""
    _need(target, "target")
    for p in preds:
        _need(p, "pred")
        if p.shape != target.shape:
            raise ValueError("pred and target must have the same shape")
    return [_aligned16(p) for p in preds], _aligned16(target)


def _loss_heads(preds, target: torch.Tensor, want_grad: bool):
    """What the fused head losses share -> (aligned preds, aligned target, the filled FocalHeads, grads or None)."""
    if not 1 <= len(preds) <= _lib.MAX_HEADS:
        raise ValueError("1 to %d heads" % _lib.MAX_HEADS)
    preds, target = _loss_maps(preds, target)
    grads = [torch.empty_like(p) for p in preds] if want_grad else None
    hd = _lib.FocalHeads()
    hd.n_heads = len(preds)
    for i, p in enumerate(preds):
        hd.pred[i] = p.data_ptr()
        hd.grad[i] = grads[i].data_ptr() if want_grad else None
    return preds, target, hd, grads


def focal_bce(pred: torch.Tensor, target: torch.Tensor, rows: int, gamma: float, want_grad: bool = True):
    """FocalLoss_BCE_2d value (0-dim tensor) and d loss / d pred in one pass over (pred, target)."""
    lib = _lib.lib()
    (pred,), target = _loss_maps([pred], target)
    n = pred.numel()
    blocks = int(lib.unetpp_focal_bce_blocks(n))
    partial = torch.empty(blocks, dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    check(lib.unetpp_focal_bce(_ptr(pred), _ptr(target), n, rows, float(gamma), _ptr(grad), _ptr(partial), _ptr(loss),
                               _stream()), "unetpp_focal_bce")
    return loss.reshape(()), grad


def focal_bce_heads(preds, target: torch.Tensor, rows: int, gamma: float, want_grad: bool = True, ignore: bool = False):
    """The trainer's loop over the deep-supervision heads (criterion on every head, mean over heads) in one launch:
    -> (losses [1 + heads]: the mean, then every head's FocalLoss_BCE_2d value; d mean / d pred per head or None).
    Bit for bit what the loop computes with focal_bce and tensor arithmetic (tests/test_gpu_caller.py).
    ignore: a negative target element contributes +0.0 to loss and gradient (unetpp_focal_bce_heads_ignore)."""
    lib = _lib.lib()
    preds, target, hd, grads = _loss_heads(preds, target, want_grad)
    n = target.numel()
    blocks = int(lib.unetpp_focal_bce_blocks(n))
    partial = torch.empty(len(preds) * blocks, dtype=torch.float32, device=target.device)
    loss = torch.empty(1 + len(preds), dtype=torch.float32, device=target.device)
    fn = lib.unetpp_focal_bce_heads_ignore if ignore else lib.unetpp_focal_bce_heads
    check(fn(C.byref(hd), _ptr(target), n, rows, float(gamma), _ptr(partial), _ptr(loss), _stream()),
          "unetpp_focal_bce_heads_ignore" if ignore else "unetpp_focal_bce_heads")
    return loss, grads


def topk_focal_heads(preds, target: torch.Tensor, k: int, denom: int, gamma: float, want_grad: bool = True,
                     ignore: bool = False):
    """Top-k focal loss of every head against one target [..., H, W] (a row is one map of P = H*W pixels): per head and
    row only the min(k, P) pixels with the largest |pred - target| enter FocalLoss_BCE_2d, ties at the threshold taken in
    index order (csrc/topk_loss.hip: an exact radix select, one launch for all heads).
    -> (losses [1 + heads]: the mean over heads, then every head's value; d mean / d pred per head (+0.0 on every pixel
    that is not selected) or None; kth [heads, rows]: the k-th largest |pred - target| of every head and row).
    ignore: a negative target element has key 0 and contributes +0.0 (unetpp_topk_focal_heads_ignore)."""
    lib = _lib.lib()
    preds, target, hd, grads = _loss_heads(preds, target, want_grad)
    if target.dim() < 3:
        raise ValueError("target must be [..., H, W]")
    if int(k) < 1 or int(denom) < 1:
        raise ValueError("k and denom must be at least 1")
    pixels = target.shape[-2] * target.shape[-1]
    rows = target.numel() // max(pixels, 1)
    nbytes = int(lib.unetpp_topk_focal_workspace_bytes(len(preds), rows, pixels))
    if nbytes <= 0:
        raise ValueError("topk_focal_heads: %d rows of %d pixels are outside what the kernel takes" % (rows, pixels))
    workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=target.device)
    loss = torch.empty(1 + len(preds), dtype=torch.float32, device=target.device)
    kth = torch.empty(len(preds), rows, dtype=torch.float32, device=target.device)
    fn = lib.unetpp_topk_focal_heads_ignore if ignore else lib.unetpp_topk_focal_heads
    check(fn(C.byref(hd), _ptr(target), rows, pixels, int(k), int(denom), float(gamma), _ptr(workspace), _ptr(kth),
             _ptr(loss), _stream()), "unetpp_topk_focal_heads_ignore" if ignore else "unetpp_topk_focal_heads")
    return loss, grads, kth


def pr_focal_heads(preds, target: torch.Tensor, alpha: float, beta: float, eps: float, positive: float,
                   want_grad: bool = True, ignore: bool = False):
    """Penalty-reduced focal loss of every head against one target, normalised by the number of positives (t >=
    positive) of the target (csrc/pr_focal.hip: a count pass, the main pass, a finish; no read-back).
    -> (losses [1 + heads]: the mean over heads, then every head's value; d mean / d pred per head or None; n_pos: the
    number of positives, a 0-dim int64 tensor on the device).
    ignore: a negative target element contributes +0.0 to loss and gradient (unetpp_pr_focal_heads_ignore)."""
    lib = _lib.lib()
    preds, target, hd, grads = _loss_heads(preds, target, want_grad)
    n = target.numel()
    nbytes = int(lib.unetpp_pr_focal_workspace_bytes(len(preds), n))
    if nbytes <= 0:
        raise ValueError("pr_focal_heads: %d elements are outside what the kernel takes" % n)
    workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=target.device)
    loss = torch.empty(1 + len(preds), dtype=torch.float32, device=target.device)
    n_pos = torch.empty((), dtype=torch.int64, device=target.device)
    fn = lib.unetpp_pr_focal_heads_ignore if ignore else lib.unetpp_pr_focal_heads
    check(fn(C.byref(hd), _ptr(target), n, float(alpha), float(beta), float(eps), float(positive), _ptr(workspace),
             _ptr(n_pos), _ptr(loss), _stream()), "unetpp_pr_focal_heads_ignore" if ignore else "unetpp_pr_focal_heads")
    return loss, grads, n_pos


DISTILL_TEACHERS = {"last": _lib.DISTILL_LAST, "next": _lib.DISTILL_NEXT}
DISTILL_GATES = {"none": 0, "teacher_better": 1}


def distill_heads(preds, target: torch.Tensor, rows: int, gamma: float, weight_dev: torch.Tensor, teacher: str = "last",
                  gate: str = "none", want_grad: bool = True, ignore: bool = False, distill_ignored: bool = True):
    """focal_bce_heads with self-distillation across the heads (csrc/distill.hip, one call): every head but the deepest
    is also held against its teacher's map -- the deepest head ("last") or the next deeper one ("next"), read as data --
    by the same element rule, over the elements the gate ("none" / "teacher_better": where the teacher is closer to the
    target than the student) and the ignore rule admit; L_h = S_h + w D_h with w = weight_dev[0], read on the device.
    preds: shallow to deep.
    -> (losses [1 + heads]: the mean over heads of L_h, then every L_h; d mean / d pred per head or None;
    supervised [heads]: S_h, focal_bce_heads' values bit for bit; distill [heads]: D_h, +0.0 for the deepest head).
    ignore: a negative target element has a supervised term of +0.0, counts as having passed the gate, and keeps its
    distillation term iff distill_ignored."""
    if teacher not in DISTILL_TEACHERS:
        raise ValueError("teacher must be one of %s, got %r" % (sorted(DISTILL_TEACHERS), teacher))
    if gate not in DISTILL_GATES:
        raise ValueError("gate must be one of %s, got %r" % (sorted(DISTILL_GATES), gate))
    if not torch.is_tensor(weight_dev) or weight_dev.numel() != 1:
        raise ValueError("weight_dev must be a tensor of one element")
    if weight_dev.dtype != torch.float32:
        raise TypeError("weight_dev must be torch.float32, got %s" % weight_dev.dtype)
    if weight_dev.device != target.device:
        raise ValueError("weight_dev must live on the device of the target")
    lib = _lib.lib()
    preds, target, hd, grads = _loss_heads(preds, target, want_grad)
    heads, n = len(preds), target.numel()
    blocks = int(lib.unetpp_focal_bce_blocks(n))
    partial = torch.empty(2 * heads * blocks, dtype=torch.float32, device=target.device)
    loss = torch.empty(1 + 3 * heads, dtype=torch.float32, device=target.device)
    check(lib.unetpp_distill_heads(C.byref(hd), _ptr(target), n, rows, float(gamma), _ptr(weight_dev),
                                   DISTILL_TEACHERS[teacher], DISTILL_GATES[gate], int(bool(ignore)),
                                   int(bool(distill_ignored)), _ptr(partial), _ptr(loss), _stream()), "unetpp_distill_heads")
    return loss[:1 + heads], grads, loss[1 + heads:1 + 2 * heads], loss[1 + 2 * heads:]


def teacher_heads(preds, target: torch.Tensor, teacher: torch.Tensor, rows: int, gamma: float, weight_dev: torch.Tensor,
                  gate: str = "none", want_grad: bool = True, ignore: bool = False, distill_ignored: bool = True):
    """focal_bce_heads with distillation from one external map (csrc/distill.hip: unetpp_teacher_heads, one call): every
    head, the deepest included, is also held against `teacher` -- float32, of the target's shape, read as data -- by the
    same element rule, over the elements where the teacher exists (an element < 0 has none; -0.0 and a NaN are not
    negative) and that the gate and the ignore rule admit; L_h = S_h + w D_h with w = weight_dev[0], read on the device.
    -> (losses [1 + heads]: the mean over heads of L_h, then every L_h; d mean / d pred per head or None;
    supervised [heads]: S_h, focal_bce_heads' values bit for bit; distill [heads]: D_h).
    ignore: a negative target element has a supervised term of +0.0, counts as having passed the gate, and keeps its
    distillation term iff distill_ignored and the teacher exists there."""
    if gate not in DISTILL_GATES:
        raise ValueError("gate must be one of %s, got %r" % (sorted(DISTILL_GATES), gate))
    if not torch.is_tensor(weight_dev) or weight_dev.numel() != 1:
        raise ValueError("weight_dev must be a tensor of one element")
    if weight_dev.dtype != torch.float32:
        raise TypeError("weight_dev must be torch.float32, got %s" % weight_dev.dtype)
    if weight_dev.device != target.device:
        raise ValueError("weight_dev must live on the device of the target")
    if not torch.is_tensor(teacher):
        raise TypeError("teacher must be a tensor")
    if teacher.dtype != torch.float32:
        raise TypeError("teacher must be torch.float32, got %s" % teacher.dtype)
    if teacher.device != target.device:
        raise ValueError("teacher must live on the device of the target")
    if teacher.shape != target.shape:
        raise ValueError("teacher must have the shape of the target")
    lib = _lib.lib()
    preds, target, hd, grads = _loss_heads(preds, target, want_grad)
    teacher = _aligned16(_need(teacher, "teacher"))
    heads, n = len(preds), target.numel()
    blocks = int(lib.unetpp_focal_bce_blocks(n))
    partial = torch.empty(2 * heads * blocks, dtype=torch.float32, device=target.device)
    loss = torch.empty(1 + 3 * heads, dtype=torch.float32, device=target.device)
    check(lib.unetpp_teacher_heads(C.byref(hd), _ptr(target), _ptr(teacher), n, rows, float(gamma), _ptr(weight_dev),
                                   DISTILL_GATES[gate], int(bool(ignore)), int(bool(distill_ignored)), _ptr(partial),
                                   _ptr(loss), _stream()), "unetpp_teacher_heads")
    return loss[:1 + heads], grads, loss[1 + heads:1 + 2 * heads], loss[1 + 2 * heads:]


def create_heatmap(points: torch.Tensor, height: int, width: int, radius: float = 3.0) -> torch.Tensor:
    """points [N, P, 2] (x, y) fp32 on the GPU -> target heat maps [N, 4, H, W] (tools/misc/helper.py:87-172)."""
    lib = _lib.lib()
    _need(points, "points")
    if points.dim() != 3 or points.shape[2] != 2 or points.shape[1] < 6:
        raise ValueError("points must be [N, P >= 6, 2]")
    n, p = points.shape[0], points.shape[1]
    out = torch.empty(n, 4, height, width, dtype=torch.float32, device=points.device)
    ws = torch.empty(int(lib.unetpp_heatmap_workspace_bytes(n, height, width)), dtype=torch.uint8, device=points.device)
    check(lib.unetpp_create_heatmap(_ptr(points), n, p, height, width, float(radius), _ptr(out), _ptr(ws), _stream()),
          "unetpp_create_heatmap")
    return out


def heatmap_pattern(points: torch.Tensor, pattern, height: int, width: int, radius: float = 3.0) -> torch.Tensor:
    """points [N, P, 2] (x, y) fp32 on the GPU, pattern = list of lists of key-point indices -> [N, len(pattern), H, W]
    (tools/misc/heatmap.py:203-230)."""
    lib = _lib.lib()
    _need(points, "points")
    if points.dim() != 3 or points.shape[2] != 2:
        raise ValueError("points must be [N, P, 2]")
    n, p = points.shape[0], points.shape[1]
    flat = [i for hmap in pattern for i in hmap]
    if not flat or min(flat) < 0 or max(flat) >= p or any(len(h) == 0 for h in pattern):
        raise ValueError("pattern indexes key points 0..%d, every map needs at least one" % (p - 1))
    begins = [0]
    for hmap in pattern:
        begins.append(begins[-1] + len(hmap))
    mp = torch.tensor(flat, dtype=torch.int32, device=points.device)
    mb = torch.tensor(begins, dtype=torch.int32, device=points.device)
    out = torch.empty(n, len(pattern), height, width, dtype=torch.float32, device=points.device)
    ws = torch.empty(int(lib.unetpp_heatmap_pattern_workspace_bytes(n, len(pattern), height, width)), dtype=torch.uint8,
                     device=points.device)
    check(lib.unetpp_heatmap_pattern(_ptr(points), n, p, _ptr(mp), _ptr(mb), len(pattern), height, width, float(radius),
                                     _ptr(out), _ptr(ws), _stream()), "unetpp_heatmap_pattern")
    return out


def _keypoints_stages(heat, thr, num, max_regions, segmentation, ws, changed, points, counts, select=True):
    """the staged C-ABI calls of one extraction (include/unetpp_hip.h: unetpp_keypoints_extract)"""
    lib = _lib.lib()
    maps, h, w = heat.shape
    st = _stream()
    args = (_ptr(heat), maps, h, w, _ptr(thr), num, max_regions)

    def stage(k, what, sweeps=1):
        check(lib.unetpp_keypoints_extract(k, *args, sweeps, _ptr(ws), _ptr(changed), _ptr(points), _ptr(counts), st), what)

    def until_stable(k, what, sweeps):
        # A sweep moves a label / a distance at least one pixel along its path, and a path through a mask is at most
        # h * w / 2 pixels long (a one-pixel serpentine): that many sweeps bound the loop.  Every batch ends in a blocking
        # read-back, so the batches double (normally 2-3 of them suffice).
        done, limit = 0, h * w // 2 + sweeps
        while done < limit:
            changed.zero_()
            stage(k, what, sweeps)
            done += sweeps
            if int(changed.item()) == 0:
                return
            sweeps = min(2 * sweeps, 256)
        raise RuntimeError("keypoints_extract: %s did not converge" % what)

    stage(0, "keypoints mask")
    if segmentation == "watershed":
        stage(3, "keypoints distance init")
        until_stable(4, "keypoints distance sweeps", 8)
        stage(5, "keypoints cores")
    until_stable(1, "keypoints merge", 4)
    if segmentation == "watershed":
        stage(6, "keypoints markers")
        # The watershed's two levels: level-0 rounds until stable, one cross round (stage 9), level 0 again, until a cross
        # round moves nothing.  A cross round that moves something labels at least one pixel and no pixel is labelled
        # twice: h * w bounds the loop.  Stage 9 is the cross round and the first level-0 round after it in one batch
        # with one read-back (until_stable returns with the flag at 0, and a level-0 round on a stable state moves
        # nothing, so the flag says whether the cross round did): a batch without holes costs two launches and one read.
        for _ in range(h * w + 1):
            until_stable(7, "keypoints flood", 4)
            stage(9, "keypoints flood across the mask edge")
            if int(changed.item()) == 0:
                break
        else:
            raise RuntimeError("keypoints_extract: keypoints flood did not converge")
        stage(8, "keypoints regions")
    if select:
        stage(2, "keypoints select")


def keypoints_regions(heat: torch.Tensor, threshold: float = 0.5, segmentation: str = "watershed"):
    """heat [maps, H, W] fp32 on the GPU -> (labels int32 [maps, H, W]: the raster index of the region's first (core) pixel,
    -1 outside every region; distance int32 [maps, H, W]: the 3x3 chamfer distance in 16-bit fixed point, zeros for
    "components").  The region step of the extraction alone (region_segment_, tools/misc/heatmap.py:100-144, returns
    one boolean mask per region: ``labels == root`` here)."""
    lib = _lib.lib()
    _need(heat, "heat")
    if heat.dim() != 3:
        raise ValueError("heat must be [maps, H, W]")
    if segmentation not in ("watershed", "components"):
        raise ValueError("segmentation must be 'watershed' or 'components'")
    maps, h, w = heat.shape
    dev, hw = heat.device, h * w
    ws = torch.zeros(int(lib.unetpp_keypoints_workspace_bytes(maps, h, w, 1)), dtype=torch.uint8, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    points = torch.empty(maps, 1, 2, dtype=torch.float32, device=dev)
    counts = torch.empty(maps, dtype=torch.int32, device=dev)
    thr = torch.full((maps,), float(threshold), dtype=torch.float32, device=dev)
    _keypoints_stages(heat, thr, 1, 1, segmentation, ws, changed, points, counts, select=False)
    ints = ws[maps * hw * 8 + maps * 16:].view(torch.int32)   # workspace: best u64 [maps*hw], cand u64 [maps*max_regions*2], label, dist, marker
    return ints[:maps * hw].view(maps, h, w).clone(), ints[maps * hw:2 * maps * hw].view(maps, h, w).clone()


def keypoints_extract(heat: torch.Tensor, num: int, threshold: float = 0.5, max_regions: int = 4096,
                      segmentation: str = "watershed"):
    """heat [maps, H, W] fp32 on the GPU -> (points [maps, num, 2] as (x, y), -1 padded; counts [maps] regions found).
    tools/misc/heatmap.py:148-200; a map without any region is retried once at 0.9 * threshold (heatmap.py:176-198).
    segmentation="watershed": the reference's region step (region_segment_, heatmap.py:100-144) -- chamfer distance
    cores grown back through the binary mask, touching blobs split, coreless blobs dropped; "components": a region is
    an 8-connected component of the mask (the round-2 stand-in).  max_regions sizes the fast ranking buffer only: maps
    with more regions are selected exactly over all of them (no failure mode the reference does not have)."""
    lib = _lib.lib()
    _need(heat, "heat")
    if heat.dim() != 3:
        raise ValueError("heat must be [maps, H, W]")
    if segmentation not in ("watershed", "components"):
        raise ValueError("segmentation must be 'watershed' or 'components'")
    maps, h, w = heat.shape
    dev = heat.device
    ws = torch.empty(int(lib.unetpp_keypoints_workspace_bytes(maps, h, w, max_regions)), dtype=torch.uint8, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    points = torch.empty(maps, num, 2, dtype=torch.float32, device=dev)
    counts = torch.empty(maps, dtype=torch.int32, device=dev)
    thr = torch.full((maps,), float(threshold), dtype=torch.float32, device=dev)

    def run():
        _keypoints_stages(heat, thr, num, max_regions, segmentation, ws, changed, points, counts)

    run()
    # one small read-back per call: are there maps without any region?  (the sweeps above already read a flag back
    # every few iterations; everything else -- mask, labels, peaks, the exact top-`num` selection over ALL regions --
    # stays on the device, and there is no limit on the number of regions: kp_select_kernel)
    if bool((counts == 0).any()):  # retry the empty maps at 0.9 * threshold; the others keep their result
        keep_points, keep_counts = points.clone(), counts.clone()
        empty = (counts == 0)
        thr = torch.where(empty, thr * 0.9, thr)
        run()
        points = torch.where(empty.view(-1, 1, 1), points, keep_points)
        counts = torch.where(empty, counts, keep_counts)
    return points, counts


def check_match_pattern(pattern, n_labels: int) -> None:
    """The matcher's limits on a pattern (list of lists of label indices), checked on the host before any launch."""
    flat = [i for hmap in pattern for i in hmap]
    if not pattern:
        raise ValueError("the pattern needs at least one map")
    if any(len(hmap) > _lib.MATCH_MAX for hmap in pattern):
        raise ValueError("a map of the pattern holds at most %d key points" % _lib.MATCH_MAX)
    if any(not 0 <= int(i) < n_labels for i in flat):
        raise ValueError("pattern indexes labels 0..%d (labels are [N, %d, 2])" % (n_labels - 1, n_labels))
    if len(set(flat)) != len(flat):
        raise ValueError("a label index appears twice in the pattern")


@functools.lru_cache(maxsize=16)
def _pattern_tensors(pattern, device):
    begins = [0]
    for hmap in pattern:
        begins.append(begins[-1] + len(hmap))
    flat = [i for hmap in pattern for i in hmap] or [0]
    mp = torch.tensor(flat, dtype=torch.int32, device=device)
    mb = torch.tensor(begins, dtype=torch.int32, device=device)
    return mp, mb, mb[1:] - mb[:-1]


def match_pattern_tensors(pattern, device):
    """(map_points, map_begin, lengths) of a pattern as device int32 tensors, uploaded once per pattern and device."""
    return _pattern_tensors(tuple(tuple(int(i) for i in hmap) for hmap in pattern), torch.device(device))


def match_points(points: torch.Tensor, found: torch.Tensor, labels: torch.Tensor, pattern, heads: int = 1):
    """Min-distance matching of extracted key points to labels and the landmark loss, every head in one launch
    (include/unetpp_hip.h: unetpp_match_points; the rule and the summation order are in csrc/validate.hip).
    points [heads*N*C, K, 2] (x, y) fp32, found [heads*N*C] int32 (predictions per map), labels [N, S, 2] fp32, pattern =
    C lists of label indices -> (matched [heads, N, S, 2] fp32, (-1, -1) where unmatched; mask [heads, N, S] bool;
    loss [heads] fp32: MSELoss over the matched coordinates, NaN when none; count [heads] int32)."""
    if points.dim() != 3 or points.shape[2] != 2:
        raise ValueError("points must be [maps, K, 2]")
    if labels.dim() != 3 or labels.shape[2] != 2:
        raise ValueError("labels must be [N, S, 2]")
    n, s = int(labels.shape[0]), int(labels.shape[1])
    c, k = len(pattern), int(points.shape[1])
    check_match_pattern(pattern, s)
    if heads < 1 or points.shape[0] != heads * n * c or tuple(found.shape) != (heads * n * c,):
        raise ValueError("points [heads*N*C, K, 2] and found [heads*N*C] for %d heads, N = %d, C = %d" % (heads, n, c))
    if not 1 <= k <= _lib.MATCH_MAX:
        raise ValueError("1 to %d points per map" % _lib.MATCH_MAX)
    _need(points, "points")
    _need(found, "found", torch.int32)
    _need(labels, "labels")
    lib = _lib.lib()
    dev = labels.device
    mp, mb, _ = match_pattern_tensors(pattern, dev)
    matched = torch.empty(heads, n, s, 2, dtype=torch.float32, device=dev)
    mask = torch.empty(heads, n, s, dtype=torch.bool, device=dev)
    loss = torch.empty(heads, dtype=torch.float32, device=dev)
    count = torch.empty(heads, dtype=torch.int32, device=dev)
    check(lib.unetpp_match_points(_ptr(points), _ptr(found), heads, n, c, k, _ptr(labels), s, _ptr(mp), _ptr(mb),
                                  _ptr(matched), _ptr(mask), _ptr(loss), _ptr(count), _stream()), "unetpp_match_points")
    return matched, mask, loss, count


def warp_batch(store: torch.Tensor, index: torch.Tensor, params: torch.Tensor, out_size, mul: torch.Tensor,
               add: torch.Tensor, fill: float = 0.0, labels: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None):
    """One launch: gather index [N] from the store (uint8 [M, Hs, Ws, C] or float32 [M, C, Hs, Ws]), warp by params
    [N, 16], normalise by mul / add [C] -> float32 [N, C, Ho, Wo]; with labels [M, S, 2] also (labels_out [N, S, 2],
    inside [N, S] uint8) (include/unetpp_hip.h: unetpp_warp_batch).  out: a contiguous float32 [N, C, Ho, Wo] to write."""
    u8, m, hs, ws, c = _frame_store(store)
    if not 1 <= c <= _lib.WARP_MAX_C:
        raise ValueError("a store has 1 to %d channels, got %d" % (_lib.WARP_MAX_C, c))
    _need(index, "index", torch.int64)
    _need(params, "params")
    _need(mul, "mul")
    _need(add, "add")
    n = _window_rows(index, params)
    if tuple(mul.shape) != (c,) or tuple(add.shape) != (c,):
        raise ValueError("mul and add must be [%d]" % c)
    ho, wo = int(out_size[0]), int(out_size[1])
    dev = store.device
    if out is None:
        out = torch.empty(n, c, ho, wo, dtype=torch.float32, device=dev)
    elif tuple(_need(out, "out").shape) != (n, c, ho, wo):
        raise ValueError("out must be [%d, %d, %d, %d]" % (n, c, ho, wo))
    s, labels_out, inside = 0, None, None
    if labels is not None:
        _need(labels, "labels")
        if labels.dim() != 3 or labels.shape[0] != m or labels.shape[2] != 2:
            raise ValueError("labels must be [M, S, 2] with the store's M")
        s = int(labels.shape[1])
        labels_out = torch.empty(n, s, 2, dtype=torch.float32, device=dev)
        inside = torch.empty(n, s, dtype=torch.uint8, device=dev)
    nbytes = 4.0 * n * c * ho * wo + (1 if u8 else 4) * float(n) * c * min(hs * ws, ho * wo) + 17.0 * n * s
    _timed_call("warp_batch", 0.0, lambda: check(_lib.lib().unetpp_warp_batch(
        _ptr(store), _lib.STORE_U8 if u8 else _lib.STORE_F32, m, hs, ws, c, _ptr(index), n, _ptr(params), _ptr(mul),
        _ptr(add), float(fill), _ptr(out), ho, wo, _ptr(labels), s, _ptr(labels_out), _ptr(inside), _stream()),
        "unetpp_warp_batch"), nbytes)
    return out if labels is None else (out, labels_out, inside)


def augment_draw(n: int, seed: int, src_size, out_size, desc: "_lib.AugmentDesc", device) -> torch.Tensor:
    """params [n, 16] drawn on the device from a 64-bit seed (include/unetpp_hip.h: unetpp_augment_draw)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the parameter table is drawn on the GPU: this path has no CPU fallback")
    params = torch.empty(int(n), _lib.WARP_PARAMS, dtype=torch.float32, device=device)
    check(_lib.lib().unetpp_augment_draw(_ptr(params), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(src_size[0]),
                                         int(src_size[1]), int(out_size[0]), int(out_size[1]), C.byref(desc), _stream()),
          "unetpp_augment_draw")
    return params


def scene_rects(rows) -> torch.Tensor:
    """Host table for scene_stitch: rows of (frame, oy, ox, y_lo, y_hi, x_lo, x_hi) -> int32 [n, 8] (CPU, the layout of
    struct unetpp_scene_rect); frame < 0 marks a padding tile."""
    t = torch.zeros(len(rows), 8, dtype=torch.int32)
    if len(rows):
        t[:, :7] = torch.tensor([[int(v) for v in r] for r in rows], dtype=torch.int32).reshape(len(rows), 7)
    return t


def scene_stitch(tiles: torch.Tensor, rects: torch.Tensor, rects_dev: torch.Tensor, variants, out: torch.Tensor) -> None:
    """One launch: out [S, C, H, W] fp32 gets, on every tile's owned rectangle, the mean over the K dihedral variants of
    tiles [n, K, C, Th, Tw] fp32, each read at the inverse-transformed position (include/unetpp_hip.h:
    unetpp_scene_stitch).  rects: the int32 [n, 8] table of scene_rects on the host, rects_dev the same rows on the
    device; variants: the K variant codes.  Pixels no tile of the call owns are left as they are."""
    _need(tiles, "tiles")
    _need(out, "out")
    if tiles.dim() != 5 or out.dim() != 4 or out.shape[1] != tiles.shape[2]:
        raise ValueError("tiles must be [n, K, C, Th, Tw] and out [S, C, H, W] with the same C")
    n, k, c, th, tw = (int(v) for v in tiles.shape)
    codes = [int(v) for v in variants]
    if len(codes) != k or not 1 <= k <= _lib.SCENE_MAX_VARIANTS:
        raise ValueError("one variant code per variant, 1 to %d variants; got %d codes for K = %d"
                         % (_lib.SCENE_MAX_VARIANTS, len(codes), k))
    if rects.is_cuda or rects.dtype != torch.int32 or tuple(rects.shape) != (n, 8) or not rects.is_contiguous():
        raise ValueError("rects must be a contiguous CPU int32 [%d, 8] table (ops.scene_rects)" % n)
    _need(rects_dev, "rects_dev", torch.int32)
    if tuple(rects_dev.shape) != (n, 8) or rects_dev.device != tiles.device or out.device != tiles.device:
        raise ValueError("rects_dev must be int32 [%d, 8] on the device of tiles and out" % n)
    s, _, h, w = (int(v) for v in out.shape)
    host = C.cast(C.c_void_p(rects.data_ptr()), C.POINTER(_lib.SceneRect))
    nbytes = 0.0
    if _TIMER is not None:   # K reads and one write per owned pixel and class
        nbytes = 4.0 * (k + 1) * c * float((rects[:, 4] - rects[:, 3]).clamp_min(0).mul(rects[:, 6] - rects[:, 5]).sum())
    _timed_call("scene_stitch", 0.0, lambda: check(_lib.lib().unetpp_scene_stitch(
        _ptr(tiles), n, k, c, th, tw, (C.c_int32 * k)(*codes), host, _ptr(rects_dev), _ptr(out), s, h, w, _stream()),
        "unetpp_scene_stitch"), nbytes)


def scene_screen(maps: torch.Tensor, rects: torch.Tensor, rects_dev: torch.Tensor, threshold: float):
    """One launch: maps [S, C, H, W] fp32 -> (active int32 [n], score float32 [n]) on the device, one entry per row of the
    table: over all classes and all pixels of the row's rectangle [y_lo, y_hi) x [x_lo, x_hi), active = any(!(v <
    threshold)) (a value equal to the threshold and a NaN both activate) and score = fmax of the values, -inf when all
    are NaN (include/unetpp_hip.h: unetpp_scene_screen).  rects: the int32 [n, 8] table of scene_rects on the host,
    rects_dev the same rows on the device; a padding row (frame < 0) gives (0, -inf).  Nothing is read back."""
    _need(maps, "maps")
    if maps.dim() != 4:
        raise ValueError("maps must be [S, C, H, W]")
    n = int(rects.shape[0]) if rects.dim() == 2 else -1
    if rects.is_cuda or rects.dtype != torch.int32 or n < 1 or tuple(rects.shape) != (n, 8) or not rects.is_contiguous():
        raise ValueError("rects must be a contiguous CPU int32 [n, 8] table with n >= 1 (ops.scene_rects)")
    _need(rects_dev, "rects_dev", torch.int32)
    if tuple(rects_dev.shape) != (n, 8) or rects_dev.device != maps.device:
        raise ValueError("rects_dev must be int32 [%d, 8] on the device of maps" % n)
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold must not be NaN")
    s, c, h, w = (int(v) for v in maps.shape)
    dev = maps.device
    if not bool((rects[:, 0] >= 0).any()):   # nothing but padding rows: the library launches nothing
        return (torch.zeros(n, dtype=torch.int32, device=dev),
                torch.full((n,), float("-inf"), dtype=torch.float32, device=dev))
    active = torch.empty(n, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    host = C.cast(C.c_void_p(rects.data_ptr()), C.POINTER(_lib.SceneRect))
    nbytes = 0.0
    if _TIMER is not None:   # one read per class and pixel of every rectangle
        live = rects[rects[:, 0] >= 0]
        nbytes = 4.0 * c * float((live[:, 4] - live[:, 3]).clamp_min(0).mul(live[:, 6] - live[:, 5]).sum())
    _timed_call("scene_screen", 0.0, lambda: check(_lib.lib().unetpp_scene_screen(
        _ptr(maps), s, c, h, w, host, _ptr(rects_dev), n, threshold, _ptr(active), _ptr(score), _stream()),
        "unetpp_scene_screen"), nbytes)
    return active, score


def peaks_detect(maps: torch.Tensor, threshold: float, radius: int, cap: int, refine: bool = True):
    """maps [M, H, W] fp32 on the GPU -> (xy [M, cap, 2] as (x, y), score [M, cap], count [M] int32): the local maxima of
    every map that reach `threshold`, in raster order (include/unetpp_hip.h: unetpp_peaks_detect; rule, sub-pixel
    offset and order guarantee in csrc/detect.hip).  count may exceed cap: the first cap peaks in raster order are
    kept; rows k >= min(count, cap) are xy = -1, score = -inf.  Three launches, nothing is read back."""
    _need(maps, "maps")
    if maps.dim() != 3:
        raise ValueError("maps must be [M, H, W]")
    m, h, w = (int(v) for v in maps.shape)
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= _lib.PEAKS_MAX_RADIUS:
        raise ValueError("radius must be an int in 1..%d, got %r" % (_lib.PEAKS_MAX_RADIUS, radius))
    if isinstance(cap, bool) or not isinstance(cap, int) or cap < 1:
        raise ValueError("cap must be a positive int, got %r" % (cap,))
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold must not be NaN")
    if m < 1 or h < 1 or w < 1 or m > _lib.PEAKS_MAX_MAPS or h >= (1 << 24) or w >= (1 << 24):
        raise ValueError("1 to %d non-empty maps with sides below 2^24 (coordinates are carried in fp32), got %dx%dx%d"
                         % (_lib.PEAKS_MAX_MAPS, m, h, w))
    lib = _lib.lib()
    dev = maps.device
    nbytes = int(lib.unetpp_peaks_workspace_bytes(m, h, w))
    if nbytes <= 0:
        raise ValueError("maps of %dx%dx%d are beyond what one call takes" % (m, h, w))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    xy = torch.empty(m, cap, 2, dtype=torch.float32, device=dev)
    score = torch.empty(m, cap, dtype=torch.float32, device=dev)
    count = torch.empty(m, dtype=torch.int32, device=dev)
    _timed_call("peaks_detect", 0.0, lambda: check(lib.unetpp_peaks_detect(
        _ptr(maps), m, h, w, threshold, radius, 1 if refine else 0, cap, _ptr(xy), _ptr(score), _ptr(count), _ptr(ws),
        _stream()), "unetpp_peaks_detect"), 4.0 * m * h * w)
    return xy, score, count


def detect_match(xy: torch.Tensor, n_pred: torch.Tensor, order: torch.Tensor, labels: torch.Tensor,
                 label_class: torch.Tensor, tolerance: float):
    """Detections against labels, one launch (include/unetpp_hip.h: unetpp_detect_match).  xy [S, C, cap, 2] fp32,
    n_pred [S, C] int32 (predictions of the group), order [S, C, cap] int32 (the slots in the order they are served),
    labels [S, L, 2] fp32, label_class [S, L] int32 (-1: padding) -> (pred_label [S, C, cap] int32: the label a
    prediction took or -1; label_pred [S, L] int32: the slot that took the label or -1; stats [S, C, 3] int32: true
    positives, false positives, false negatives).  Each prediction in turn takes the nearest unspent label of its
    (frame, class) within `tolerance`, ties to the lowest label index."""
    _need(xy, "xy")
    _need(n_pred, "n_pred", torch.int32)
    _need(order, "order", torch.int32)
    _need(labels, "labels")
    _need(label_class, "label_class", torch.int32)
    if xy.dim() != 4 or xy.shape[3] != 2:
        raise ValueError("xy must be [S, C, cap, 2]")
    s, c, cap = (int(v) for v in xy.shape[:3])
    if tuple(n_pred.shape) != (s, c) or tuple(order.shape) != (s, c, cap):
        raise ValueError("n_pred must be [%d, %d] and order [%d, %d, %d]" % (s, c, s, c, cap))
    if labels.dim() != 3 or labels.shape[0] != s or labels.shape[2] != 2:
        raise ValueError("labels must be [%d, L, 2]" % s)
    n_labels = int(labels.shape[1])
    if tuple(label_class.shape) != (s, n_labels):
        raise ValueError("label_class must be [%d, %d]" % (s, n_labels))
    if min(s, c, cap, n_labels) < 1:
        raise ValueError("S, C, cap and L must be positive (pad an empty label list with one label of class -1)")
    tolerance = float(tolerance)
    if not tolerance >= 0.0:
        raise ValueError("tolerance must be a non-negative number, got %r" % (tolerance,))
    dev = xy.device
    if any(t.device != dev for t in (n_pred, order, labels, label_class)):
        raise ValueError("all tensors must live on one device")
    pred_label = torch.empty(s, c, cap, dtype=torch.int32, device=dev)
    label_pred = torch.empty(s, n_labels, dtype=torch.int32, device=dev)
    stats = torch.empty(s, c, 3, dtype=torch.int32, device=dev)
    _timed_call("detect_match", 0.0, lambda: check(_lib.lib().unetpp_detect_match(
        _ptr(xy), _ptr(n_pred), _ptr(order), s, c, cap, _ptr(labels), _ptr(label_class), n_labels, tolerance,
        _ptr(pred_label), _ptr(label_pred), _ptr(stats), _stream()), "unetpp_detect_match"))
    return pred_label, label_pred, stats


def points_target(labels: torch.Tensor, label_class: torch.Tensor, index: torch.Tensor, params: torch.Tensor,
                  n_classes: int, out_size, radius: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch: the target maps [N, n_classes, Ho, Wo] fp32 of N warped windows from labels [M, L, 2] fp32 as (x, y),
    label_class [M, L] int32, index [N] int64 and the warp's params [N, 16]: per class exp(-0.5 d / radius) of the distance
    d to the nearest valid label under the sample's forward map, 0 where the class has none (include/unetpp_hip.h:
    unetpp_points_target).  out: a contiguous float32 [N, n_classes, Ho, Wo] to write."""
    _need(labels, "labels")
    _need(label_class, "label_class", torch.int32)
    _need(index, "index", torch.int64)
    _need(params, "params")
    m, n_labels = _label_table(labels, label_class)
    n = _window_rows(index, params)
    c, (ho, wo) = int(n_classes), (int(out_size[0]), int(out_size[1]))
    radius = float(radius)
    if not radius > 0.0:
        raise ValueError("radius must be a positive number, got %r" % (radius,))
    if min(m, n_labels, n, ho, wo) < 1 or not 1 <= c <= 65535:
        raise ValueError("M, L, N and the window must be positive and n_classes in 1..65535 (pad an empty label list "
                         "with one label of class -1)")
    dev = labels.device
    if any(t.device != dev for t in (label_class, index, params)):
        raise ValueError("all tensors must live on one device")
    if out is None:
        out = torch.empty(n, c, ho, wo, dtype=torch.float32, device=dev)
    elif tuple(_need(out, "out").shape) != (n, c, ho, wo) or out.device != dev:
        raise ValueError("out must be [%d, %d, %d, %d] on the labels' device" % (n, c, ho, wo))
    _timed_call("points_target", 0.0, lambda: check(_lib.lib().unetpp_points_target(
        _ptr(labels), _ptr(label_class), m, n_labels, _ptr(index), n, _ptr(params), c, ho, wo, radius, _ptr(out),
        _stream()), "unetpp_points_target"), 4.0 * n * c * ho * wo)
    return out


def _ignore_rows(target: torch.Tensor, index: torch.Tensor, params: torch.Tensor):
    """(N, C, Ho, Wo) of a target [N, C, Ho, Wo] and the check of the warp rows index / params that belong to it."""
    _need(target, "target")
    _need(index, "index", torch.int64)
    _need(params, "params")
    if target.dim() != 4:
        raise ValueError("target must be [N, C, Ho, Wo]")
    n, c, ho, wo = (int(v) for v in target.shape)
    _window_rows(index, params, n)
    return n, c, ho, wo


def _ignore_frames(m, n_frames, things: str, tensors, target: torch.Tensor, src_size):
    """(M, Hs, Ws) of an ignore launch.  m: the table's M, else n_frames; things: its rows' name; tensors: on target's device."""
    if m is None or (n_frames is not None and int(n_frames) != m):
        raise ValueError("the number of frames: give n_frames without %s, and the %s' own M with them" % (things, things))
    if any(t.device != target.device for t in tensors):
        raise ValueError("all tensors must live on one device")
    hs, ws = int(src_size[0]), int(src_size[1])
    if min(int(m), hs, ws, *target.shape) < 1 or target.shape[1] > 65535:
        raise ValueError("N, the window and the frame must be positive and C in 1..65535")
    return int(m), hs, ws


def target_ignore(target: torch.Tensor, rects: Optional[torch.Tensor], rect_class: Optional[torch.Tensor],
                  index: torch.Tensor, params: torch.Tensor, src_size, outside: bool = False,
                  n_frames: Optional[int] = None) -> torch.Tensor:
    """One launch: writes -1.0 into the ignored elements of target [N, C, Ho, Wo] fp32, in place, and returns it.  rects
    [M, R, 4] fp32 as (x0, y0, x1, y1) in source pixels with rect_class [M, R] int32 (-1: every class), or None / R = 0
    for no rectangles -- then n_frames says how many frames there are (an index outside [0, M) is an all-fill sample);
    index [N] int64 and params [N, 16]: the rows of the warp; src_size = (Hs, Ws); outside: also mark what lies outside
    the frame (include/unetpp_hip.h: unetpp_target_ignore).  Nothing else of target is touched."""
    n, c, ho, wo = _ignore_rows(target, index, params)
    m, r = n_frames, 0
    if rects is not None and rects.numel() > 0:
        _need(rects, "rects")
        _need(rect_class, "rect_class", torch.int32)
        if rects.dim() != 3 or rects.shape[2] != 4 or tuple(rect_class.shape) != tuple(rects.shape[:2]):
            raise ValueError("rects must be [M, R, 4] and rect_class [M, R]")
        m, r = int(rects.shape[0]), int(rects.shape[1])
    elif rects is not None and rects.dim() == 3 and rects.shape[0] > 0:
        m = int(rects.shape[0])
    m, hs, ws = _ignore_frames(m, n_frames, "rectangles", (index, params) + ((rects, rect_class) if r else ()), target, src_size)
    _timed_call("target_ignore", 0.0, lambda: check(_lib.lib().unetpp_target_ignore(
        _ptr(rects) if r else None, _ptr(rect_class) if r else None, m, r, _ptr(index), n, _ptr(params), c, ho, wo, hs, ws,
        1 if outside else 0, _ptr(target), _stream()), "unetpp_target_ignore"), 4.0 * n * c * ho * wo)
    return target


def mask_pack(mask: torch.Tensor) -> torch.Tensor:
    """One launch: packs a raster mask [..., H, W] (bool, uint8 or float32; another type is compared with zero first)
    into bit planes int32 [..., H, ceil(W / 32)]: bit x & 31 of word x >> 5 is pixel x, set iff the pixel is non-zero (a
    NaN is, -0.0 is not); tail bits are zero (include/unetpp_hip.h: unetpp_mask_pack)."""
    if not mask.is_cuda:
        raise RuntimeError("mask must live on the GPU: this path has no CPU fallback")
    if mask.dim() < 2:
        raise ValueError("mask must be [..., H, W]")
    if mask.dtype == torch.bool:
        src, kind = mask.contiguous().view(torch.uint8), _lib.MASK_U8
    elif mask.dtype == torch.uint8:
        src, kind = mask.contiguous(), _lib.MASK_U8
    elif mask.dtype == torch.float32:
        src, kind = mask.contiguous(), _lib.MASK_F32
    else:
        src, kind = (mask != 0).contiguous().view(torch.uint8), _lib.MASK_U8
    w = int(mask.shape[-1])
    rows = int(mask.numel()) // max(w, 1)
    if w < 1 or rows < 1:
        raise ValueError("mask must hold at least one pixel")
    if rows * w > 2 ** 31 - 1:
        raise ValueError("a mask of more than 2^31 - 1 pixels must be packed in parts")
    bits = torch.empty(tuple(mask.shape[:-1]) + ((w + 31) // 32,), dtype=torch.int32, device=mask.device)
    _timed_call("mask_pack", 0.0, lambda: check(_lib.lib().unetpp_mask_pack(
        _ptr(src), kind, rows, w, _ptr(bits), _stream()), "unetpp_mask_pack"), float(src.element_size() * rows * w))
    return bits


def mask_polygons(vertices: torch.Tensor, counts: torch.Tensor, poly_plane: torch.Tensor, poly_clear: torch.Tensor,
                  planes: int, size) -> torch.Tensor:
    """One launch: rasterises polygon rings into bit planes int32 [S, planes, H, ceil(W / 32)] by the polygon rule of
    ignore.py.  vertices [S, G, V, 2] fp32 as (x, y); counts, poly_plane, poly_clear int32 [S, G]; size = (H, W); G may
    be 0 (include/unetpp_hip.h: unetpp_mask_polygons)."""
    _need(vertices, "vertices")
    if vertices.dim() != 4 or vertices.shape[3] != 2:
        raise ValueError("vertices must be [S, G, V, 2]")
    s, g, v = (int(x) for x in vertices.shape[:3])
    for t, what in ((counts, "counts"), (poly_plane, "poly_plane"), (poly_clear, "poly_clear")):
        _need(t, what, torch.int32)
        if tuple(t.shape) != (s, g):
            raise ValueError("%s must be [%d, %d]" % (what, s, g))
        if t.device != vertices.device:
            raise ValueError("all tensors must live on one device")
    h, w, p = int(size[0]), int(size[1]), int(planes)
    if min(s, p, h, w) < 1:
        raise ValueError("S, the planes and the frame must be positive")
    bits = torch.empty(s, p, h, (w + 31) // 32, dtype=torch.int32, device=vertices.device)
    some = g > 0
    _timed_call("mask_polygons", 0.0, lambda: check(_lib.lib().unetpp_mask_polygons(
        _ptr(vertices) if some and v > 0 else None, _ptr(counts) if some else None, _ptr(poly_plane) if some else None,
        _ptr(poly_clear) if some else None, s, g, v, p, h, w, _ptr(bits), _stream()), "unetpp_mask_polygons"),
        4.0 * bits.numel())
    return bits


def target_ignore_mask(target: torch.Tensor, bits: Optional[torch.Tensor], plane_class: Optional[torch.Tensor],
                       index: torch.Tensor, params: torch.Tensor, src_size, outside: bool = False,
                       n_frames: Optional[int] = None) -> torch.Tensor:
    """One launch: ``target_ignore`` with bit planes in place of rectangles.  Writes -1.0 into target [N, C, Ho, Wo] fp32,
    in place, where the pixel's source position is ignored by the lookup rule of ignore.py, and returns it.  bits int32
    [M, P, Hs, ceil(Ws / 32)] with plane_class int32 [P], or None / P = 0 for the `outside` rule alone -- then n_frames
    says how many frames there are; index [N] int64, params [N, 16]; src_size = (Hs, Ws) must be the planes' size
    (include/unetpp_hip.h: unetpp_target_ignore_mask)."""
    n, c, ho, wo = _ignore_rows(target, index, params)
    hs, ws = int(src_size[0]), int(src_size[1])
    m, p = n_frames, 0
    if bits is not None and bits.numel() > 0:
        _need(bits, "bits", torch.int32)
        _need(plane_class, "plane_class", torch.int32)
        if bits.dim() != 4 or plane_class.dim() != 1 or int(plane_class.numel()) != int(bits.shape[1]):
            raise ValueError("bits must be [M, P, Hs, ceil(Ws / 32)] and plane_class [P]")
        if int(bits.shape[2]) != hs or int(bits.shape[3]) != (ws + 31) // 32:
            raise ValueError("bits %s do not hold frames of src_size %d x %d" % (tuple(bits.shape), hs, ws))
        m, p = int(bits.shape[0]), int(bits.shape[1])
    elif bits is not None and bits.dim() == 4 and bits.shape[0] > 0:
        m = int(bits.shape[0])
    m, hs, ws = _ignore_frames(m, n_frames, "planes", (index, params) + ((bits, plane_class) if p else ()), target, src_size)
    _timed_call("target_ignore_mask", 0.0, lambda: check(_lib.lib().unetpp_target_ignore_mask(
        _ptr(bits) if p else None, _ptr(plane_class) if p else None, m, p, hs, ws, _ptr(index), n, _ptr(params), c, ho, wo,
        1 if outside else 0, _ptr(target), _stream()), "unetpp_target_ignore_mask"), 4.0 * n * c * ho * wo)
    return target


def crops_draw(n: int, seed: int, n_frames: int, src_size, out_size, centre_frame: Optional[torch.Tensor],
               centre_xy: Optional[torch.Tensor], p_object: float, jitter, desc: "_lib.AugmentDesc", device):
    """One launch: n windows of out_size in n_frames frames of src_size drawn from a 64-bit seed -> (params [n, 16] fp32,
    index [n] int64, origin [n, 2] int32 as (ox, oy)) on the device.  centre_frame [V] int32 / centre_xy [V, 2] fp32: the
    table object windows are centred on (None or V = 0: every window is uniform) (include/unetpp_hip.h:
    unetpp_crops_draw)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("windows are drawn on the GPU: this path has no CPU fallback")
    v = 0
    if centre_frame is not None and centre_frame.numel() > 0:
        _need(centre_frame, "centre_frame", torch.int32)
        _need(centre_xy, "centre_xy")
        v = int(centre_frame.numel())
        if centre_frame.dim() != 1 or tuple(centre_xy.shape) != (v, 2):
            raise ValueError("centre_frame must be [V] and centre_xy [V, 2]")
        if centre_frame.device != device or centre_xy.device != device:
            raise ValueError("the centre table must live on %s" % device)
    n = int(n)
    params = torch.empty(n, _lib.WARP_PARAMS, dtype=torch.float32, device=device)
    index = torch.empty(n, dtype=torch.int64, device=device)
    origin = torch.empty(n, 2, dtype=torch.int32, device=device)
    check(_lib.lib().unetpp_crops_draw(
        _ptr(params), _ptr(index), _ptr(origin), n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(n_frames), int(src_size[0]),
        int(src_size[1]), int(out_size[0]), int(out_size[1]), _ptr(centre_frame) if v else None,
        _ptr(centre_xy) if v else None, v, float(p_object), float(jitter[0]), float(jitter[1]), C.byref(desc), _stream()),
        "unetpp_crops_draw")
    return params, index, origin


def _paste_sources(src_frame: torch.Tensor, src_xy: torch.Tensor, src_class: torch.Tensor, dev) -> int:
    _need(src_frame, "src_frame", torch.int32)
    _need(src_xy, "src_xy")
    _need(src_class, "src_class", torch.int32)
    t = int(src_frame.numel())
    if t < 1 or src_frame.dim() != 1 or tuple(src_xy.shape) != (t, 2) or tuple(src_class.shape) != (t,):
        raise ValueError("the source table is src_frame [T], src_xy [T, 2] and src_class [T] with T >= 1")
    if any(v.device != dev for v in (src_frame, src_xy, src_class)):
        raise ValueError("the source table must live on %s" % dev)
    return t


def _paste_radius(patch_radius: int) -> int:
    r = int(patch_radius)
    if not 0 <= r <= _lib.PASTE_MAX_RADIUS:
        raise ValueError("patch_radius must lie in 0..%d, got %r" % (_lib.PASTE_MAX_RADIUS, patch_radius))
    return r


def paste_draw(max_pastes: int, seed: int, src_frame: torch.Tensor, src_xy: torch.Tensor, src_class: torch.Tensor,
               labels: torch.Tensor, label_class: torch.Tensor, index: torch.Tensor, params: torch.Tensor,
               n_classes: int, src_size, out_size, p: float, patch_radius: int, clearance: float, dihedral: bool = True):
    """One launch: what is pasted where in N windows, K = max_pastes slots each -> (src [N, K] int32: the row of the
    source table or -1, dst [N, K, 2] int32 as (px, py), code [N, K] int32, xy [N, K, 2] fp32: the pasted label, cls
    [N, K] int32: its class or -1) on the device.  src_frame [T] int32, src_xy [T, 2] fp32, src_class [T] int32: the
    source table; labels, label_class, index, params: as points_target takes them (include/unetpp_hip.h:
    unetpp_paste_draw)."""
    _need(labels, "labels")
    _need(label_class, "label_class", torch.int32)
    _need(index, "index", torch.int64)
    _need(params, "params")
    dev = params.device
    t = _paste_sources(src_frame, src_xy, src_class, dev)
    m, n_labels = _label_table(labels, label_class)
    k, r = int(max_pastes), _paste_radius(patch_radius)
    n = _window_rows(index, params)
    if any(v.device != dev for v in (labels, label_class, index)):
        raise ValueError("all tensors must live on one device")
    if not 1 <= k <= _lib.PASTE_MAX_SLOTS:
        raise ValueError("max_pastes must lie in 1..%d, got %r" % (_lib.PASTE_MAX_SLOTS, max_pastes))
    c, (hs, ws), (ho, wo) = int(n_classes), (int(src_size[0]), int(src_size[1])), (int(out_size[0]), int(out_size[1]))
    if min(m, n_labels, n, hs, ws) < 1 or not 1 <= c <= 65535 or min(ho, wo) < 2 * r + 1:
        raise ValueError("M, L, N and the frame must be positive, n_classes in 1..65535 and the window at least "
                         "%d on both sides" % (2 * r + 1))
    p, clearance = float(p), float(clearance)
    if not p >= 0.0 or not clearance >= 0.0:
        raise ValueError("p and clearance must not be negative")
    src = torch.empty(n, k, dtype=torch.int32, device=dev)
    dst = torch.empty(n, k, 2, dtype=torch.int32, device=dev)
    code = torch.empty(n, k, dtype=torch.int32, device=dev)
    xy = torch.empty(n, k, 2, dtype=torch.float32, device=dev)
    cls = torch.empty(n, k, dtype=torch.int32, device=dev)
    check(_lib.lib().unetpp_paste_draw(
        _ptr(src), _ptr(dst), _ptr(code), _ptr(xy), _ptr(cls), n, k, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(src_frame),
        _ptr(src_xy), _ptr(src_class), t, _ptr(labels), _ptr(label_class), m, n_labels, _ptr(index), _ptr(params), c, hs,
        ws, ho, wo, p, r, clearance, 1 if dihedral else 0, _stream()), "unetpp_paste_draw")
    return src, dst, code, xy, cls


def paste_apply(inputs: torch.Tensor, src: torch.Tensor, dst: torch.Tensor, code: torch.Tensor, src_frame: torch.Tensor,
                src_xy: torch.Tensor, src_class: torch.Tensor, store: torch.Tensor, params: torch.Tensor,
                mul: torch.Tensor, add: torch.Tensor, alpha: torch.Tensor, n_classes: int) -> torch.Tensor:
    """One launch: blends the patches of the rows (src [N, K], dst [N, K, 2], code [N, K], all int32) into inputs
    [N, C, Ho, Wo] fp32, in place, and returns it.  store: the frames as warp_batch takes them; params [N, 16]: the
    windows' gain and bias; alpha [2R+1, 2R+1] fp32: the blend weights.  Rows of any content are safe: one that names no
    patch inside its frame and window is skipped (include/unetpp_hip.h: unetpp_paste_apply)."""
    _need(inputs, "inputs")
    for name, v in (("src", src), ("dst", dst), ("code", code)):
        _need(v, name, torch.int32)
    for name, v in (("params", params), ("mul", mul), ("add", add), ("alpha", alpha)):
        _need(v, name)
    u8, m, hs, ws, cin = _frame_store(store, "store must be a contiguous 4-d tensor and inputs [N, C, Ho, Wo]")
    if inputs.dim() != 4:
        raise ValueError("store must be a contiguous 4-d tensor and inputs [N, C, Ho, Wo]")
    n, ci, ho, wo = (int(v) for v in inputs.shape)
    dev = inputs.device
    t = _paste_sources(src_frame, src_xy, src_class, dev)
    if ci != cin or not 1 <= cin <= _lib.WARP_MAX_C:
        raise ValueError("inputs and the store must have the same 1 to %d channels" % _lib.WARP_MAX_C)
    if src.dim() != 2 or src.shape[0] != n or tuple(dst.shape) != tuple(src.shape) + (2,) or code.shape != src.shape:
        raise ValueError("src [N, K], dst [N, K, 2] and code [N, K] for inputs of N = %d windows" % n)
    k = int(src.shape[1])
    side = int(alpha.shape[0]) if alpha.dim() == 2 else 0
    if side < 1 or side % 2 == 0 or tuple(alpha.shape) != (side, side):
        raise ValueError("alpha must be [2R+1, 2R+1]")
    r = _paste_radius(side // 2)
    if tuple(params.shape) != (n, _lib.WARP_PARAMS) or tuple(mul.shape) != (cin,) or tuple(add.shape) != (cin,):
        raise ValueError("params [N, %d], mul and add [%d]" % (_lib.WARP_PARAMS, cin))
    c = int(n_classes)
    if min(m, n, ho, wo, hs, ws) < 1 or not 1 <= k <= _lib.PASTE_MAX_SLOTS or not 1 <= c <= 65535:
        raise ValueError("sizes must be positive, K in 1..%d and n_classes in 1..65535" % _lib.PASTE_MAX_SLOTS)
    if any(v.device != dev for v in (src, dst, code, store, params, mul, add, alpha)):
        raise ValueError("all tensors must live on one device")
    _timed_call(None, 0.0, lambda: check(_lib.lib().unetpp_paste_apply(
        _ptr(inputs), n, k, cin, ho, wo, _ptr(src), _ptr(dst), _ptr(code), _ptr(src_frame), _ptr(src_xy), _ptr(src_class),
        t, _ptr(store), _lib.STORE_U8 if u8 else _lib.STORE_F32, m, hs, ws, c, _ptr(params), _ptr(mul), _ptr(add),
        _ptr(alpha), r, _stream()), "unetpp_paste_apply"), (9.0 if u8 else 12.0) * n * k * cin * side * side)
    return inputs


def paste_target(target: torch.Tensor, xy: torch.Tensor, cls: torch.Tensor, radius: float) -> torch.Tensor:
    """One launch: folds the pasted labels xy [N, K, 2] fp32 of class cls [N, K] int32 (outside [0, C): no label) into
    target [N, C, Ho, Wo] fp32, in place, and returns it: per live class exp(-0.5 d / radius) of the distance to the
    nearest pasted label, stored where it exceeds a target that is not negative -- what points_target would have written
    with those labels in the frame's list (include/unetpp_hip.h: unetpp_paste_target)."""
    _need(target, "target")
    _need(xy, "xy")
    _need(cls, "cls", torch.int32)
    if target.dim() != 4:
        raise ValueError("target must be [N, C, Ho, Wo]")
    n, c, ho, wo = (int(v) for v in target.shape)
    if cls.dim() != 2 or cls.shape[0] != n or tuple(xy.shape) != tuple(cls.shape) + (2,):
        raise ValueError("xy [N, K, 2] and cls [N, K] for a target of N = %d windows" % n)
    k = int(cls.shape[1])
    radius = float(radius)
    if not radius > 0.0:
        raise ValueError("radius must be a positive number, got %r" % (radius,))
    if min(n, ho, wo) < 1 or not 1 <= k <= _lib.PASTE_MAX_SLOTS or not 1 <= c <= 65535:
        raise ValueError("N and the window must be positive, K in 1..%d and C in 1..65535" % _lib.PASTE_MAX_SLOTS)
    if xy.device != target.device or cls.device != target.device:
        raise ValueError("all tensors must live on one device")
    _timed_call("paste_target", 0.0, lambda: check(_lib.lib().unetpp_paste_target(
        _ptr(target), n, k, c, ho, wo, _ptr(xy), _ptr(cls), radius, _stream()), "unetpp_paste_target"),
        8.0 * n * c * ho * wo)
    return target
