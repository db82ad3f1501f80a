"""No kernel of the path reads memory that this pass did not write.

Workspaces (BatchNorm partial rows, weight-gradient slabs, head partials), activations and gradient buffers are
``torch.empty``: whatever the allocator hands out.  Eager, the caching allocator makes that "the bytes of an earlier
tensor"; inside a captured HIP graph (graph.GraphedTrainStep, serving.GraphedForward) it is the graph's private pool, i.e.
the previous REPLAY's bytes -- a kernel that sums a row no workgroup wrote, or a border the staging did not fill, gives
plausible-looking and run-dependent numbers there (the class of failure of GPUTEST_r04).  The test runs the reference's
step body (trainer/trainer.py:114-136) twice from the same state: once as it is, once with every ``torch.empty`` /
``torch.empty_like`` of the package POISONED (NaN for floating storage, 0xFF.. for integers; a second run poisons with a
large finite value, which also survives compare-and-select masking of NaN), and a third and fourth time with every
tensor of the step -- workspaces, activations, gradients, parameters, buffers, inputs, targets, masks -- placed between
two GUARD BANDS of the same filling, so that a read before the first or behind the last element of any tensor lands in
poison instead of in a neighbouring allocation -- outputs, loss, BatchNorm buffers and every gradient must be
bit-identical and finite.  Self-comparison, not parity: it runs after the oracle / golden tests.

And no kernel WRITES memory that is not its own.  A vector store over a row tail, or a workspace whose carve-up on the
device disagrees with the size query the Python layer allocated from, lands in a neighbouring allocation or in allocator
slack and every output still compares equal; GPU sanitizers are not available for this path.  So the allocator of
tests/guard_alloc.py registers every guarded tensor with a copy of its two bands, and after each guarded run
``violations()`` reads the bands back byte by byte and ``changed_operands()`` compares every read-only operand (inputs,
targets, masks, and the parameters where nothing updates them) with the tensor it was copied from.  In a guarded run
``torch.zeros`` / ``zeros_like`` / ``full`` / ``full_like`` / ``ones`` are wrapped beside ``torch.empty`` /
``empty_like`` (flags, counters, -inf score rows, padded buffers), and bool and float64 storage is poisoned and banded
like the rest.  Each front runs under both poisons, because a stray write of the very bytes a band holds is invisible
under that poison.  LIMIT: the bands are GUARD_BYTES = 8192 bytes wide; a write further away than that is not seen.

Fronts under the regime: the three earlier ones (train_step with FocalLoss_BCE_2d and SGD over nine network structures,
the eval forward, the classic UNet step) and, through ``check_contained``: the fused AdamW (clipping, non-finite skip)
with WeightAverager, AdaBound, SGDW; the top-k, penalty-reduced, self-distillation and teacher losses with ignored
elements; train_step(head=J); frozen BatchNorm; the fused head_train pass; infer / infer_mc; SceneInference (call,
detect, uncertainty) and CascadeSceneInference; PeakDetector and evaluate; transfer_points, keypoints_extract in both
carve-ups of its workspace, validate_step; DeviceLoader, SceneCrops with ObjectPaste and the ignore union, the target heat
maps; clip_grad_norm_, the autograd form of the ensemble mean, the gradient of the network input, and the two-call
convolution + BatchNorm finalize by direct ``ops`` calls (no front reaches those two entry points any more).  A test on
the device plants single bytes into the bands of real allocations of the package and expects them reported.
The last test asserts that every launching entry point of the C ABI was called inside a guarded run.  Captured
graphs are outside: their allocations come from the graph's private pool during capture.
"""
import contextlib
import copy

import pytest
import torch

from tests import guard_alloc as ga
from tests.guard_alloc import GUARD_BYTES, guarded, poisoned_empty  # noqa: F401

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _assert_contained(what):
    """After torch.cuda.synchronize(): no guard band of this run was written, no read-only operand changed."""
    bad = ga.violations()
    assert bad == [], "%s: %d writes outside a tensor, e.g. %s" % (what, len(bad), bad[:6])
    changed = ga.changed_operands()
    assert changed == [], "%s: read-only operands were written: %s" % (what, changed[:6])


def _state(model, outs, loss):
    d = {"loss": loss.detach().clone()}
    for i, o in enumerate(outs):
        d["out%d" % i] = o.detach().clone()
    for k, p in model.named_parameters():
        d["grad/" + k] = p.grad.detach().clone()
    for k, b in model.named_buffers():
        d["buf/" + k] = b.detach().clone()
    return d


CASES = [
    # (id, constructor, bf16, batch, H, W, model class)
    ("f32-fs4-64", dict(in_channels=1, n_classes=4, feature_scale=4), False, 2, 64, 64),
    ("f32-fs1-96x160", dict(in_channels=1, n_classes=4, feature_scale=1), False, 3, 96, 160),
    ("f32-bilinear-nobn", dict(in_channels=3, n_classes=5, feature_scale=4, is_deconv=False, is_batchnorm=False), False, 2, 48, 80),
    ("f32-d5", dict(in_channels=3, n_classes=5, feature_scale=4, depth=5), False, 2, 64, 96),
    ("f32-d2", dict(in_channels=1, n_classes=4, feature_scale=4, depth=2), False, 4, 64, 64),
    ("bf16-bilinear-fs2-64", dict(in_channels=1, n_classes=4, feature_scale=2, is_deconv=False), True, 2, 64, 64),  # GPUTEST_r04's case
    ("bf16-fs1-128x96", dict(in_channels=1, n_classes=4, feature_scale=1), True, 3, 128, 96),
    ("bf16-d5-base64", dict(in_channels=3, n_classes=5, feature_scale=1, depth=5), True, 1, 96, 48),
    ("bf16-nobn", dict(in_channels=1, n_classes=4, feature_scale=2, is_batchnorm=False), True, 2, 64, 96),
]


@pytest.mark.parametrize("name,ctor,bf16,b,h,w", CASES, ids=[c[0] for c in CASES])
def test_no_launch_reads_unwritten_memory(dev, name, ctor, bf16, b, h, w):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet_Nested, train_step
    torch.manual_seed(17)
    base = UNet_Nested(**ctor).to(dev).train()
    if bf16:
        base.set_activation_dtype(BF)
    base.drop_out.p = 0.4
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    g = torch.Generator().manual_seed(23)
    x = torch.randn(b, ctor["in_channels"], h, w, generator=g).to(dev)
    t = torch.rand(b, ctor["n_classes"], h, w, generator=g).to(dev)
    masks = [(torch.rand(b, h, w, base.filters[0], generator=g) >= 0.4).to(torch.uint8).to(dev)   # NHWC keep-masks
             for _ in range(base.depth - 1)]

    def run(poison, guard=False):
        ga.reset()
        m = copy.deepcopy(base)
        xx, tt, mm = x, t, masks
        if guard:   # parameters, buffers, inputs, targets and masks between guard bands as well
            with torch.no_grad():
                for k, p in m.named_parameters():       # lr = 0: the step leaves every parameter as it is
                    p.data = guarded(p.data, poison, name=k, readonly=True)
                for k, p in m.named_buffers():
                    p.data = guarded(p.data, poison, name=k)
            xx, tt = guarded(x, poison, name="x", readonly=True), guarded(t, poison, name="target", readonly=True)
            mm = [guarded(k, poison, name="mask%d" % i, readonly=True) for i, k in enumerate(masks)]
        m.dropout_masks = mm                  # explicit masks: the runs draw no seeds
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        ctx = contextlib.nullcontext() if poison is None else guarded_regime(poison, guard)
        with ctx:
            train_step(m, opt, crit, xx, tt)    # first pass: records the weight-image jobs
            outs, loss = train_step(m, opt, crit, xx, tt)
        torch.cuda.synchronize()
        if guard:
            _assert_contained("poison %r" % poison)
        ga.reset()
        return _state(m, outs, loss)

    ref = run(None)
    for k, v in ref.items():
        assert torch.isfinite(v.float()).all(), k
    for poison, guard in ((float("nan"), False), (3.0e30, False), (float("nan"), True), (3.0e30, True)):
        got = run(poison, guard)
        bad = [k for k in ref if not torch.equal(ref[k], got[k])]
        assert not bad, "poison %r (guard bands: %s) changes %d tensors, e.g. %s" % (poison, guard, len(bad), bad[:6])


def test_eval_forward_reads_no_unwritten_memory(dev):
    from unet_nested4tiny_objects_keypoints_amd import UNet, UNet_Nested
    torch.manual_seed(3)
    for make, bf16, shape in ((lambda: UNet_Nested(in_channels=1, n_classes=4, feature_scale=2), False, (2, 1, 64, 96)),
                              (lambda: UNet_Nested(in_channels=1, n_classes=4, feature_scale=2), True, (2, 1, 64, 96)),
                              (lambda: UNet(n_classes=5, n_channels=3), False, (1, 3, 40, 56))):
        m = make().to(dev).eval()
        if bf16:
            m.set_activation_dtype(BF)
        x = torch.randn(*shape, device=dev)
        with torch.no_grad():
            ref = m(x)
            ref = ref if isinstance(ref, tuple) else (ref,)
            for poison, guard in ((float("nan"), False), (3.0e30, False), (float("nan"), True), (3.0e30, True)):
                ga.reset()
                with guarded_regime(poison, guard):
                    got = m(guarded(x, poison, name="x", readonly=True) if guard else x)
                got = got if isinstance(got, tuple) else (got,)
                for p, q in zip(ref, got):
                    assert torch.equal(p, q)
                if guard:
                    torch.cuda.synchronize()
                    _assert_contained("poison %r" % poison)
                ga.reset()


@pytest.mark.parametrize("name,ctor,bf16", [
    ("bf16-bilinear-fs2", dict(in_channels=1, n_classes=4, feature_scale=2, is_deconv=False), True),   # GPUTEST_r04's network
    ("bf16-deconv-fs2", dict(in_channels=1, n_classes=4, feature_scale=2), True),                       # dgrad into 32 channels: one column tile
    ("f32-fs2", dict(in_channels=1, n_classes=4, feature_scale=2), False),
], ids=lambda v: v if isinstance(v, str) else None)
def test_the_step_is_reproducible_run_to_run(dev, name, ctor, bf16):
    """Every tensor of a training step -- all activations kept for backward, BatchNorm coefficients, outputs, loss,
    every gradient -- is bit-identical from run to run, back to back and from an idle device (no floating-point
    atomics on the path; every cross-workgroup sum has a fixed order).  This is the comparison that found the cause of
    GPUTEST_r04: one 256-pixel x 32-column unit of the bilinear path's 1x1 convolution differed in ~1 of 100 steps
    (profiles/r5/gputest_r04_root_cause.txt).  Twelve runs per regime: a guard, not a stress loop."""
    import time

    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet_Nested
    torch.manual_seed(81)
    m = UNet_Nested(**ctor).to(dev).train()
    if bf16:
        m.set_activation_dtype(BF)
    m.drop_out.p = 0.0
    m._debug_keep_saved = True
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 1, 64, 64, generator=g).to(dev)
    t = torch.rand(2, 4, 64, 64, generator=g).to(dev)
    running = [b.clone() for b in m.buffers()]

    def one_step():
        for p in m.parameters():
            p.grad = None
        outs = m(x)
        loss = sum(crit(o, t) for o in outs) / len(outs)
        s = m._debug_saved
        got = {}
        for key, r in s.pairs.items():
            for nm in ("y1", "a1", "y2", "out", "pooled", "pool_idx"):
                v = getattr(r, nm)
                if v is not None:
                    got["X%d%d.%s" % (key + (nm,))] = v.clone()
        for key, u in s.ups.items():
            for nm in ("interp", "up"):
                v = getattr(u, nm)
                if v is not None:
                    got["up%d%d.%s" % (key + (nm,))] = v.clone()
        for i, o in enumerate(outs):
            got["out%d" % i] = o.detach().clone()
        got["loss"] = loss.detach().clone()
        loss.backward()
        for k, p in m.named_parameters():
            got["grad/" + k] = p.grad.clone()
        with torch.no_grad():
            for b, v in zip(m.buffers(), running):
                b.copy_(v)
        torch.cuda.synchronize()
        return got

    def bits(v):
        return v.view(torch.int16) if v.dtype == BF else v

    ref = one_step()
    for i in range(24):
        if i >= 12:
            time.sleep(0.01)    # idle start
        got = one_step()
        bad = [k for k in ref if not torch.equal(bits(ref[k]), bits(got[k]))]
        assert not bad, "run %d: %d tensors differ, first %s" % (i, len(bad), bad[:4])


def test_classic_unet_step_reads_no_unwritten_memory_and_is_reproducible(dev):
    """The same two properties for the classic UNet (models/unet.py:8-117; engine_unet.py schedules the same kernels,
    plus floor pooling / zero padding of odd sizes): poisoned + guard-banded allocations change nothing, and eight runs
    of the step give bit-identical outputs, loss and gradients."""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet
    torch.manual_seed(29)
    base = UNet(n_classes=5, n_channels=3, widths=(16, 32, 64, 128, 128)).to(dev).train()
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 3, 40, 56, generator=g).to(dev)       # not a multiple of 16: the reference's padding path
    t = torch.rand(2, 5, 40, 56, generator=g).to(dev)

    def run(poison=None, guard=False):
        ga.reset()
        m = copy.deepcopy(base)
        xx, tt = x, t
        if guard:
            with torch.no_grad():
                for k, p in m.named_parameters():       # no optimizer: nothing writes a parameter
                    p.data = guarded(p.data, poison, name=k, readonly=True)
                for k, p in m.named_buffers():
                    p.data = guarded(p.data, poison, name=k)
            xx, tt = guarded(x, poison, name="x", readonly=True), guarded(t, poison, name="target", readonly=True)
        ctx = contextlib.nullcontext() if poison is None else guarded_regime(poison, guard)
        with ctx:
            for _ in range(2):
                for p in m.parameters():
                    p.grad = None
                out = m(xx)
                loss = crit(out, tt)
                loss.backward()
        torch.cuda.synchronize()
        if guard:
            _assert_contained("poison %r" % poison)
        d = {"out": out.detach().clone(), "loss": loss.detach().clone()}
        d.update({"grad/" + k: p.grad.clone() for k, p in m.named_parameters()})
        ga.reset()
        return d

    ref = run()
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
    for poison, guard in ((float("nan"), False), (3.0e30, True), (float("nan"), True)):
        got = run(poison, guard)
        bad = [k for k in ref if not torch.equal(ref[k], got[k])]
        assert not bad, "poison %r (guard bands: %s): %s" % (poison, guard, bad[:6])
    for i in range(8):
        if i % 2:
            torch.cuda.synchronize()
        got = run()
        bad = [k for k in ref if not torch.equal(ref[k], got[k])]
        assert not bad, "run %d: %s" % (i, bad[:6])


# ---------------------------------------------------------------------------------------------------------------------
# Write containment on every front: one helper, one case per front
# ---------------------------------------------------------------------------------------------------------------------
POISONS = (float("nan"), 3.0e30)
PACKAGE = "unet_nested4tiny_objects_keypoints_amd"
CALLS = {}              # entry point of the library -> calls made while a guarded run was active
_REGIME = [None]        # the poison of the guarded run that is active, None in a plain run


@contextlib.contextmanager
def counting_calls():
    """Counts, per entry point of _lib.SIGNATURES, the calls made through the loaded library inside the block."""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    handle = _lib.lib()
    real = {name: getattr(handle, name) for name in _lib.SIGNATURES}

    def counted(name, fn):
        def call(*args):
            CALLS[name] = CALLS.get(name, 0) + 1
            return fn(*args)
        return call

    for name, fn in real.items():
        setattr(handle, name, counted(name, fn))
    try:
        yield
    finally:
        for name, fn in real.items():
            setattr(handle, name, fn)


@contextlib.contextmanager
def guarded_regime(poison, guard=True):
    """poisoned_empty(poison, guard); with guard bands the library's entry points are counted as covered."""
    with poisoned_empty(poison, guard):
        if guard:
            with counting_calls():
                yield
        else:
            yield


def place(t, name, readonly=True):
    """An operand of a front: `t` itself in a plain run, its guarded copy in a guarded run (read-only unless said)."""
    if _REGIME[0] is None:
        return t
    return guarded(t, _REGIME[0], name=name, readonly=readonly)


def place_model(m, readonly_parameters=False):
    """Every parameter and buffer of `m` through place(): buffers and, unless said, parameters are written by the front."""
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.data = place(p.data, k, readonly_parameters)
        for k, b in m.named_buffers():
            b.data = place(b.data, k, False)
    return m


def _flatten(value, prefix, out):
    if value is None or isinstance(value, (str, bool)):
        return out
    if torch.is_tensor(value):
        out[prefix] = value.detach().clone()
    elif isinstance(value, (int, float)):
        out[prefix] = torch.tensor(value, dtype=torch.float64)
    elif isinstance(value, dict):
        for k, v in value.items():
            _flatten(v, "%s/%s" % (prefix, k), out)
    elif hasattr(value, "_asdict"):
        _flatten(value._asdict(), prefix, out)
    elif hasattr(value, "__dataclass_fields__"):
        _flatten({k: getattr(value, k) for k in value.__dataclass_fields__}, prefix, out)
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            _flatten(v, "%s/%d" % (prefix, i), out)
    else:
        raise TypeError("cannot compare a %s at %s" % (type(value).__name__, prefix))
    return out


def _same_bytes(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def check_contained(fn, nonfinite_by_contract=()):
    """fn() -> nested tensors, run plain, then with every allocation poisoned with NaN and guard-banded, then with 3.0e30.
    fn places its operands with place() / place_model() and builds its state anew in every call (deep copies of what the
    test made once); torch's CPU generator is re-seeded before each run, because the eager step draws its dropout seeds
    there.  Asserted: the plain run is finite (floating results, except under the prefixes `nonfinite_by_contract`: the
    -inf / NaN an API documents); no guard band was written; no read-only operand changed; every returned tensor has the
    bytes of the plain run -- every byte: none of the fronts below returns entries that its API leaves unspecified (lists
    are padded with -1 / -inf by contract)."""
    def run(poison):
        ga.reset()
        _REGIME[0] = poison
        torch.manual_seed(4242)
        try:
            if poison is None:
                value = fn()
            else:
                with guarded_regime(poison):
                    value = fn()
            torch.cuda.synchronize()
            flat = _flatten(value, "", {})
            if poison is not None:
                assert any(r.site.startswith(PACKAGE) for r in ga.REGISTRY), "no allocation of the package was guarded"
                _assert_contained("poison %r" % poison)
        finally:
            _REGIME[0] = None
            ga.reset()
        return flat

    ref = run(None)
    assert ref, "the front returned nothing to compare"
    for k, v in ref.items():
        if v.dtype.is_floating_point and not any(k.startswith(p) for p in nonfinite_by_contract):
            assert bool(torch.isfinite(v.float()).all()), "the plain run is not finite at %s" % k
    for poison in POISONS:
        got = run(poison)
        assert sorted(got) == sorted(ref)
        bad = [k for k, v in ref.items() if not _same_bytes(v, got[k])]
        assert not bad, "poison %r changes %d tensors, e.g. %s" % (poison, len(bad), bad[:6])
    return ref


@pytest.mark.parametrize("poison", POISONS, ids=["nan", "3e30"])
def test_the_checker_sees_a_planted_write_on_the_device(dev, poison):
    """The net itself, on the device: allocations made inside the package under guard_allocations() are registered under
    the allocating line, and one byte written (by plain indexing into the store) before or behind any of them, or behind
    an operand, is reported; nothing is reported before."""
    from unet_nested4tiny_objects_keypoints_amd import create_heatmap
    ga.reset()
    points = torch.tensor([[[3.0, 4.0], [10.0, 2.0], [7.0, 7.0], [1.0, 9.0], [12.0, 12.0], [5.0, 1.0]]], device=dev)
    try:
        pp = guarded(points, poison, name="points", readonly=True)
        with guarded_regime(poison):
            maps = create_heatmap(pp, 13, 15)
            flag = torch.zeros(3, dtype=torch.bool, device=dev)
            wide = torch.full((5,), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert float(maps.max()) > 0.5 and not bool(flag.any()) and bool((wide == -1).all())
        sites = [r.site for r in ga.REGISTRY]
        assert sites[0] == "points" and sum(s.startswith(PACKAGE + "/ops.py:") for s in sites) >= 2, sites   # out, workspace
        assert ga.violations() == [] and ga.changed_operands() == []
        for rec in list(ga.REGISTRY):
            n = rec.n_bytes
            for at, want in ((GUARD_BYTES - 1, (rec.site, "before", -1)), (GUARD_BYTES + n, (rec.site, "behind", n)),
                             (n + 2 * GUARD_BYTES - 1, (rec.site, "behind", n + GUARD_BYTES - 1))):
                old = int(rec.store[at])
                rec.store[at] = old ^ 0x5A
                assert ga.violations() == [want]
                rec.store[at] = old
        assert ga.violations() == []
        pp[0, 0, 0] = 99.0
        assert ga.changed_operands() == ["points"]
    finally:
        ga.reset()


# ---- training-step variants ------------------------------------------------------------------------------------------
FS4 = dict(in_channels=1, n_classes=4, feature_scale=4)


@pytest.fixture(scope="module")
def fs4(dev):
    """The fs=4 network in training mode with a batch, targets that hold negatives and exact ones, and a teacher map with
    holes: made once, deep-copied by every run."""
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(57)
    base = UNet_Nested(**FS4).to(dev).train()
    base.drop_out.p = 0.4
    g = torch.Generator().manual_seed(58)
    x = torch.randn(2, 1, 64, 64, generator=g)
    t = torch.rand(2, 4, 64, 64, generator=g)
    plain_t = t.clone()
    pick = torch.rand(t.shape, generator=g)
    t[pick < 0.10] = -1.0                    # ignored elements
    t[pick > 0.97] = 1.0                     # the positives of the penalty-reduced loss
    plain_t[pick > 0.97] = 1.0
    teacher = torch.rand(t.shape, generator=g)
    teacher[torch.rand(t.shape, generator=g) < 0.05] = -1.0      # "no teacher here"
    return base, x.to(dev), t.to(dev), plain_t.to(dev), teacher.to(dev)


def _train_state(m, opt, outs, loss, extra=None):
    d = {"loss": loss, "outs": list(outs), "extra": extra,
         "param": dict(m.named_parameters()), "buf": dict(m.named_buffers()),
         "grad": {k: p.grad for k, p in m.named_parameters() if p.grad is not None}}
    state = {}
    for k, p in m.named_parameters():
        for key, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v) or isinstance(v, (int, float)):
                state["%s/%s" % (k, key)] = v
    d["state"] = state
    return d


def _optimizers():
    from unet_nested4tiny_objects_keypoints_amd import AdaBound, AdamW, SGDW
    return {
        "adamw": lambda ps: AdamW(ps, lr=1e-3, weight_decay=0.01, capturable=True, max_grad_norm=1.0, skip_nonfinite=True),
        "adabound": lambda ps: AdaBound(ps, lr=1e-3, final_lr=0.1, amsbound=True),
        "sgdw": lambda ps: SGDW(ps, lr=1e-2, momentum=0.9, weight_decay=1e-4, nesterov=True),
        "sgd": lambda ps: torch.optim.SGD(ps, lr=1e-2),
    }


def _criteria():
    import unet_nested4tiny_objects_keypoints_amd as pkg

    def teacher(q):
        crit = pkg.TeacherDistillLoss(weight=0.5, ignore_negative=True)
        crit.set_teacher(q)
        return crit

    return {
        "focal": lambda q: pkg.FocalLoss_BCE_2d(gamma=3, size_average=False),
        "focal-ignore": lambda q: pkg.FocalLoss_BCE_2d(gamma=3, size_average=False, ignore_negative=True),
        "topk": lambda q: pkg.TopKFocalLoss_BCE_2d(k=500, ignore_negative=True),        # 500 of the 4096 pixels of a map
        "topk-plain": lambda q: pkg.TopKFocalLoss_BCE_2d(k=500),
        "prfocal": lambda q: pkg.PenaltyReducedFocalLoss(ignore_negative=True),
        "prfocal-plain": lambda q: pkg.PenaltyReducedFocalLoss(),
        "distill": lambda q: pkg.HeadDistillLoss(weight=0.5, ignore_negative=True),
        "teacher": teacher,
    }


TRAIN_CASES = [
    # (id, optimizer, criterion, bf16, head, frozen BatchNorm: None or its `affine`, WeightAverager)
    ("adamw-clip-skip-averager-f32", "adamw", "focal", False, None, None, True),
    ("adamw-clip-skip-averager-bf16", "adamw", "focal", True, None, None, True),
    ("adabound-amsbound", "adabound", "focal", False, None, None, False),
    ("sgdw-nesterov", "sgdw", "focal", False, None, None, False),
    ("topk-f32", "sgd", "topk", False, None, None, False),
    ("topk-bf16", "sgd", "topk", True, None, None, False),
    ("prfocal", "sgd", "prfocal", False, None, None, False),
    ("head-distill", "sgd", "distill", False, None, None, False),
    ("teacher-f32", "sgd", "teacher", False, None, None, False),
    ("teacher-bf16", "sgd", "teacher", True, None, None, False),
    # the entry points of the same losses without / with the ignore rule
    ("focal-ignore", "sgd", "focal-ignore", False, None, None, False),
    ("topk-no-ignore", "sgd", "topk-plain", False, None, None, False),
    ("prfocal-no-ignore", "sgd", "prfocal-plain", False, None, None, False),
    ("head1", "sgd", "focal", False, 1, None, False),
    ("head2", "sgd", "focal", False, 2, None, False),
    ("frozen-bn-affine", "sgd", "focal", False, None, True, False),
    ("frozen-bn-statistics-only", "sgd", "focal", False, None, False, False),
    ("frozen-bn-affine-bf16", "sgd", "focal", True, None, True, False),
    ("head-train-generated-masks", "sgd", "focal", False, None, None, False),     # p = 0.4, no explicit masks: ops.head_train
]


@pytest.mark.parametrize("name,optimizer,criterion,bf16,head,frozen,averager", TRAIN_CASES, ids=[c[0] for c in TRAIN_CASES])
def test_training_step_variants_write_only_their_own_memory(dev, fs4, name, optimizer, criterion, bf16, head, frozen, averager):
    """Two steps of train_step from the same state: outputs, loss, parameters, buffers, gradients and optimizer state (and
    the averager's shadow, its count, the clip block's norm and skip count) have the bytes of the plain run."""
    from unet_nested4tiny_objects_keypoints_amd import WeightAverager, train_step
    base, x, t, plain_t, teacher = fs4
    make_opt, make_crit = _optimizers()[optimizer], _criteria()[criterion]
    target = plain_t if criterion in ("focal", "topk-plain", "prfocal-plain") else t    # negatives only where ignored
    launched = []

    def fn():
        fused_before = CALLS.get("unetpp_head_train", 0)
        m = copy.deepcopy(base)
        if bf16:
            m.set_activation_dtype(BF)
        if frozen is not None:
            m.freeze_batchnorm(True, affine=frozen)
        place_model(m)
        xx, tt = place(x, "x"), place(target, "target")
        crit = make_crit(place(teacher, "teacher"))
        opt = make_opt([p for p in m.parameters() if p.requires_grad])
        avg = WeightAverager(m) if averager else None
        for _ in range(2):
            outs, loss = train_step(m, opt, crit, xx, tt, head=head)
            if avg is not None:
                avg.update()
        extra = {}
        if avg is not None:
            with avg.applied():           # the swap launch, in and out
                extra["applied"] = [p.detach().clone() for p in m.parameters()]
            extra.update(shadow=avg._flat, ints=avg._ints, n=avg.n_averaged)
        if getattr(opt, "max_grad_norm", None) is not None:
            extra.update(norm=opt.last_grad_norm, skipped=opt.skipped_steps)
        for k in ("last_supervised", "last_distill"):
            extra[k] = getattr(crit, k, None)
        launched.append(CALLS.get("unetpp_head_train", 0) - fused_before)      # (counted in the guarded runs only)
        return _train_state(m, opt, outs, loss, extra)

    ref = check_contained(fn)
    assert len([k for k in ref if k.startswith("/outs/")]) == (head or 3)
    if name == "head-train-generated-masks":
        assert launched[-1] > 0, "the fused head_train pass did not run"


def test_clip_grad_norm_writes_only_the_gradients(dev, fs4):
    """clip_grad_norm_ after a backward pass, with a bound far below the norm so that the scale launch writes."""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, clip_grad_norm_
    from unet_nested4tiny_objects_keypoints_amd.step import forward_loss_backward
    base, x, _, plain_t, _ = fs4

    def fn():
        m = place_model(copy.deepcopy(base), readonly_parameters=True)
        outs, loss = forward_loss_backward(m, FocalLoss_BCE_2d(gamma=3), place(x, "x"), place(plain_t, "target"))
        before = [p.grad.clone() for p in m.parameters()]
        norm = clip_grad_norm_(m.parameters(), 1e-3)
        return {"loss": loss, "outs": list(outs), "norm": norm, "before": before, "grad": [p.grad for p in m.parameters()]}

    ref = check_contained(fn)
    assert float(ref["/norm"]) > 1e-3 and not torch.equal(ref["/before/0"], ref["/grad/0"])


# ---- inference -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fs4_eval(dev):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(61)
    base = UNet_Nested(**FS4).to(dev)
    with torch.no_grad():                       # running statistics that are not the initial 0 / 1
        for k, b in base.named_buffers():
            if k.endswith("running_mean"):
                b.normal_(0.0, 0.1)
            elif k.endswith("running_var"):
                b.uniform_(0.5, 1.5)
    base.drop_out.p = 0.4
    x = torch.randn(2, 1, 32, 48, generator=torch.Generator().manual_seed(62)).to(dev)
    return base.eval(), x


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_inference_modes_write_only_their_own_memory(dev, fs4_eval, bf16):
    """infer at every head, the ensemble mean and infer_mc: the weights and the input are read-only operands."""
    base, x = fs4_eval

    def fn():
        m = copy.deepcopy(base)
        if bf16:
            m.set_activation_dtype(BF)
        place_model(m, readonly_parameters=True)
        xx = place(x, "x")
        with torch.no_grad():
            out = {"head%d" % j: m.infer(xx, head=j) for j in range(1, m.depth)}
            out["ensemble"] = m.infer(xx, ensemble=True)
            out["ensemble2"] = m.infer(xx, head=2, ensemble=True)
            out["mc"] = m.infer_mc(xx, samples=4, seed=7)
            out["mc1"] = m.infer_mc(xx, head=1, samples=4, seed=7)
        return out

    ref = check_contained(fn)
    assert ref["/mc/var"].max() > 0


# ---- scenes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_case(dev):
    """A depth-3 network in eval mode (head 2 needs a halo of 24, so 52 is the smallest tile the class accepts) and two
    uint8 frames of 88 x 84."""
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(71)
    base = UNet_Nested(in_channels=1, n_classes=2, feature_scale=4, depth=3).to(dev)
    with torch.no_grad():
        for k, b in base.named_buffers():
            if k.endswith("running_mean"):
                b.normal_(0.0, 0.1)
            elif k.endswith("running_var"):
                b.uniform_(0.5, 1.5)
    base.drop_out.p = 0.4
    g = torch.Generator().manual_seed(72)
    frames = torch.randint(0, 256, (2, 88, 84, 1), generator=g, dtype=torch.uint8)
    frames[0, 20:40, 10:50] //= 8                  # structure for the cascade's screen: dark and bright patches
    frames[1, 50:80, 40:80] //= 8
    return base.eval(), frames.to(dev)


def _scene_model(base):
    return place_model(copy.deepcopy(base), readonly_parameters=True)


SCENES = {
    # tile 64, halo 24: origins 0, 16, 24 (rows) and 0, 16, 20 (columns) -- the last row and column of tiles are ragged;
    # 18 tiles in chunks of 4; all eight variants, so flips and the transposing ones
    "ragged-dihedral": dict(tile=64, tta="dihedral", chunk=4),
    # the smallest tile: a step of 4 pixels, 10 x 9 tiles a frame, in chunks of 32; flips
    "smallest-tile-flips": dict(tile=52, tta="flips", chunk=32),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_inference_writes_only_its_own_memory(dev, scene_case, name):
    from unet_nested4tiny_objects_keypoints_amd import PeakDetector, SceneInference
    from unet_nested4tiny_objects_keypoints_amd.scene import plan_tiles
    base, frames = scene_case
    kw = SCENES[name]
    rows, cols = plan_tiles(88, 84, kw["tile"], 24, 4)
    assert len(rows) >= 2 and len(cols) >= 2 and 2 * len(rows) * len(cols) > kw["chunk"]
    if name == "ragged-dihedral":
        assert rows[-1][0] - rows[-2][0] != rows[1][0] and cols[-1][0] - cols[-2][0] != cols[1][0]

    def fn():
        m = _scene_model(base)
        ff = place(frames, "frames")
        scene = SceneInference(m, **kw)
        out = {"maps": scene(ff)}
        out["detections"] = scene.detect(ff, PeakDetector(radius=2))
        if name == "ragged-dihedral":      # uncertainty() has no form under test-time augmentation: the same plan without
            out["uncertainty"] = SceneInference(m, tile=kw["tile"], chunk=kw["chunk"]).uncertainty(ff, samples=4)
        return out

    ref = check_contained(fn, nonfinite_by_contract=("/detections/score",))     # -inf pads a list
    assert int(ref["/detections/count"].min()) >= 0


def test_cascade_scene_inference_writes_only_its_own_memory(dev, scene_case):
    from unet_nested4tiny_objects_keypoints_amd import CascadeSceneInference
    base, frames = scene_case
    kw = dict(tile=64, tta="flips", chunk=4)
    probe = CascadeSceneInference(copy.deepcopy(base), threshold=0.0, **kw)
    probe(frames)
    threshold = float(probe.last_scores.float().median())

    def fn():
        m = _scene_model(base)
        cascade = CascadeSceneInference(m, threshold=threshold, **kw)
        out = cascade(place(frames, "frames"))
        return {"maps": out, "active": cascade.last_active, "scores": cascade.last_scores}

    ref = check_contained(fn)
    active = ref["/active"]
    assert bool(active.any()) and not bool(active.all()), "the threshold must leave some tiles active and some not"


# ---- detection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_points", [64, 8], ids=["all-peaks", "truncated"])
def test_peak_detector_and_evaluate_write_only_their_own_memory(dev, max_points):
    """The constructed maps of tests/test_gpu_detect.py, 70 x 90 (neither a multiple of 4): every map holds at least 12
    peaks, so max_points = 8 truncates every list."""
    from tests.test_gpu_detect import THR, seeded_maps
    from unet_nested4tiny_objects_keypoints_amd import PeakDetector, evaluate
    maps = torch.from_numpy(seeded_maps(4, 70, 90, 2, seed=270)).view(2, 2, 70, 90).to(dev)
    labels = torch.tensor([[[0.0, 0.0], [88.5, 0.0], [62.0, 16.0], [30.0, 12.0], [-1.0, -1.0], [50.0, 50.0]]] * 2).to(dev)
    classes = torch.tensor([0, 1, 0, 1, 0, 1], dtype=torch.int32).to(dev)

    def fn():
        dets = PeakDetector(threshold=THR, radius=2, max_points=max_points)(place(maps, "maps"))
        score = evaluate(dets, place(labels, "labels"), place(classes, "classes"), tolerance=2.0)
        return {"detections": dets, "score": score}

    ref = check_contained(fn, nonfinite_by_contract=("/detections/score", "/score/mean_distance"))
    count = ref["/detections/count"]
    assert int(count.min()) >= 12
    assert bool((count > max_points).all()) == (max_points == 8)
    assert int(ref["/score/tp_total"]) > 0


# ---- key points ------------------------------------------------------------------------------------------------------
def test_transfer_points_on_the_hole_cases_writes_only_its_own_memory(dev):
    """Heatmap.transfer_points on the constructed hole cases, built as test_holes_end_to_end_through_the_heatmap_front
    builds them (tests/test_gpu_keypoints.py)."""
    import numpy as np

    from tests import keypoints_corpus as corpus
    from unet_nested4tiny_objects_keypoints_amd import Heatmap
    maps = np.zeros((3, 2, 64, 72), dtype=np.float32)
    for k, (_, heat, _) in enumerate(corpus.hole_cases()):
        maps[k // 2, k % 2, :heat.shape[0], :heat.shape[1]] = heat
    maps = torch.from_numpy(maps).to(dev)

    def fn():
        points, found = Heatmap([[0], [1, 2]], 72, 64).transfer_points(place(maps, "maps"), threshold=corpus.THRESHOLD)
        return {"points": points, "found": found}

    ref = check_contained(fn)
    assert ref["/points"][0, 0, 0].tolist() == [11.0, 11.0]          # the plus-shaped hole's bright centre


@pytest.mark.parametrize("segmentation", ["watershed", "components"])
def test_keypoints_extract_in_both_carve_ups_of_its_workspace(dev, segmentation):
    """ops.keypoints_extract carves one byte workspace sized by unetpp_keypoints_workspace_bytes(maps, h, w, max_regions)
    into five arrays; max_regions = the region count takes the ranked selection, one below it the exact rounds."""
    from tests import keypoints_corpus as corpus
    from unet_nested4tiny_objects_keypoints_amd import ops
    cases = {name: (heat, thr) for name, heat, thr in corpus.tie_cases()}
    heat, thr = cases["speckle 33x47"]
    count = dict(zip(("components", "watershed"), corpus.TIE_COUNTS["speckle 33x47"]))[segmentation]
    heat = torch.from_numpy(heat[None]).to(dev)

    def fn():
        hh = place(heat, "heat")
        out = {}
        for limit in (count, count - 1):
            points, counts = ops.keypoints_extract(hh, 4, thr, max_regions=limit, segmentation=segmentation)
            out["limit%d" % limit] = {"points": points, "counts": counts}
        labels, dist = ops.keypoints_regions(hh, thr, segmentation)
        out["regions"] = {"labels": labels, "distance": dist}
        return out

    ref = check_contained(fn)
    assert int(ref["/limit%d/counts" % count][0]) == count
    assert torch.equal(ref["/limit%d/points" % count], ref["/limit%d/points" % (count - 1)])


def test_validate_step_writes_only_its_own_memory(dev, fs4_eval):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, Heatmap, validate_step
    base, _ = fs4_eval
    g = torch.Generator().manual_seed(91)
    x = torch.randn(2, 1, 32, 48, generator=g).to(dev)
    labels = (torch.rand(2, 5, 2, generator=g) * torch.tensor([47.0, 31.0])).to(dev)

    def fn():
        m = place_model(copy.deepcopy(base), readonly_parameters=True)
        hm = Heatmap([[0], [1], [2], [3, 4]], 48, 32)
        return validate_step(m, FocalLoss_BCE_2d(gamma=3), hm, place(x, "x"), place(labels, "labels"))

    check_contained(fn, nonfinite_by_contract=("/landmark_losses",))     # NaN where nothing matched


# ---- data ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["uint8", "float32"])
def test_device_loader_writes_only_its_own_memory(dev, store):
    """out_size (16, 13): rows of 13 floats, so every row but the first starts off a 16-byte boundary and ends in a tail."""
    from unet_nested4tiny_objects_keypoints_amd import Augment, DeviceLoader
    g = torch.Generator().manual_seed(101)
    if store == "uint8":
        images = torch.randint(0, 256, (5, 20, 22, 3), generator=g, dtype=torch.uint8).to(dev)
    else:
        images = torch.rand(5, 3, 20, 22, generator=g).to(dev)
    labels = (torch.rand(5, 4, 2, generator=g) * torch.tensor([21.0, 19.0]))
    labels[1, 2] = -1.0
    labels = labels.to(dev)
    index = torch.tensor([4, 0, 2, 2, 1], dtype=torch.int64).to(dev)

    def fn():
        aug = Augment(rotate=25.0, scale=(0.8, 1.25), translate=(2, 2), contrast=(0.8, 1.2), brightness=0.1)
        loader = DeviceLoader(place(images, "images"), place(labels, "labels"), (16, 13), augment=aug, seed=3)
        plain = DeviceLoader(place(images, "images2"), None, (16, 13), seed=3)
        return {"augmented": [loader.batch(place(index, "index")) for _ in range(2)], "identity": plain.batch([0, 3, 4])[0]}

    check_contained(fn)


def test_scene_crops_with_paste_and_ignore_write_only_their_own_memory(dev):
    """SceneCrops with an ObjectPaste and the union of rectangles and two masks (one packed from a raster, one from
    polygon rings), crop (24, 30): a width that is no multiple of 4."""
    import numpy as np

    from tests.test_gpu_mask import _scene
    from unet_nested4tiny_objects_keypoints_amd import (Augment, IgnoreMask, IgnoreRegions, IgnoreUnion, ObjectPaste,
                                                        SceneCrops)
    frames, labels, classes, raster, rects, rcls = _scene()
    frames, labels, classes, raster = (torch.from_numpy(np.array(a, order="C")).to(dev) for a in (frames, labels, classes, raster))
    rects, rcls = torch.from_numpy(rects).to(dev), torch.from_numpy(rcls).to(dev)
    ring = torch.tensor([[[[70.0, 5.0], [90.0, 8.0], [85.0, 30.0], [72.0, 24.0]]]] * 2).to(dev)       # [S, 1 ring, 4, 2]
    ring_counts = torch.tensor([[4], [4]], dtype=torch.int32).to(dev)

    def fn():
        mask = IgnoreMask.from_raster(place(raster, "raster"), [-1, 0])
        polygons = IgnoreMask.from_polygons(place(ring, "ring"), place(ring_counts, "ring counts"), (80, 96), plane_class=[1])
        ignore = IgnoreUnion(IgnoreRegions(place(rects, "rects"), place(rcls, "rect classes")), mask, polygons)
        crops = SceneCrops(place(frames, "frames"), place(labels, "labels"), place(classes, "classes"), n_classes=2,
                           crop=(24, 30), p_object=0.6, jitter=(8, 8), radius=3.0, seed=6, ignore=ignore,
                           ignore_outside=True, augment=Augment(rot90=False, rotate=20.0, scale=(0.8, 1.25)),
                           paste=ObjectPaste(max_pastes=3, p=0.8, patch_radius=2, core=1.5))
        out = {"bits": mask.bits, "polygon bits": polygons.bits, "batches": []}
        for _ in range(2):
            batch = crops.batch(5)
            out["batches"].append({"batch": batch, "paste": crops.last_paste, "last": crops.last})
        return out

    ref = check_contained(fn)
    target = ref["/batches/0/batch/1"]
    assert bool((target < 0).any()) and bool((target > 0).any())
    assert bool((ref["/batches/0/paste/src"] >= 0).any()) or bool((ref["/batches/1/paste/src"] >= 0).any())
    assert bool(ref["/polygon bits"].ne(0).any())


def test_create_heatmap_writes_only_its_own_memory(dev):
    from unet_nested4tiny_objects_keypoints_amd import Heatmap, create_heatmap
    g = torch.Generator().manual_seed(111)
    points = (torch.rand(3, 6, 2, generator=g) * torch.tensor([44.0, 37.0])).to(dev)

    def fn():
        pp = place(points, "points")
        return {"reference": create_heatmap(pp, 38, 45), "pattern": Heatmap([[0, 3], [1, 4], [2, 5]], 45, 38).create_heatmap(pp)}

    ref = check_contained(fn)
    assert float(ref["/pattern"].max()) > 0.5


# ---- entry points that no front above reaches: the autograd form of the ensemble, direct ops calls ---------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_pruned_ensemble_step_writes_only_its_own_memory(dev, fs4, bf16):
    """forward_pruned(ensemble=True) and its backward (the heads-mean kernels), one map through the criterion."""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    base, x, _, plain_t, _ = fs4

    def fn():
        m = copy.deepcopy(base)
        m.drop_out.p = 0.0                    # the mean of the heads has no dropout
        if bf16:
            m.set_activation_dtype(BF)
        place_model(m, readonly_parameters=True)
        out = m.forward_pruned(place(x, "x"), 2, ensemble=True)
        loss = FocalLoss_BCE_2d(gamma=3)(out, place(plain_t, "target"))
        loss.backward()
        return {"out": out, "loss": loss, "grad": {k: p.grad for k, p in m.named_parameters() if p.grad is not None}}

    ref = check_contained(fn)
    assert len([k for k in ref if k.startswith("/grad/")]) > 4


@pytest.mark.parametrize("cin", [1, 3], ids=["grey", "rgb"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_input_gradient_writes_only_its_own_memory(dev, bf16, cin):
    """A network input that requires a gradient: the first layer's input gradient (with bf16 storage its own kernel) and,
    with three channels, the layout changes NCHW -> NHWC -> NCHW (one channel is the same bytes either way)."""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet_Nested
    from unet_nested4tiny_objects_keypoints_amd.step import forward_loss_backward
    torch.manual_seed(131)
    base = UNet_Nested(in_channels=cin, n_classes=4, feature_scale=4).to(dev).train()
    g = torch.Generator().manual_seed(132)
    x = torch.randn(2, cin, 64, 64, generator=g).to(dev)
    t = torch.rand(2, 4, 64, 64, generator=g).to(dev)

    def fn():
        m = copy.deepcopy(base)
        if bf16:
            m.set_activation_dtype(BF)
        place_model(m, readonly_parameters=True)
        xx = place(x, "x").detach().requires_grad_(True)       # (detach: a leaf of this run, `x` itself stays as it is)
        outs, loss = forward_loss_backward(m, FocalLoss_BCE_2d(gamma=3), xx, place(t, "target"))
        return {"loss": loss, "outs": list(outs), "dx": xx.grad}

    ref = check_contained(fn)
    assert not x.requires_grad and ref["/dx"].shape == x.shape and float(ref["/dx"].abs().max()) > 0


def test_separate_convolution_and_batchnorm_finalize_write_only_their_own_memory(dev):
    """The two-call form that the engine no longer takes: ops.gemm_fwd without a pack plan (the call packs its own weight
    image) into per-block statistics rows, then ops.bn_finalize over them.  40 x 24 pixels, 16 -> 24 channels: ragged
    patches and a partial column tile."""
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    from unet_nested4tiny_objects_keypoints_amd.ops import V
    b, h, w, ci, co = 3, 40, 24, 16, 24
    g = torch.Generator().manual_seed(121)
    src = torch.randn(b, h, w, ci, generator=g).to(dev)
    weight = engine.pack_conv_fwd((torch.randn(co, ci, 3, 3, generator=g) * 0.2).to(dev)).packed()    # [taps][K][N]
    bias, gamma, beta = (torch.randn(co, generator=g).to(dev) for _ in range(3))

    def fn():
        y = torch.empty(b, h, w, co, device=dev)
        blocks = ops.gemm_pixel_blocks(b, h, w)
        part = torch.empty(blocks * co * 2, device=dev)
        ops.gemm_fwd(b, h, w, 9, [V(place(src, "x"))], [V(y)], place(weight, "weight"), place(bias, "bias"), part)
        rm = place(torch.zeros(co, device=dev), "running_mean", readonly=False)
        rv = place(torch.ones(co, device=dev), "running_var", readonly=False)
        stats = ops.bn_finalize(part, blocks, co, b * h * w, place(gamma, "gamma"), place(beta, "beta"), 1e-5, 0.1, rm, rv)
        return {"y": y, "stats": list(stats), "running": [rm, rv]}

    check_contained(fn)


# ---- coverage: runs last in this module --------------------------------------------------------------------------------
QUERY = "a size query: launches nothing"
PLAN = "a host-side plan: launches nothing"
SWITCH = "a host-side switch or report: launches nothing"
EXEMPT = {
    "unetpp_abi_version": SWITCH, "unetpp_build_arch": SWITCH, "unetpp_last_kernel_name": SWITCH,
    "unetpp_set_reserved_cus": SWITCH, "unetpp_debug_set": SWITCH, "unetpp_debug_get": SWITCH, "unetpp_usable_cus": SWITCH,
    "unetpp_gemm_pixel_blocks": QUERY, "unetpp_gemm_stats_rows": QUERY, "unetpp_gemm_weight_image_floats": QUERY,
    "unetpp_bn_bwd_blocks": QUERY, "unetpp_bn_bwd_blocks_bf16": QUERY, "unetpp_bn_frozen_bwd_blocks": QUERY,
    "unetpp_bn_frozen_bwd_blocks_bf16": QUERY, "unetpp_head_bwd_blocks": QUERY, "unetpp_focal_bce_blocks": QUERY,
    "unetpp_heatmap_workspace_bytes": QUERY, "unetpp_heatmap_pattern_workspace_bytes": QUERY,
    "unetpp_keypoints_workspace_bytes": QUERY, "unetpp_peaks_workspace_bytes": QUERY,
    "unetpp_topk_focal_workspace_bytes": QUERY, "unetpp_pr_focal_workspace_bytes": QUERY, "unetpp_optim_chunk_elems": QUERY,
    "unetpp_bn_bwd_pool_ok": QUERY,
    "unetpp_gemm_plan": PLAN, "unetpp_wgrad_plan": PLAN, "unetpp_bn_bwd_plan": PLAN,
}


def test_every_launching_entry_point_ran_under_guards(dev):
    """Runs last in this module: every entry point of _lib.SIGNATURES was called while a guarded run was active -- its
    operands between bands, the bands read back afterwards -- or stands in EXEMPT, which holds only entry points that
    launch nothing."""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    unknown = sorted(set(EXEMPT) - set(_lib.SIGNATURES))
    assert not unknown, unknown
    missing = sorted(k for k in _lib.SIGNATURES if k not in EXEMPT and not CALLS.get(k))
    assert not missing, "no guarded run reached: %s" % missing
