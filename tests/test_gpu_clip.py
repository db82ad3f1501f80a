"""Gradient clipping and the non-finite skip of the fused optimizers, and the stand-alone clip_grad_norm_ (optim.py,
csrc/optim.hip: unetpp_grad_norm, unetpp_optim_step_clip, unetpp_grad_scale) on the GPU.

One small synthetic parameter set hits every kernel path: a 1-element tensor, a 7-element one (tail only), 4096*2 + 5
elements (crosses chunks, leaves a remainder), a tensor whose gradient is a view offset by one float (an unaligned
segment, vec = 0), a parameter without a gradient, a zero-element parameter, and 300 007 elements so that a grid sized
for 8 CUs (64 workgroups) walks several of the 81 chunks; two parameter groups.  Gradients are seeded randn scaled per
tensor by 1e-3 ... 1e3.

The oracle of the clipped step is the EXISTING unclipped kernel (pinned by the reference's fixtures in
tests/test_gpu_optim.py) on gradients that torch scaled beforehand; the oracle of the norm is numpy float64.  That
compares kernel with kernel (the unaligned segment included); the clipped step also has an oracle that shares no code
with the kernel: tests/test_gpu_optim_elementwise.py takes the norm a clipped step published, recomputes the coefficient
and the update in numpy float32 (tests/optim_oracle.py) and holds every element of every step to it, bit for bit."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (7,), (4096 * 2 + 5,), (4096 + 3,), (10,), (0,), (300007,)]
SCALES = [1e3, 1e-3, 1.0, 10.0, None, 1.0, 1e-1]        # None: this parameter never has a gradient
OFFSET = 3                                              # its gradient is a view one float into a larger buffer
STEPS = 4
M_ACTIVE, M_IDLE = 8.0, 1.0e6                           # the norms are ~650 ... 2000 (asserted below)


def _host_inputs():
    g = torch.Generator().manual_seed(1234)
    params = [torch.randn(s, generator=g).numpy() for s in SHAPES]
    grads = []
    for step in range(STEPS):
        grads.append([None if sc is None else (torch.randn(s, generator=g) * sc).numpy() for s, sc in zip(SHAPES, SCALES)])
    return params, grads


PARAMS0, GRADS = _host_inputs()
# float64 references, computed once: the norm of every step's gradients
NORM64 = [float(np.sqrt(sum(np.sum(g.astype(np.float64) ** 2) for g in gs if g is not None))) for gs in GRADS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


def _params(dev):
    return [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in PARAMS0]


def _groups(params, lr):
    return [{"params": params[0::2], "lr": lr}, {"params": params[1::2], "lr": 0.5 * lr}]


def _set_grads(params, step, dev, coef=None, edit=None):
    """p.grad = GRADS[step] (times coef, one fp32 multiply by torch, when given); the OFFSET gradient is unaligned."""
    for i, (p, g) in enumerate(zip(params, GRADS[step])):
        if g is None:
            p.grad = None
            continue
        t = torch.from_numpy(g.copy()).to(dev)
        if edit is not None and i in edit:
            t.view(-1)[edit[i][0]] = edit[i][1]
        if coef is not None:
            t = t * coef
        if i == OFFSET:
            buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
            view = buf[1:].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            t = view
        p.grad = t


def _coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient in fp32 from a 0-dim fp32 norm (on the CPU: IEEE arithmetic)."""
    c = max_norm / (norm.detach().cpu().float() + 1e-6)
    assert c.dtype == torch.float32
    return torch.clamp(c, max=1.0)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32)))


def _check_norm(got, step, what):
    """One fp32 ulp of the float64 reference.  Why: every product double(g)^2 is exact (24-bit x 24-bit fits 53 bits),
    a sum of n <= 2^19 non-negative doubles in any order is off by at most n * 2^-53 < 6e-11 relative, double sqrt adds
    2^-53; the only rounding that matters is the final conversion to float, half an ulp.  One ulp leaves room for the
    reference's own double rounding at a tie and nothing else."""
    got = float(got)
    ref = NORM64[step]
    assert 100.0 < ref < 1.0e4                       # M_ACTIVE clips, M_IDLE does not
    err = abs(got - ref)
    print("%s step %d: norm %.9g reference %.17g err %.3g ulp" % (what, step, got, ref, err / _ulp32(ref)))
    assert err <= _ulp32(ref), (what, step, got, ref)


def _opt_norm(dev, step=0, **kw):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    params = _params(dev)
    opt = pkg.AdamW(_groups(params, 1e-3), max_grad_norm=M_ACTIVE, **kw)
    _set_grads(params, step, dev)
    opt.step()
    return opt.last_grad_norm.clone(), params


# ---- 1. the norm -----------------------------------------------------------------------------------------------------
def test_norm_against_float64(dev):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    from tests.helpers import usable_cus
    a, pa = _opt_norm(dev)
    b, pb = _opt_norm(dev)
    with usable_cus(8) as u:
        c, pc = _opt_norm(dev)
        assert 81 > 8 * u.cus                         # 81 chunks on 64 workgroups: some walk two chunks
    d, _ = _opt_norm(dev, capturable=True)
    params = _params(dev)
    _set_grads(params, 0, dev)
    e = pkg.clip_grad_norm_(params, M_IDLE)
    with usable_cus(8):
        f = pkg.clip_grad_norm_(params, M_IDLE)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and a.dim() == 0 and a.is_cuda
    assert e.dtype == torch.float32 and e.dim() == 0 and e.is_cuda
    _check_norm(a, 0, "last_grad_norm")
    _check_norm(e, 0, "clip_grad_norm_")
    for other in (b, c, d, e, f):                     # run to run, any grid, either mode, either caller: the same bits
        assert torch.equal(a, other), (float(a), float(other))
    for x, y, z in zip(pa, pb, pc):
        assert torch.equal(x, y) and torch.equal(x, z)


# ---- 2. clip_grad_norm_ ----------------------------------------------------------------------------------------------
def test_clip_grad_norm_scales_in_place(dev):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    params = _params(dev)
    _set_grads(params, 1, dev)
    g0 = [None if p.grad is None else p.grad.clone() for p in params]
    ptrs = [None if p.grad is None else p.grad.data_ptr() for p in params]
    norm = pkg.clip_grad_norm_(params, M_ACTIVE)
    torch.cuda.synchronize()
    _check_norm(norm, 1, "clip_grad_norm_")
    coef = _coef(norm, M_ACTIVE)
    assert float(coef) < 1.0
    for p, g in zip(params, g0):
        assert (p.grad is None) == (g is None)
        if g is not None:
            assert torch.equal(p.grad, g * coef.to(dev))                  # bit for bit: one fp32 multiply
    assert ptrs == [None if p.grad is None else p.grad.data_ptr() for p in params]
    # torch's own function on float64 copies: 2 ulp of fp32
    ref = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in PARAMS0]
    for q, g in zip(ref, GRADS[1]):
        q.grad = None if g is None else torch.from_numpy(g.astype(np.float64))
    ref_norm = torch.nn.utils.clip_grad_norm_(ref, M_ACTIVE)
    assert abs(float(ref_norm) - NORM64[1]) <= 1e-12 * NORM64[1]
    worst = 0.0
    for p, q in zip(params, ref):
        if q.grad is None or q.grad.numel() == 0:
            continue
        want = q.grad.numpy()
        err = np.abs(p.grad.cpu().numpy().astype(np.float64) - want) / _ulp32(want)
        worst = max(worst, float(err.max()))
    print("clipped gradients against torch float64: worst %.3f ulp" % worst)
    assert worst <= 2.0
    # the norm of what is left is max_norm
    again = pkg.clip_grad_norm_(params, M_ACTIVE)
    assert abs(float(again) - M_ACTIVE) <= 1e-5 * M_ACTIVE


def test_clip_grad_norm_leaves_small_gradients_alone(dev):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    params = _params(dev)
    _set_grads(params, 2, dev)
    g0 = [None if p.grad is None else p.grad.clone() for p in params]
    norm = pkg.clip_grad_norm_(params, M_IDLE)
    torch.cuda.synchronize()
    _check_norm(norm, 2, "clip_grad_norm_")
    assert float(_coef(norm, M_IDLE)) == 1.0
    for p, g in zip(params, g0):
        if g is not None:
            assert torch.equal(p.grad, g)
    bf = torch.nn.Parameter(torch.zeros(8, device=dev, dtype=torch.bfloat16))
    bf.grad = torch.ones_like(bf)
    with pytest.raises(TypeError):
        pkg.clip_grad_norm_([bf], 1.0)
    with pytest.raises(RuntimeError, match="non-finite"):
        _set_grads(params, 2, dev, edit={2: (17, float("inf"))})
        pkg.clip_grad_norm_(params, 1.0, error_if_nonfinite=True)
    assert torch.isinf(params[2].grad.view(-1)[17]) and float(params[2].grad.view(-1)[16]) == float(GRADS[2][2][16])


# ---- 3. clipped step == unclipped step on gradients scaled beforehand ------------------------------------------------
CONFIGS = {
    "adamw": ("AdamW", dict(lr=1e-2, weight_decay=1e-2)),
    "adamw_amsgrad": ("AdamW", dict(lr=1e-2, weight_decay=1e-2, amsgrad=True)),
    "adabound": ("AdaBound", dict(lr=1e-2, final_lr=0.1, weight_decay=1e-3)),
    "sgdw": ("SGDW", dict(lr=0.1, momentum=0.9, weight_decay=1e-2)),
}


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_clipped_step_equals_step_on_scaled_gradients(name, capturable, dev):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    cls_name, kw = CONFIGS[name]
    kw = dict(kw)
    lr = kw.pop("lr")
    pa, pb = _params(dev), _params(dev)
    A = getattr(pkg, cls_name)(_groups(pa, lr), **kw, lr=lr, capturable=capturable, max_grad_norm=M_ACTIVE)
    B = getattr(pkg, cls_name)(_groups(pb, lr), **kw, lr=lr, capturable=capturable)
    for step in range(3):
        _set_grads(pa, step, dev)
        kept = [None if p.grad is None else p.grad.clone() for p in pa]
        A.step()
        norm = A.last_grad_norm.clone()
        _check_norm(norm, step, name)
        assert float(norm) > M_ACTIVE                                     # clipping is active
        for p, g in zip(pa, kept):                                        # p.grad is read, never written
            assert (p.grad is None) == (g is None)
            if g is not None:
                assert torch.equal(p.grad, g)
        _set_grads(pb, step, dev, coef=_coef(norm, M_ACTIVE).to(dev))
        B.step()
        torch.cuda.synchronize()
        for i, (p, q) in enumerate(zip(pa, pb)):
            assert torch.equal(p, q), (name, step, i)
            sa, sb = A.state.get(p, {}), B.state.get(q, {})
            assert sa.keys() == sb.keys(), (name, step, i)
            for k in sa:
                if k == "step":
                    assert float(sa[k]) == float(sb[k]), (name, step, i)
                    assert torch.is_tensor(sa[k]) == torch.is_tensor(sb[k]) == capturable
                else:
                    assert torch.equal(sa[k], sb[k]), (name, step, i, k)
    assert any(not torch.equal(p.detach().cpu(), torch.from_numpy(p0)) for p, p0 in zip(pa, PARAMS0))
    assert int(A.skipped_steps) == 0


def test_max_grad_norm_attribute_takes_effect(dev):
    """opt.max_grad_norm = x holds from the next eager step; without a max_norm the coefficient is 1."""
    import unet_nested4tiny_objects_keypoints_amd as pkg
    pa, pb = _params(dev), _params(dev)
    A = pkg.AdamW(_groups(pa, 1e-2), max_grad_norm=M_IDLE)
    B = pkg.AdamW(_groups(pb, 1e-2))
    _set_grads(pa, 0, dev)
    _set_grads(pb, 0, dev)
    A.step()
    B.step()
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))                 # coef = 1: g * 1 = g
    A.max_grad_norm = M_ACTIVE
    _set_grads(pa, 1, dev)
    A.step()
    _set_grads(pb, 1, dev, coef=_coef(A.last_grad_norm, M_ACTIVE).to(dev))
    B.step()
    assert all(torch.equal(p, q) for p, q in zip(pa, pb))


# ---- 4. the non-finite skip ------------------------------------------------------------------------------------------
def _snapshot(params, opt):
    out = [p.detach().clone() for p in params]
    for p in params:
        out += [v.clone() for _, v in sorted(opt.state.get(p, {}).items())]
    return out


def test_nonfinite_steps_are_skipped(dev):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    kw = dict(weight_decay=1e-2, capturable=True, max_grad_norm=M_ACTIVE)
    pa, pb, pc = _params(dev), _params(dev), _params(dev)
    A = pkg.AdamW(_groups(pa, 1e-2), **kw, skip_nonfinite=True)
    B = pkg.AdamW(_groups(pb, 1e-2), **kw, skip_nonfinite=True)          # only ever sees steps 1 and 4
    Cn = pkg.AdamW(_groups(pc, 1e-2), **kw)                               # no skip flag
    bad = [None, {6: (123456, float("inf"))}, {3: (5, float("nan"))}, None]
    _set_grads(pa, 0, dev)
    A.step()
    after1 = _snapshot(pa, A)
    assert all("step" in A.state[p] and float(A.state[p]["step"]) == 1.0 for p in pa if p.grad is not None and p.numel())
    for step in (1, 2):
        _set_grads(pa, step, dev, edit=bad[step])
        A.step()
        now = _snapshot(pa, A)
        assert len(now) == len(after1)
        assert all(torch.equal(x, y) for x, y in zip(now, after1)), step
        assert not bool(torch.isfinite(A.last_grad_norm))
    assert int(A.skipped_steps) == 2
    _set_grads(pa, 3, dev)
    A.step()
    for step in (0, 3):
        _set_grads(pb, step, dev)
        B.step()
    torch.cuda.synchronize()
    assert int(A.skipped_steps) == 2 and int(B.skipped_steps) == 0
    assert all(torch.equal(x, y) for x, y in zip(_snapshot(pa, A), _snapshot(pb, B)))
    assert all(bool(torch.isfinite(p).all()) for p in pa)
    assert not all(torch.equal(x, y) for x, y in zip(_snapshot(pa, A), after1))      # step 4 did update
    # without the flag the same inf step poisons the parameters
    _set_grads(pc, 0, dev)
    Cn.step()
    _set_grads(pc, 1, dev, edit=bad[1])
    Cn.step()
    assert not all(bool(torch.isfinite(p).all()) for p in pc)
    # the skip alone, without a max_norm: the norm pass runs for the decision only
    pd, pe = _params(dev), _params(dev)
    D = pkg.AdamW(_groups(pd, 1e-2), weight_decay=1e-2, capturable=True, skip_nonfinite=True)
    E = pkg.AdamW(_groups(pe, 1e-2), weight_decay=1e-2, capturable=True)
    _set_grads(pd, 0, dev)
    D.step()
    _set_grads(pd, 2, dev, edit=bad[2])
    D.step()
    _set_grads(pe, 0, dev)
    E.step()
    torch.cuda.synchronize()
    assert int(D.skipped_steps) == 1
    assert all(torch.equal(x, y) for x, y in zip(_snapshot(pd, D), _snapshot(pe, E)))


# ---- 5. launches -----------------------------------------------------------------------------------------------------
def test_clipped_step_is_two_kernels(dev):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    from torch.profiler import ProfilerActivity, profile
    params = _params(dev)
    opt = pkg.AdamW(_groups(params, 1e-3), max_grad_norm=M_ACTIVE)
    _set_grads(params, 0, dev)
    opt.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            opt.step()
        torch.cuda.synchronize()
    events = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [n for n in events if not n.lower().startswith(("memcpy", "memset"))]   # eager mode's one small copy
    assert len([n for n in kernels if "grad_norm_kernel" in n]) == 3, events
    assert len([n for n in kernels if "optim_clip_kernel" in n]) == 3, events
    assert len(kernels) <= 3 * 2, events
    assert len(events) <= 3 * 3, events


# ---- 6. the captured step --------------------------------------------------------------------------------------------
def test_graphed_clipped_step_matches_eager(dev):
    from unet_nested4tiny_objects_keypoints_amd import AdamW, FocalLoss_BCE_2d, GraphedTrainStep, UNet_Nested, train_step
    torch.manual_seed(5)
    m = UNet_Nested(in_channels=1, n_classes=4, feature_scale=4).to(dev).train()
    m.drop_out.p = 0.0
    ref = copy.deepcopy(m)
    x = torch.randn(2, 1, 32, 32, device=dev)
    t = torch.rand(2, 4, 32, 32, device=dev)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    max_norm = 1.0
    kw = dict(lr=1e-2, weight_decay=1e-4, capturable=True, max_grad_norm=max_norm, skip_nonfinite=True)
    opt_g, opt_e = AdamW(m.parameters(), **kw), AdamW(ref.parameters(), **kw)
    g = GraphedTrainStep(m, opt_g, crit, x, t, capture_optimizer=True, check_topology=True)
    assert g.topology["chain"] is True, g.topology
    assert int(opt_g.skipped_steps) == 0 and float(opt_g.last_grad_norm) == 0.0      # the warm-up is undone
    for step in range(3):
        outs_g, loss_g = g(x, t)
        outs_e, loss_e = train_step(ref, opt_e, crit, x, t)
        torch.cuda.synchronize()
        assert torch.equal(loss_g, loss_e), step
        for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
            assert torch.equal(p, q), (step, k)
        assert torch.equal(opt_g.last_grad_norm, opt_e.last_grad_norm), step
        print("captured step %d: gradient norm %.6g" % (step, float(opt_g.last_grad_norm)))
        assert float(opt_g.last_grad_norm) > max_norm                     # clipping is active
    for p, q in zip(m.parameters(), ref.parameters()):
        sg, se = opt_g.state[p], opt_e.state[q]
        assert float(sg["step"]) == float(se["step"]) == 3.0
        assert torch.equal(sg["exp_avg"], se["exp_avg"]) and torch.equal(sg["exp_avg_sq"], se["exp_avg_sq"])
    assert int(opt_g.skipped_steps) == 0 and int(opt_e.skipped_steps) == 0
