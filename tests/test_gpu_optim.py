"""The fused AdamW / AdaBound / SGDW (optim.py, csrc/optim.hip) on the GPU: element-wise against the reference's own
optimizers (tests/golden/optim_*.npz, CPU runs of tools/optimizers/*), in eager and capturable mode; determinism;
checkpoints in the reference's format; the weight-image pack plan; launches per step; graph capture.

The fixture comparison samples ~70 elements per tensor with 4 ulp + 1e-5*lr*t on parameters and 1e-6 relative on state.
The only reason it cannot be exact is aten's CPU sqrt: in the torch build that made the fixtures it is not correctly
rounded (every other op of the sequence is: a numpy restatement with that sqrt injected reproduces every recorded value
bit for bit, tests/test_optim_oracle_host.py), while the kernel's is.  The exact check -- every element of every step
against the IEEE restatement of the kernel's contract, at non-default hyper-parameters per group, misaligned segments,
tails and large step counts -- is tests/test_gpu_optim_elementwise.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_optim_golden", os.path.join(GOLDEN, "make_optim_golden.py"))
gm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gm)
SHAPES = gm.shapes()
PARAMS0, GRADS = gm.make_inputs(SHAPES)
WORST_ULP = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


def _make(name, dev, capturable=False):
    import unet_nested4tiny_objects_keypoints_amd as pkg
    cls_name, kw = gm.CONFIGS[name]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in PARAMS0]
    lr = kw["lr"]
    ga, gb = gm.groups_of(params)
    lrs = gm.group_lrs(lr)
    opt = getattr(pkg, cls_name)([{"params": ga, "lr": lrs[0]}, {"params": gb, "lr": lrs[1]}],
                                 **{k: v for k, v in kw.items() if k != "lr"}, lr=lr, capturable=capturable)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[3], gamma=0.1)
    return params, opt, sched


def _set_grads(params, step, dev):
    for p, g in zip(params, GRADS[step - 1]):
        p.grad = None if g is None else torch.from_numpy(g.copy()).to(dev)


def _run(name, dev, capturable=False, steps=gm.STEPS, on_step=None):
    params, opt, sched = _make(name, dev, capturable)
    for step in range(1, steps + 1):
        _set_grads(params, step, dev)
        opt.step()
        sched.step()
        if on_step is not None:
            on_step(step, params, opt)
    torch.cuda.synchronize()
    return params, opt


def _compare(name, step, params, opt, z):
    cls_name, kw = gm.CONFIGS[name]
    lr = kw["lr"]
    worst = 0.0
    for i, p in enumerate(params):
        idx = gm.sample_index(p.numel())
        pre = "s%d/" % step
        b = z[pre + "param/%d" % i]
        a = p.detach().reshape(-1).cpu().numpy()[idx]
        t = step
        ulp = np.spacing(np.abs(b).astype(np.float32))
        bound = 4 * ulp + 1e-5 * lr * t
        err = np.abs(a.astype(np.float64) - b)
        assert (err <= bound).all(), (name, step, i, float((err / ulp).max()))
        worst = max(worst, float((err / ulp).max()))
        st = opt.state.get(p, {})
        for k in gm.STATE_KEYS:
            key = pre + "%s/%d" % (k, i)
            assert (key in z) == (k in st), (name, step, i, k)
            if key in z:
                got = st[k].reshape(-1).cpu().numpy()[idx].astype(np.float64)
                ref = z[key].astype(np.float64)
                assert (np.abs(got - ref) <= 1e-6 * np.abs(ref) + 1e-30).all(), (name, step, i, k)
        want_step = int(z[pre + "step/%d" % i])
        if want_step >= 0:
            s = st["step"]
            assert (float(s) if torch.is_tensor(s) else s) == want_step
            assert torch.is_tensor(s) == opt.capturable
    return worst


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("name", list(gm.CONFIGS))
def test_matches_reference_fixture(name, capturable, dev):
    _check_fixture(name, capturable, dev)


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
@pytest.mark.parametrize("name", list(gm.CONFIGS))
def test_matches_reference_fixture_on_eight_cus(name, capturable, dev):
    """The same fixture check with the persistent grid sized for 8 CUs (the data-parallel reservation knob): the grid
    is min(chunks, 8 x 8) workgroups, so every workgroup walks several chunks (grid-stride loop) and the capturable
    arrival counter counts fewer arrivals than chunks."""
    from tests.helpers import usable_cus
    with usable_cus(8) as u:
        opt = _check_fixture(name, capturable, dev)
        n_chunks = max(t.n_chunks for t in opt._tables.values())
        assert n_chunks > 8 * u.cus, (n_chunks, u.cus)   # optim.hip launch(): grid = min(n_chunks, 8 * cus)


def _check_fixture(name, capturable, dev):
    z = np.load(os.path.join(GOLDEN, "optim_%s.npz" % name))
    worst = []
    _, opt = _run(name, dev, capturable, on_step=lambda step, params, opt: worst.append(_compare(name, step, params, opt, z))
                  if step in gm.RECORD else None)
    WORST_ULP[(name, capturable)] = max(worst)
    print("%s %s: worst parameter error %.1f ulp" % (name, "capturable" if capturable else "eager", max(worst)))
    return opt


@pytest.mark.parametrize("name", ["adamw_amsgrad", "adabound", "sgdw_nesterov"])
def test_bitwise_deterministic(name, dev):
    a, _ = _run(name, dev)
    b, _ = _run(name, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_reference_state_dict_loads_and_continues(dev, tmp_path):
    """A reference-format state (int steps, CPU tensors; here: our eager state after step 3 moved to the CPU, which the
    fixture pins to the reference's) loads into a fresh fused optimizer and the next steps match the fixture; a .tar saved
    by save_checkpoint mid-run and resumed continues bit for bit like the uninterrupted run."""
    from unet_nested4tiny_objects_keypoints_amd.checkpoint import resume, save_checkpoint
    name = "adabound"
    z = np.load(os.path.join(GOLDEN, "optim_%s.npz" % name))
    params, opt, sched = _make(name, dev)
    for step in range(1, 4):
        _set_grads(params, step, dev)
        opt.step()
        sched.step()
    sd = opt.state_dict()
    ref_sd = {"state": {k: {kk: (vv.cpu() if torch.is_tensor(vv) else vv) for kk, vv in v.items()}
                        for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]}
    assert all(isinstance(v["step"], int) for v in ref_sd["state"].values())
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList(params)
    ckpt = save_checkpoint(model, opt, 3, str(tmp_path / "mid.tar"))
    mid_params = [p.detach().clone() for p in params]
    for step in range(4, 7):                       # uninterrupted
        _set_grads(params, step, dev)
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    _compare(name, 6, params, opt, z)
    final = [p.detach().clone() for p in params]

    p2, opt2, sched2 = _make(name, dev)            # resumed from the .tar
    m2 = torch.nn.Module()
    m2.ps = torch.nn.ParameterList(p2)
    assert resume(m2, ckpt, opt2, resume_opt=True) == 4
    sched2.last_epoch = 3                          # the scheduler is not in the .tar (nor in the reference trainer's)
    for step in range(4, 7):
        _set_grads(p2, step, dev)
        opt2.step()
        sched2.step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(p2, final))

    p3, opt3, sched3 = _make(name, dev)            # a reference-format dict: CPU tensors, int steps
    with torch.no_grad():
        for q, v in zip(p3, mid_params):
            q.copy_(v)
    opt3.load_state_dict(ref_sd)
    assert isinstance(next(iter(opt3.state.values()))["step"], int)
    sched3.last_epoch = 3
    for step in range(4, 7):
        _set_grads(p3, step, dev)
        opt3.step()
        sched3.step()
    torch.cuda.synchronize()
    _compare(name, 6, p3, opt3, z)


def test_pack_plan_and_versions(dev):
    """train_step with the fused AdamW on an fs4 network: bit-identical with the weight-image pack plan on and off, and
    p._version untouched (the update writes through raw pointers, as the reference writes through p.data)."""
    import copy

    from unet_nested4tiny_objects_keypoints_amd import AdamW, FocalLoss_BCE_2d, UNet_Nested, engine, train_step
    torch.manual_seed(22)
    m = UNet_Nested(in_channels=1, n_classes=4, feature_scale=4).to(dev).train()
    m.drop_out.p = 0.0
    ref = copy.deepcopy(m)
    x = torch.randn(2, 1, 32, 32, device=dev)
    t = torch.rand(2, 4, 32, 32, device=dev)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    opt_m, opt_r = AdamW(m.parameters(), lr=1e-2, weight_decay=1e-4), AdamW(ref.parameters(), lr=1e-2, weight_decay=1e-4)
    v0 = [p._version for p in m.parameters()]
    losses = []
    for step in range(4):
        outs_m, loss_m = train_step(m, opt_m, crit, x, t)
        engine.USE_PACK_PLAN = False
        try:
            outs_r, loss_r = train_step(ref, opt_r, crit, x, t)
        finally:
            engine.USE_PACK_PLAN = True
        assert all(torch.equal(a, b) for a, b in zip(outs_m, outs_r)), step
        assert torch.equal(loss_m, loss_r), step
        for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
            assert torch.equal(p, q), (step, k)
        losses.append(float(loss_m))
    assert [p._version for p in m.parameters()] == v0
    assert len(set(losses)) == 4


def test_at_most_two_launches_per_step(dev):
    from torch.profiler import ProfilerActivity, profile
    params, opt, sched = _make("adamw", dev)
    _set_grads(params, 1, dev)
    opt.step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(3):
            opt.step()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    names = [e.name for e in kernels]
    assert 1 <= len([n for n in names if "optim_kernel" in n]) <= 3 * 1, names
    assert len(kernels) <= 3 * 2, names


def test_graphed_capture_matches_eager(dev):
    """GraphedTrainStep(capture_optimizer=True) with AdamW(capturable=True) equals eager train_step with the same
    optimizer, bit for bit, over 3 replays."""
    import copy

    from unet_nested4tiny_objects_keypoints_amd import AdamW, FocalLoss_BCE_2d, GraphedTrainStep, UNet_Nested, train_step
    torch.manual_seed(5)
    m = UNet_Nested(in_channels=1, n_classes=4, feature_scale=4).to(dev).train()
    m.drop_out.p = 0.0
    ref = copy.deepcopy(m)
    x = torch.randn(2, 1, 32, 32, device=dev)
    t = torch.rand(2, 4, 32, 32, device=dev)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    opt_g = AdamW(m.parameters(), lr=1e-2, weight_decay=1e-4, capturable=True)
    opt_e = AdamW(ref.parameters(), lr=1e-2, weight_decay=1e-4, capturable=True)
    g = GraphedTrainStep(m, opt_g, crit, x, t, capture_optimizer=True)
    for step in range(3):
        outs_g, loss_g = g(x, t)
        outs_e, loss_e = train_step(ref, opt_e, crit, x, t)
        torch.cuda.synchronize()
        assert torch.equal(loss_g, loss_e), step
        for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
            assert torch.equal(p, q), (step, k)
    for p, q in zip(m.parameters(), ref.parameters()):
        sg, se = opt_g.state[p], opt_e.state[q]
        assert float(sg["step"]) == float(se["step"]) == 3.0
        assert torch.equal(sg["exp_avg"], se["exp_avg"]) and torch.equal(sg["exp_avg_sq"], se["exp_avg_sq"])
