"""Frozen BatchNorm through the whole network: every BatchNormParams obeys its OWN ``training`` flag, and a layer that
normalised with its running statistics back-propagates through the one-pass kernel (unetpp_bn_frozen_bwd).  Against
``UNetNestedOracle`` / ``UNetOracle`` in float64 -- real ``nn.BatchNorm2d`` modules put into the same modes -- with the
HIP forward's ReLU gates and pool winners (tests/helpers.install_hip_gates, check_flips with their caps).  Bar: 1e-4.

The BatchNorm buffers get real values (seeded_state, then running_mean ~ N(0, 0.5^2), running_var ~ U(0.5, 2)).  Under a
frozen layer the bias of the convolution before it is an ordinary parameter (its gradient is as large as the weight's), so
tests/helpers.assert_grads_close's noise rule applies only to biases that feed a layer still in training mode.
"""

import pytest
import torch

from tests.helpers import check_flips, install_hip_gates, install_hip_gates_plain, load_golden, rel_err, seeded_state

pytestmark = pytest.mark.gpu

TOL = 1e-4
BF = torch.bfloat16
C1 = dict(in_channels=1, n_classes=4, feature_scale=4)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def real_state(oracle, seed):
    """seeded_state with running statistics a trained network would have"""
    state = seeded_state(oracle, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    for k, v in state.items():
        if k.endswith("running_mean"):
            state[k] = 0.5 * torch.randn(v.shape, generator=g)
        elif k.endswith("running_var"):
            state[k] = 0.5 + 1.5 * torch.rand(v.shape, generator=g)
    return state


def bn_layers(m):
    from unet_nested4tiny_objects_keypoints_amd.unet import BatchNormParams
    return [(k, mod) for k, mod in m.named_modules() if isinstance(mod, BatchNormParams)]


def mirror_modes(m, ref):
    """The oracle's nn.BatchNorm2d modules and parameters in the modes / requires_grad of the HIP model's holders."""
    ref.train(m.training)
    for k, mod in bn_layers(m):
        ref.get_submodule(k).train(mod.training)
    for (k, p), (kr, pr) in zip(m.named_parameters(), ref.named_parameters()):
        assert k == kr
        pr.requires_grad_(p.requires_grad)


def loss_dev(outs, target):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    if not isinstance(outs, tuple):
        return crit(outs, target)
    return sum(crit(o, target) for o in outs) / len(outs)


def loss_cpu(outs, target):
    from oracle.step_oracle import focal_bce_2d_oracle
    if not isinstance(outs, tuple):
        return focal_bce_2d_oracle(outs, target.to(outs.dtype))
    return sum(focal_bce_2d_oracle(o, target.to(o.dtype)) for o in outs) / len(outs)


def feeds_training_bn(k, m):
    """k names the bias of a convolution whose BatchNorm is in training mode (batch mean removes it: rounding noise)."""
    if not k.endswith(".bias"):
        return False
    head, _, idx = k[:-len(".bias")].rpartition(".")
    if not head or not idx.isdigit():
        return False
    from unet_nested4tiny_objects_keypoints_amd.unet import BatchNormParams
    try:
        nxt = m.get_submodule("%s.%d" % (head, int(idx) + 1))
    except AttributeError:
        return False
    return isinstance(nxt, BatchNormParams) and nxt.training


def hip_step(m, x, target, dev):
    """forward + backward of the HIP model with an input gradient -> (outs, loss, dx); parameter grads in p.grad"""
    m.zero_grad(set_to_none=True)
    m._debug_keep_saved = True
    xg = x.to(dev).requires_grad_(True)
    outs = m(xg)
    loss = loss_dev(outs, target.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return outs, loss.detach(), xg.grad


def compare_with_oracle(m, ref, gate_installer, x, target, outs, loss, dx, buf0, label):
    """ref: the float64 oracle holding the same state, modes mirrored.  Everything the issue lists for cases (a)-(d), (f)."""
    gated = gate_installer(ref, m._debug_saved)
    x64 = x.double().requires_grad_(True)
    ro = ref(x64)
    rl = loss_cpu(ro, target.double())
    rl.backward()
    check_flips(gated, label)
    for o, r in zip(outs if isinstance(outs, tuple) else (outs,), ro if isinstance(ro, tuple) else (ro,)):
        assert rel_err(o.detach().cpu(), r.detach()) < TOL, label
    assert abs(float(loss) - float(rl.detach())) <= TOL * abs(float(rl.detach())), (float(loss), float(rl.detach()))
    assert rel_err(dx.cpu(), x64.grad) < TOL, ("input gradient", rel_err(dx.cpu(), x64.grad))
    want = dict(ref.named_parameters())
    bad = []
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None and want[k].grad is None, k
            continue
        assert p.grad is not None, k
        g, w = p.grad.cpu(), want[k].grad
        if feeds_training_bn(k, m):
            scale = float(want[k[:-len("bias")] + "weight"].grad.abs().max())
            if not float(g.abs().max()) <= 1e-3 * scale + 1e-30:
                bad.append((k, "pre-BN bias", float(g.abs().max()), scale))
        elif not rel_err(g, w) < TOL:
            bad.append((k, rel_err(g, w)))
    assert not bad, bad
    frozen = {k for k, mod in bn_layers(m) if not mod.training}
    refbuf = dict(ref.named_buffers())
    for k, b in m.named_buffers():
        if k.rsplit(".", 1)[0] in frozen:
            assert torch.equal(b.cpu(), buf0[k]), ("a frozen layer's buffer changed", k)
        elif b.dtype.is_floating_point:
            assert rel_err(b.cpu(), refbuf[k]) < TOL, k
        else:
            assert int(b) == int(refbuf[k]) == int(buf0[k]) + 1, k


def nested_case(dev, ctor, b, h, w, setup, seed, label):
    from oracle.unet_nested_oracle import UNetNestedOracle
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    ref = UNetNestedOracle(**ctor)
    state = real_state(ref, seed)
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.randn(b, ctor["in_channels"], h, w, generator=g)
    target = torch.rand(b, ctor["n_classes"], h, w, generator=g)
    m = UNet_Nested(**ctor)
    m.load_state_dict(state)
    m = m.to(dev)
    setup(m)
    m.drop_out.eval()
    buf0 = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
    outs, loss, dx = hip_step(m, x, target, dev)
    ref.load_state_dict(state)
    ref = ref.double()
    mirror_modes(m, ref)
    ref.drop_out.eval()
    compare_with_oracle(m, ref, install_hip_gates, x, target, outs, loss, dx, buf0, label)
    return m, x, target, outs, loss, dx


class count_calls:
    """Counts the calls of one entry point of the loaded library for the duration of a block."""

    def __init__(self, name):
        self.name, self.calls = name, 0

    def __enter__(self):
        from unet_nested4tiny_objects_keypoints_amd import _lib
        self.lib = _lib.lib()
        self.orig = getattr(self.lib, self.name)

        def wrapped(*a):
            self.calls += 1
            return self.orig(*a)
        setattr(self.lib, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.name, self.orig)
        return False


# --------------------------------------------------------------------------------------------- (a) eval mode with grad
def test_eval_mode_backward_vs_oracle(dev):
    m, *_ = nested_case(dev, C1, 4, 64, 64, lambda m: m.eval(), 11, "frozen:eval")
    assert all(p.grad is not None for p in m.parameters())   # gamma and beta of a frozen layer included


# --------------------------------------------------------------------------------------------- (b), (g) frozen, training mode
def test_frozen_training_mode_vs_oracle_and_bitwise(dev):
    with count_calls("unetpp_bn_bwd_finalize") as fin, count_calls("unetpp_bn_frozen_bwd") as frz:
        m, x, target, outs, loss, dx = nested_case(dev, C1, 4, 64, 64, lambda m: m.train().freeze_batchnorm(), 12,
                                                   "frozen:train")
    n_bn = len(bn_layers(m))
    assert n_bn == 2 * m.depth and frz.calls == n_bn
    assert fin.calls == 0   # gamma and beta frozen too: no sums, no finalize launch
    for k, mod in bn_layers(m):
        assert not mod.training and mod.weight.grad is None and mod.bias.grad is None, k
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    # outputs: the bits of model.eval() under no_grad
    m.eval()
    with torch.no_grad():
        ev = m(x.to(dev))
    assert all(torch.equal(a, b) for a, b in zip(outs, ev))
    # (g) a second run: every output and gradient again, bit for bit
    m.train().freeze_batchnorm()
    m.drop_out.eval()   # (train() switched the dropout holder on again)
    outs2, loss2, dx2 = hip_step(m, x, target, dev)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2)) and torch.equal(loss, loss2) and torch.equal(dx, dx2)
    for k, p in m.named_parameters():
        assert (p.grad is None) == (k not in grads) and (p.grad is None or torch.equal(p.grad, grads[k])), k
    # affine=False: gamma and beta get their sums (one finalize per layer); every other gradient keeps its bits
    m.train().freeze_batchnorm(affine=False)
    m.drop_out.eval()
    for _, mod in bn_layers(m):
        mod.weight.requires_grad_(True)
        mod.bias.requires_grad_(True)
    with count_calls("unetpp_bn_bwd_finalize") as fin:
        outs3, _, dx3 = hip_step(m, x, target, dev)
    assert fin.calls == n_bn
    assert all(torch.equal(a, b) for a, b in zip(outs, outs3)) and torch.equal(dx, dx3)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        if k in grads:
            assert torch.equal(p.grad, grads[k]), k


# --------------------------------------------------------------------------------------------- (c) mixed modes
def _freeze_levels_0_1(m):
    m.train()
    for k, mod in bn_layers(m):
        if k.startswith("conv00.") or k.startswith("conv10."):
            mod.eval()


def _freeze_first_stage(m):
    m.train()
    for k, mod in bn_layers(m):
        if ".conv1." in k:
            mod.eval()


@pytest.mark.parametrize("setup", [_freeze_levels_0_1, _freeze_first_stage], ids=["levels-0-1", "conv1.1-of-every-block"])
def test_mixed_modes_vs_oracle(dev, setup):
    m, *_ = nested_case(dev, C1, 4, 64, 64, setup, 13, "frozen:mixed:" + setup.__name__)
    modes = [mod.training for _, mod in bn_layers(m)]
    assert any(modes) and not all(modes)


# --------------------------------------------------------------------------------------------- (d) structure variants
@pytest.mark.parametrize("name", ["d5_fs8_bilinear_32x48_b2", "fs8_rgb5_24x40_b2"])
def test_structure_variants_vs_oracle(dev, name):
    z, ctor = load_golden(name)
    b, _, h, w = z["x"].shape
    nested_case(dev, ctor, b, h, w, lambda m: m.train().freeze_batchnorm(affine=False), 14, "frozen:" + name)


# --------------------------------------------------------------------------------------------- (e) bf16 storage
def test_bf16_frozen_step_vs_oracles(dev):
    """One step with every BatchNorm frozen in bf16 storage, held to the bounds tests/test_gpu_bf16.py::
    test_bf16_train_step_vs_oracles states for the training-mode step (no looser): against the fp32 oracle outputs <= 3e-2
    (mean <= 4e-3) and loss 2e-3; against the oracle with the bf16 path's roundings (oracle/bf16_sim.py) every parameter
    gradient <= 6 % relative L2 with cosine >= 0.998; against the float64 oracle with the HIP routing <= 10 %.  Buffers
    do not move at all."""
    from oracle.bf16_sim import forward_bf16_sim, routing_of
    from oracle.unet_nested_oracle import UNetNestedOracle
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    ctor, b, h, w = C1, 4, 64, 64
    ref = UNetNestedOracle(**ctor)
    state = real_state(ref, 15)
    ref.load_state_dict(state)
    g = torch.Generator().manual_seed(16)
    x, target = torch.randn(b, 1, h, w, generator=g), torch.rand(b, 4, h, w, generator=g)
    m = UNet_Nested(**ctor)
    m.load_state_dict(state)
    m = m.to(dev).train().set_activation_dtype(BF).freeze_batchnorm()
    m.drop_out.eval()
    buf0 = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
    m._debug_keep_saved = True
    m.zero_grad(set_to_none=True)
    outs = m(x.to(dev))
    loss = loss_dev(outs, target.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    for k, v in m.named_buffers():
        assert torch.equal(v.cpu(), buf0[k]), k
    mirror_modes(m, ref)
    ref.drop_out.eval()
    ro = ref(x)
    rl = loss_cpu(ro, target)
    out_max = max(float((o.detach().cpu() - r.detach()).abs().max()) for o, r in zip(outs, ro))
    out_mean = max(float((o.detach().cpu() - r.detach()).abs().mean()) for o, r in zip(outs, ro))
    loss_rel = abs(float(loss.detach()) - float(rl.detach())) / abs(float(rl.detach()))
    so = forward_bf16_sim(ref, x, training=False, routing=routing_of(m._debug_saved), stats={})
    loss_cpu(so, target).backward()
    gsim = {k: p.grad.double().clone() for k, p in ref.named_parameters() if p.grad is not None}
    routed = UNetNestedOracle(**ctor)
    routed.load_state_dict(state)
    routed = routed.double()
    mirror_modes(m, routed)
    routed.drop_out.eval()
    install_hip_gates(routed, m._debug_saved)
    loss_cpu(routed(x.double()), target.double()).backward()
    grouted = {k: p.grad.double().clone() for k, p in routed.named_parameters() if p.grad is not None}
    sim_l2, cos, routed_l2 = {}, {}, {}
    for k, p in m.named_parameters():
        if not p.requires_grad:
            assert p.grad is None and k not in gsim, k
            continue
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), k
        gd = p.grad.double().cpu().flatten()
        sim_l2[k] = float((gd - gsim[k].flatten()).norm() / gsim[k].norm())
        routed_l2[k] = float((gd - grouted[k].flatten()).norm() / grouted[k].norm())
        cos[k] = float(torch.dot(gd, gsim[k].flatten()) / (gd.norm() * gsim[k].norm()))
    line = {"out_max": out_max, "out_mean": out_mean, "loss_rel": loss_rel,
            "worst_grad_l2_vs_bf16_sim": max(sim_l2.items(), key=lambda kv: kv[1]), "min_cos": min(cos.values()),
            "worst_grad_l2_vs_fp64_routed": max(routed_l2.items(), key=lambda kv: kv[1])}
    print("bf16 frozen vs oracles:", line)
    assert out_max <= 3e-2 and out_mean <= 4e-3, line
    assert loss_rel <= 2e-3, line
    assert max(sim_l2.values()) <= 0.06 and min(cos.values()) >= 0.998, line
    assert max(routed_l2.values()) <= 0.10, line


# --------------------------------------------------------------------------------------------- (f) classic UNet
def test_plain_unet_eval_mode_backward_vs_oracle(dev):
    from oracle.unet_plain_oracle import UNetOracle
    from unet_nested4tiny_objects_keypoints_amd import UNet
    z, ctor = load_golden("unet_w8_rgb5_32x48_b2")
    ref = UNetOracle(**ctor)
    state = real_state(ref, 17)
    g = torch.Generator().manual_seed(18)
    x = torch.randn(tuple(z["x"].shape), generator=g)
    target = torch.rand(tuple(z["target"].shape), generator=g)
    m = UNet(**ctor)
    m.load_state_dict(state)
    m = m.to(dev).eval()
    buf0 = {k: v.detach().cpu().clone() for k, v in m.named_buffers()}
    out, loss, dx = hip_step(m, x, target, dev)
    ref.load_state_dict(state)
    ref = ref.double()
    mirror_modes(m, ref)
    compare_with_oracle(m, ref, install_hip_gates_plain, x, target, out, loss, dx, buf0, "frozen:plain-unet-eval")
    # freeze_batchnorm is the same method on the classic network
    assert m.train().freeze_batchnorm() is m and not any(mod.training for _, mod in bn_layers(m))
    out2, _, dx2 = hip_step(m, x, target, dev)
    assert torch.equal(out2, out) and torch.equal(dx2, dx)
    assert all(torch.equal(b.cpu(), buf0[k]) for k, b in m.named_buffers())


# --------------------------------------------------------------------------------------------- data-parallel delivery
def test_data_parallel_delivery_with_frozen_batchnorm(dev):
    """dp.py's contract with frozen gamma / beta: the averager is told that they are done (its frontier reaches the end of
    the flat buffer), they get no gradient (p.grad stays None), and every other gradient has the bits of the unhooked
    backward.  A world of one in this process (gloo, in-memory store): no collective is issued."""
    import torch.distributed as dist

    from oracle.unet_nested_oracle import UNetNestedOracle
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, dp
    ctor = dict(in_channels=1, n_classes=4, feature_scale=8)
    state = real_state(UNetNestedOracle(**ctor), 19)
    g = torch.Generator().manual_seed(20)
    x, target = torch.randn(2, 1, 32, 32, generator=g), torch.rand(2, 4, 32, 32, generator=g)
    m = UNet_Nested(**ctor)
    m.load_state_dict(state)
    m = m.to(dev).train().freeze_batchnorm()
    m.drop_out.eval()
    _, _, dx = hip_step(m, x, target, dev)
    want = {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
    assert not dist.is_initialized()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        avg = dp.GradientAverager(dp.ready_order(m), bucket_bytes=16 << 10).attach(m)
        _, _, dx2 = hip_step(m, x, target, dev)
        assert len(avg.buckets_last_step) >= 2 and avg.buckets_last_step[-1][1] == avg.flat.numel()
        for k, p in m.named_parameters():
            if want[k] is None:
                assert not p.requires_grad and p.grad is None, k
            else:
                assert p.grad is not None and torch.equal(p.grad, want[k]), k
        assert torch.equal(dx2, dx)
    finally:
        m._grad_alloc = m._grad_sink = m._grad_done = None
        dist.destroy_process_group()


# --------------------------------------------------------------------------------------------- (h) infer()
def test_infer_refuses_a_layer_in_training_mode(dev):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    m = UNet_Nested(**C1).to(dev).eval()
    x = torch.randn(1, 1, 32, 32, device=dev)
    want = m.infer(x, 1)
    getattr(m.conv10.conv2, "1").train()
    with pytest.raises(RuntimeError, match=r"conv10\.conv2\.1"):
        m.infer(x, 1)
    getattr(m.conv10.conv2, "1").eval()
    getattr(m.conv30.conv1, "1").train()        # head 1 does not run level 3: not its business
    assert torch.equal(m.infer(x, 1), want)
    with pytest.raises(RuntimeError, match=r"conv30\.conv1\.1"):
        m.infer(x)
