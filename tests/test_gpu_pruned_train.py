"""Training the network cut at a deep-supervision head: ``UNet_Nested.forward_pruned``, ``train_step(..., head=J)``, the
graphed step, the data-parallel averager of a cut and the fine-tune loop of a pruned checkpoint.

Weights and inputs are the committed fixtures (tests/helpers.py GOLDEN_CASES + DEPTH_CASES, 32x32 to 64x64, batch 2 to 4).
The reference for gradients is oracle.UNetNestedOracle in float64 with the focal loss summed over heads 1 .. J and divided
by J; its backward takes the ReLU gates and max-pool winners of the HIP forward (tests/helpers.py: GatedReLU,
RoutedMaxPool) on the nodes of the cut -- the oracle's own full forward also runs the nodes outside, which receive no
gradient from such a loss (checked first, on the CPU) and move BatchNorm buffers the cut network does not contain, so
buffers are compared inside the cut only."""
import copy

import pytest
import torch

from tests.helpers import (DEPTH_CASES, GOLDEN_CASES, GatedReLU, RoutedMaxPool, assert_grads_close, check_flips,
                           is_pre_bn_bias, load_golden, rel_err, seeded_state, sub)

pytestmark = [pytest.mark.gpu,
              pytest.mark.filterwarnings("error:.*AccumulateGrad node's stream does not match.*")]

TOL = 1e-4
BF = torch.bfloat16
ALL_CASES = GOLDEN_CASES + DEPTH_CASES


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _bf16_ok(ctor):
    fs, depth = ctor.get("feature_scale", 2), ctor.get("depth", 4)
    widths = [int(w / fs) for w in (32, 64, 128, 256, 512)[:depth]]
    return all(w % 8 == 0 and (w // 8) & (w // 8 - 1) == 0 for w in widths)


def _cuts(cases=ALL_CASES, proper_only=False, bf16=False):
    """(fixture, J) for every head of every fixture (proper_only: J < depth - 1; bf16: fixtures bf16 storage takes)"""
    out = []
    for name in cases:
        ctor = load_golden(name)[1]
        d = ctor.get("depth", 4)
        if bf16 and not _bf16_ok(ctor):
            continue
        out += [(name, j) for j in range(1, d - 1 if proper_only else d)]
    return out


def _ids(cuts):
    return ["%s-head%d" % c for c in cuts]


def _model(ctor, state, dev, dt="fp32"):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    m = UNet_Nested(**ctor)
    m.load_state_dict(state, strict=True)
    m = m.to(dev).train()
    if dt == "bf16":
        m.set_activation_dtype(BF)
    return m


def _seeded(dev, dt="fp32", seed=3, **ctor):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    kw = dict(in_channels=1, n_classes=4, feature_scale=4)
    kw.update(ctor)
    return _model(kw, seeded_state(UNet_Nested(**kw), seed), dev, dt), kw


def _crit():
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    return FocalLoss_BCE_2d(gamma=3, size_average=False)


def _loss(outs, target):
    crit = _crit()
    return sum(crit(o, target) for o in outs) / len(outs)


def _prefixes(depth, head):
    from unet_nested4tiny_objects_keypoints_amd.checkpoint import _pruned_prefixes
    return _pruned_prefixes(depth, head)


def _encoder_buffers(m, lo, hi):
    """named buffers of conv{lo}0 .. conv{hi-1}0"""
    names = tuple("conv%d0." % i for i in range(lo, hi))
    return {k: b for k, b in m.named_buffers() if k.startswith(names)}


# ------------------------------------------------------------------------------------------------ oracle precondition
@pytest.mark.parametrize("depth", [3, 4, 5])
@pytest.mark.parametrize("is_deconv", [True, False])
@pytest.mark.parametrize("is_batchnorm", [True, False])
def test_oracle_gives_gradients_exactly_inside_the_cut(depth, is_deconv, is_batchnorm):
    """CPU, float64: under the loss over heads 1 .. J every parameter outside the pruned prefixes has ``grad is None`` and
    every parameter inside a non-zero gradient (a convolution bias in front of a BatchNorm has an analytically zero one:
    it is only required to exist), so "outside: None, inside: compared" leaves no parameter out."""
    from oracle.step_oracle import focal_bce_2d_oracle
    from oracle.unet_nested_oracle import UNetNestedOracle
    ctor = dict(in_channels=1, n_classes=2, feature_scale=8, is_deconv=is_deconv, is_batchnorm=is_batchnorm, depth=depth)
    torch.manual_seed(depth)
    ref = UNetNestedOracle(**ctor).double().train()
    ref.drop_out.eval()
    x, t = torch.randn(2, 1, 32, 32, dtype=torch.float64), torch.rand(2, 2, 32, 32, dtype=torch.float64)
    for head in range(1, depth):
        ref.zero_grad(set_to_none=True)
        outs = ref(x)
        (sum(focal_bce_2d_oracle(o, t) for o in outs[:head]) / head).backward()
        prefixes = _prefixes(depth, head)
        for k, p in ref.named_parameters():
            if k.startswith(prefixes):
                assert p.grad is not None, (head, k)
                assert is_pre_bn_bias(k, ctor) or float(p.grad.abs().max()) > 0, (head, k)
            else:
                assert p.grad is None, (head, k)


# ------------------------------------------------------------------------------------------------ forward bits
def _masks(ctor, x, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    fs = int(32 / ctor.get("feature_scale", 2))
    b, _, h, w = x.shape
    return [(torch.rand(b, h, w, fs, generator=g, device=dev) >= 0.4).to(torch.uint8) for _ in range(ctor.get("depth", 4) - 1)]


@pytest.mark.parametrize("name,head", _cuts(), ids=_ids(_cuts()))
@pytest.mark.parametrize("mode", ["generated", "masks"])
def test_training_forward_equals_the_whole_forward_bit_for_bit(dev, name, head, mode):
    z, ctor = load_golden(name)
    d = ctor.get("depth", 4)
    whole = _model(ctor, sub(z, "state0"), dev)
    cut = copy.deepcopy(whole)
    x = torch.from_numpy(z["x"]).to(dev)
    before = {k: b.clone() for k, b in cut.named_buffers()}
    assert whole.drop_out.training and whole.drop_out.p > 0
    if mode == "masks":
        whole.dropout_masks = _masks(ctor, x, dev, 17)
        cut.dropout_masks = [mk.clone() for mk in whole.dropout_masks]
    torch.manual_seed(1234 + head)
    want = whole(x)
    torch.manual_seed(1234 + head)
    got = cut.forward_pruned(x, head)
    assert isinstance(got, tuple) and len(got) == head
    for j in range(head):
        assert got[j].grad_fn is not None and got[j].dtype == torch.float32
        assert torch.equal(got[j], want[j]), (name, head, j)
    inside, deeper = _encoder_buffers(cut, 0, head + 1), _encoder_buffers(cut, head + 1, d)
    ref_bufs = dict(whole.named_buffers())
    for k, b in inside.items():
        assert torch.equal(b, ref_bufs[k]), k
    for k, b in deeper.items():
        assert torch.equal(b, before[k]), k
    if ctor.get("is_batchnorm", True):
        assert inside and all(not torch.equal(b, before[k]) for k, b in inside.items() if k.endswith("num_batches_tracked"))
        assert deeper or head == d - 1


@pytest.mark.parametrize("name,head", _cuts(), ids=_ids(_cuts()))
def test_eval_forward_equals_infer_bit_for_bit(dev, name, head):
    z, ctor = load_golden(name)
    for dt in ("fp32", "bf16") if _bf16_ok(ctor) else ("fp32",):
        m = _model(ctor, sub(z, "state0"), dev, dt).eval()
        x = torch.from_numpy(z["x"]).to(dev)
        before = {k: b.clone() for k, b in m.named_buffers()}
        got = m.forward_pruned(x, head)
        assert len(got) == head and all(o.grad_fn is not None for o in got)
        for j in range(1, head + 1):
            assert torch.equal(got[j - 1], m.infer(x, j)), (name, dt, head, j)
        with torch.no_grad():
            quiet = m.forward_pruned(x, head)
        assert all(o.grad_fn is None and torch.equal(o, p) for o, p in zip(quiet, got))
        assert all(torch.equal(b, before[k]) for k, b in m.named_buffers())


# ------------------------------------------------------------------------------------------------ gradients
class _CutRoutedMaxPool(RoutedMaxPool):
    """the oracle's shared max-pool: the levels inside the cut route to the HIP forward's winners, the deeper levels -- which
    the cut does not contain and whose gradient is zero -- pool as they always did"""

    def forward(self, x):
        if self.calls >= len(self.hip_idx):
            self.calls += 1
            return torch.nn.functional.max_pool2d(x, 2)
        return super().forward(x)


def install_cut_gates(oracle_model, hip_saved, head):
    """tests/helpers.install_hip_gates for the nodes of a cut: hip_saved holds exactly needed_nodes(depth, head)."""
    from unet_nested4tiny_objects_keypoints_amd.engine import needed_nodes
    gated = []

    def nchw_mask(t):
        return (t.permute(0, 3, 1, 2) > 0).cpu()

    assert sorted(hip_saved.pairs) == sorted(needed_nodes(oracle_model.depth, head))
    for (i, j), rec in hip_saved.pairs.items():
        pair = getattr(oracle_model, "conv%d0" % i) if j == 0 else getattr(oracle_model, "up_concat%d%d" % (i, j)).conv
        a1 = rec.a1
        if a1 is None:
            scale, shift = rec.bn1[2].double(), rec.bn1[3].double()
            a1 = (rec.y1.double() * scale + shift).float()
        for seq, act in ((pair.conv1, a1), (pair.conv2, rec.out)):
            mod = GatedReLU(nchw_mask(act))
            seq[len(seq) - 1] = mod
            gated.append(mod)
    assert all(hip_saved.pairs[(i, 0)].pool_idx is not None for i in range(head))
    assert hip_saved.pairs[(head, 0)].pool_idx is None            # the deepest encoder node of the cut is not pooled
    pool = _CutRoutedMaxPool([hip_saved.pairs[(i, 0)].pool_idx.cpu() for i in range(head)])
    oracle_model.maxpool = pool
    gated.append(pool)
    return gated


def _oracle_step(ctor, state, x, target, head, saved, ensemble=False, loss="focal", train=True):
    """float64 oracle with the HIP forward's routing inside the cut -> (outputs, parameter grads inside the cut, input grad,
    gate stand-ins, buffers)"""
    from oracle.step_oracle import focal_bce_2d_oracle
    from oracle.unet_nested_oracle import UNetNestedOracle
    ref = UNetNestedOracle(**ctor)
    ref.load_state_dict(state)
    ref = ref.double()
    ref.train(train)
    ref.drop_out.eval()
    gated = install_cut_gates(ref, saved, head)
    xin = x.double().clone().requires_grad_(True)
    outs = ref(xin)[:head]
    if ensemble:
        mean = sum(outs) / head
        (mean.sum() if loss == "sum" else focal_bce_2d_oracle(mean, target.double())).backward()
        outs = (mean,)
    else:
        (sum(focal_bce_2d_oracle(o, target.double()) for o in outs) / head).backward()
    grads = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    return [o.detach() for o in outs], grads, xin.grad, gated, dict(ref.named_buffers())


@pytest.mark.parametrize("name,head", _cuts(), ids=_ids(_cuts()))
def test_cut_gradients_vs_float64_oracle(dev, name, head):
    z, ctor = load_golden(name)
    d = ctor.get("depth", 4)
    state = sub(z, "state0")
    m = _model(ctor, state, dev)
    m.drop_out.eval()
    m._debug_keep_saved = True
    x = torch.from_numpy(z["x"]).to(dev).requires_grad_(True)
    target = torch.from_numpy(z["target"]).to(dev)
    outs = m.forward_pruned(x, head)
    loss = _loss(outs, target)
    loss.backward()
    ro, want, want_dx, gated, ref_bufs = _oracle_step(ctor, state, x.detach().cpu(), target.cpu(), head, m._debug_saved)
    check_flips(gated, "pruned-train:%s:head%d" % (name, head))
    for o, r in zip(outs, ro):
        assert rel_err(o.detach().cpu(), r) < TOL
    prefixes = _prefixes(d, head)
    got = {}
    for k, p in m.named_parameters():
        if k.startswith(prefixes):
            assert p.grad is not None, k
            got[k] = p.grad.cpu()
        else:
            assert p.grad is None, k
    assert sorted(got) == sorted(want)
    assert_grads_close(got, want, ctor, TOL)
    err = rel_err(x.grad.cpu(), want_dx)
    print("pruned-train %s head %d: input gradient rel_err %.3e" % (name, head, err))
    assert err < TOL
    for k, b in _encoder_buffers(m, 0, head + 1).items():       # buffers inside the cut (the oracle's deeper ones moved too)
        if b.dtype.is_floating_point:
            assert rel_err(b.cpu(), ref_bufs[k]) < TOL, k
        else:
            assert int(b) == int(ref_bufs[k]), k


@pytest.mark.parametrize("name,head", _cuts(bf16=True), ids=_ids(_cuts(bf16=True)))
def test_cut_gradients_bf16_storage_vs_float64_oracle(dev, name, head):
    """bf16 storage of the same cut under the bounds tests/test_gpu_bf16.py's whole-network test names for this comparison
    (test_bf16_train_step_vs_oracles): sigmoid outputs |err| <= 3e-2, loss 2e-3 relative, and every parameter gradient
    within BF16_GRAD_VS_FP32_ORACLE_ROUTED (relative L2) of the float64 oracle whose backward takes the bf16 forward's
    ReLU gates and pool winners."""
    from tests.test_gpu_bf16 import BF16_GRAD_VS_FP32_ORACLE_ROUTED
    z, ctor = load_golden(name)
    d = ctor.get("depth", 4)
    state = sub(z, "state0")
    m = _model(ctor, state, dev, "bf16")
    m.drop_out.eval()
    m._debug_keep_saved = True
    x = torch.from_numpy(z["x"]).to(dev)
    target = torch.from_numpy(z["target"]).to(dev)
    outs = m.forward_pruned(x, head)
    loss = _loss(outs, target)
    loss.backward()
    ro, want, _, _, _ = _oracle_step(ctor, state, x.cpu(), target.cpu(), head, m._debug_saved)
    from oracle.step_oracle import focal_bce_2d_oracle
    rl = sum(focal_bce_2d_oracle(o, target.cpu().double()) for o in ro) / head
    assert abs(float(loss.detach()) - float(rl)) <= 2e-3 * abs(float(rl))
    for o, r in zip(outs, ro):
        assert o.dtype == torch.float32 and float((o.detach().cpu().double() - r).abs().max()) <= 3e-2
    prefixes = _prefixes(d, head)
    worst = ("", 0.0)
    for k, p in m.named_parameters():
        if not k.startswith(prefixes):
            assert p.grad is None, k
            continue
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
        if is_pre_bn_bias(k, ctor):
            continue
        l2 = float((p.grad.double().cpu() - want[k]).norm() / want[k].norm())
        worst = max(worst, (k, l2), key=lambda kv: kv[1])
        assert l2 <= BF16_GRAD_VS_FP32_ORACLE_ROUTED, (k, l2)
    print("pruned-train bf16 %s head %d: worst relative L2 %.4f at %s" % (name, head, worst[1], worst[0]))


# ------------------------------------------------------------------------------------------------ full cut
@pytest.mark.parametrize("name", ALL_CASES)
def test_full_cut_is_the_whole_network_bit_for_bit(dev, name):
    """head = depth - 1 (and None): outputs, every gradient and every buffer equal model(x) + backward(), fp32 and bf16,
    with the in-kernel dropout on; the two models also hold the same weight-image plan phases."""
    z, ctor = load_golden(name)
    d = ctor.get("depth", 4)
    for dt in ("fp32", "bf16") if _bf16_ok(ctor) else ("fp32",):
        for head in (d - 1, None):
            whole = _model(ctor, sub(z, "state0"), dev, dt)
            cut = copy.deepcopy(whole)
            if dt == "bf16":
                cut.set_activation_dtype(BF)
            want_dx = ctor["in_channels"] <= 4 or dt == "fp32"
            xa = torch.from_numpy(z["x"]).to(dev).requires_grad_(want_dx)
            xb = torch.from_numpy(z["x"]).to(dev).requires_grad_(want_dx)
            target = torch.from_numpy(z["target"]).to(dev)
            for step in range(2):                                  # the second pass takes the batched weight-image launch
                whole.zero_grad(set_to_none=True)
                cut.zero_grad(set_to_none=True)
                xa.grad = xb.grad = None
                torch.manual_seed(99 + step)
                oa = whole(xa)
                _loss(oa, target).backward()
                torch.manual_seed(99 + step)
                ob = cut.forward_pruned(xb, head)
                _loss(ob, target).backward()
                assert len(oa) == len(ob) and all(torch.equal(p, q) for p, q in zip(oa, ob)), (name, dt, head)
                for (k, p), (_, q) in zip(whole.named_parameters(), cut.named_parameters()):
                    assert p.grad is not None and q.grad is not None and torch.equal(p.grad, q.grad), (name, dt, k)
                for (k, p), (_, q) in zip(whole.named_buffers(), cut.named_buffers()):
                    assert torch.equal(p, q), (name, dt, k)
                if want_dx:
                    assert torch.equal(xa.grad, xb.grad)
            pa, pb = whole.__dict__["_pack_plan"], cut.__dict__["_pack_plan"]
            assert {e.phase for e in pb.entries.values()} == {e.phase for e in pa.entries.values()} == {"fwd", "bwd"}
            assert len(pa.entries) == len(pb.entries) and pa.launches == pb.launches
            assert pa.copy_launches == pb.copy_launches


# ------------------------------------------------------------------------------------------------ pruning is real
def _outside_tensors(m, head):
    prefixes = _prefixes(m.depth, head)
    return {k: t for k, t in list(m.named_parameters()) + list(m.named_buffers())
            if not k.startswith(prefixes) and t.is_floating_point()}


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("depth,head", [(4, 1), (4, 2), (5, 2), (3, 1)])
def test_pruned_step_never_touches_what_is_outside_the_cut(dev, dt, depth, head):
    from unet_nested4tiny_objects_keypoints_amd import AdamW, train_step
    m, kw = _seeded(dev, dt, seed=8, depth=depth, feature_scale=4)
    outside = _outside_tensors(m, head)
    assert outside
    with torch.no_grad():
        for t in outside.values():
            t.fill_(float("nan"))
    opt = AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
    g = torch.Generator().manual_seed(21)
    x, target = torch.randn(2, 1, 64, 64, generator=g).to(dev), torch.rand(2, 4, 64, 64, generator=g).to(dev)
    inside_before = {k: p.detach().clone() for k, p in m.named_parameters() if k.startswith(_prefixes(depth, head))}
    for _ in range(2):
        outs, loss = train_step(m, opt, _crit(), x, target, head=head)
        assert len(outs) == head and bool(torch.isfinite(loss)) and all(bool(torch.isfinite(o).all()) for o in outs)
    for k, p in m.named_parameters():
        if k in outside:
            assert p.grad is None and p not in opt.state, k
        else:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(torch.isfinite(p).all()), k
            assert p in opt.state
    for k, t in outside.items():
        assert bool(torch.isnan(t).all()), k                      # unchanged: still NaN everywhere
    assert any(not torch.equal(p, inside_before[k]) for k, p in m.named_parameters() if k in inside_before)
    for k, b in m.named_buffers():                                # counters outside the cut did not move either
        if k.endswith("num_batches_tracked") and not k.startswith(_prefixes(depth, head)):
            assert int(b) == 0, k


# ------------------------------------------------------------------------------------------------ determinism, mixing
def _snapshot(m):
    return ({k: p.detach().clone() for k, p in m.named_parameters()},
            {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()},
            {k: b.clone() for k, b in m.named_buffers()})


def _same(a, b):
    for part_a, part_b in zip(a, b):
        for k in part_a:
            if part_a[k] is None or part_b[k] is None:
                assert part_a[k] is None and part_b[k] is None, k
            else:
                assert torch.equal(part_a[k], part_b[k]), k


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_pruned_steps_are_deterministic_and_mix_with_whole_steps(dev, dt):
    """Two pruned steps from equal states give the same bits, and the sequence pruned, whole, pruned on ONE model equals
    the same steps on twins that only ever ran one kind of pass: the weight images and the grouped-weight buffers of a
    cut are its own."""
    from unet_nested4tiny_objects_keypoints_amd import train_step
    base, _ = _seeded(dev, dt, seed=9)
    base.drop_out.eval()
    g = torch.Generator().manual_seed(31)
    batches = [(torch.randn(2, 1, 64, 64, generator=g).to(dev), torch.rand(2, 4, 64, 64, generator=g).to(dev)) for _ in range(6)]
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    oa, ob = torch.optim.SGD(a.parameters(), lr=0.05), torch.optim.SGD(b.parameters(), lr=0.05)
    for (x, t) in batches[:2]:
        la = train_step(a, oa, _crit(), x, t, head=2)[1]
        lb = train_step(b, ob, _crit(), x, t, head=2)[1]
        assert float(la) == float(lb)
        _same(_snapshot(a), _snapshot(b))
    kinds = [1, None, 2, None, 1, 2]
    mixed = copy.deepcopy(base)
    om = torch.optim.SGD(mixed.parameters(), lr=0.05)
    for kind, (x, t) in zip(kinds, batches):
        # the twin starts from the mixed model's current state and has never run any other pass
        twin = copy.deepcopy(base)
        twin.load_state_dict(mixed.state_dict())
        ot = torch.optim.SGD(twin.parameters(), lr=0.05)
        lm = train_step(mixed, om, _crit(), x, t, head=kind)[1]
        lt = train_step(twin, ot, _crit(), x, t, head=kind)[1]
        assert float(lm) == float(lt), kind
        _same(_snapshot(mixed), _snapshot(twin))
    plan = mixed.__dict__["_pack_plan"]
    assert {e.phase for e in plan.entries.values()} == {"fwd", "bwd", "fwd/1", "bwd/1", "fwd/2", "bwd/2"}
    assert set(mixed._grouped_dgrad_w_cut) == {1, 2}
    whole_w, cut_w = mixed._grouped_dgrad_w, mixed._grouped_dgrad_w_cut[2]
    assert set(cut_w) < set(whole_w)
    assert all(cut_w[k].shape[0] < whole_w[k].shape[0] and cut_w[k].data_ptr() != whole_w[k].data_ptr() for k in cut_w)


# ------------------------------------------------------------------------------------------------ ensemble
@pytest.mark.parametrize("name,head", _cuts(), ids=_ids(_cuts()))
def test_ensemble_forward_and_gradients_vs_float64_oracle(dev, name, head):
    z, ctor = load_golden(name)
    d = ctor.get("depth", 4)
    state = sub(z, "state0")
    target = torch.from_numpy(z["target"]).to(dev)
    for loss_kind in ("sum", "focal"):
        m = _model(ctor, state, dev).eval()
        m._debug_keep_saved = True
        x = torch.from_numpy(z["x"]).to(dev).requires_grad_(True)
        got = m.forward_pruned(x, head, ensemble=True)
        assert isinstance(got, torch.Tensor) and got.grad_fn is not None
        assert torch.equal(got, m.infer(x, head, ensemble=True)), (name, head)
        (got.sum() if loss_kind == "sum" else _crit()(got, target)).backward()
        ro, want, want_dx, gated, _ = _oracle_step(ctor, state, x.detach().cpu(), target.cpu(), head, m._debug_saved,
                                                   ensemble=True, loss=loss_kind, train=False)
        check_flips(gated, "pruned-ensemble:%s:head%d:%s" % (name, head, loss_kind))
        assert rel_err(got.detach().cpu(), ro[0]) < TOL
        prefixes = _prefixes(d, head)
        grads = {}
        for k, p in m.named_parameters():
            if k.startswith(prefixes):
                assert p.grad is not None, k
                grads[k] = p.grad.cpu()
            else:
                assert p.grad is None, k
        assert sorted(grads) == sorted(want)
        # eval mode: BatchNorm runs on its running statistics, so a convolution bias in front of it has a real gradient
        assert_grads_close(grads, want, dict(ctor, is_batchnorm=False), TOL)
        err = rel_err(x.grad.cpu(), want_dx)
        print("pruned-ensemble %s head %d %s: input gradient rel_err %.3e" % (name, head, loss_kind, err))
        assert err < TOL


def test_ensemble_refuses_active_dropout_and_trains_without_it(dev):
    m, _ = _seeded(dev, seed=10)
    x = torch.randn(2, 1, 64, 64, device=dev)
    with pytest.raises(RuntimeError, match=r"model\.drop_out\.eval\(\)"):
        m.forward_pruned(x, 2, ensemble=True)
    m.drop_out.eval()                                              # training mode, batch statistics, no dropout
    out = m.forward_pruned(x, 2, ensemble=True)
    out.sum().backward()
    assert all((p.grad is not None) == k.startswith(_prefixes(4, 2)) for k, p in m.named_parameters())
    m.drop_out.train()
    m.drop_out.p = 0.0                                             # p = 0 is no dropout either
    assert torch.isfinite(m.forward_pruned(x, 1, ensemble=True)).all()


# ------------------------------------------------------------------------------------------------ fine-tune loop
def test_fine_tune_loop_of_a_pruned_checkpoint(dev, tmp_path):
    from unet_nested4tiny_objects_keypoints_amd import AdamW, UNet_Nested, pruned_parameters, train_step
    from unet_nested4tiny_objects_keypoints_amd.checkpoint import load_pruned, save_pruned
    src, kw = _seeded(dev, seed=11)
    head = 2
    path = save_pruned(src, head, str(tmp_path / "head2.pth"))
    torch.manual_seed(5)
    m = UNet_Nested(**kw).to(dev).train()
    assert load_pruned(m, path) == head and m.pruned_to == head
    params = pruned_parameters(m, head)
    opt = AdamW(params, lr=1e-3)
    g = torch.Generator().manual_seed(41)
    x, target = torch.randn(2, 1, 64, 64, generator=g).to(dev), torch.rand(2, 4, 64, 64, generator=g).to(dev)
    losses = []
    for _ in range(3):
        outs, loss = train_step(m, opt, _crit(), x, target, head=head)
        losses.append(float(loss))
    assert len(outs) == head and all(v == v and abs(v) != float("inf") for v in losses)
    with pytest.raises(RuntimeError, match="pruned to head 2"):
        train_step(m, opt, _crit(), x, target)                    # forward() of a pruned model keeps refusing
    with pytest.raises(RuntimeError, match="pruned to head 2"):
        train_step(m, opt, _crit(), x, target, head=3)
    m.eval()
    again = save_pruned(m, head, str(tmp_path / "tuned.pth"))
    torch.manual_seed(6)
    served = UNet_Nested(**kw).to(dev).eval()
    assert load_pruned(served, again) == head
    for j in (1, 2):
        for e in (False, True):
            assert torch.equal(served.infer(x, j, ensemble=e), m.infer(x, j, ensemble=e)), (j, e)
    assert not torch.equal(m.infer(x, 2), src.eval().infer(x, 2))  # it did train


# ------------------------------------------------------------------------------------------------ graph
@pytest.mark.parametrize("dt,head", [("fp32", 1), ("fp32", 2), ("bf16", 2)])
def test_graphed_pruned_step_replays_the_eager_step(dev, dt, head):
    from unet_nested4tiny_objects_keypoints_amd import GraphedTrainStep, train_step
    a, _ = _seeded(dev, dt, seed=12)
    a.drop_out.p = 0.0                                             # dropout off: the two paths draw different seeds by design
    b = copy.deepcopy(a)
    before = {k: v.clone() for k, v in a.state_dict().items()}
    oa, ob = torch.optim.SGD(a.parameters(), lr=2e-3, momentum=0.9), torch.optim.SGD(b.parameters(), lr=2e-3, momentum=0.9)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(2, 1, 64, 64, generator=g).to(dev) for _ in range(3)]
    ts = [torch.rand(2, 4, 64, 64, generator=g).to(dev) for _ in range(3)]
    step = GraphedTrainStep(a, oa, _crit(), xs[0], ts[0], capture_optimizer=True, check_topology=True, head=head)
    assert step.topology["chain"] and set(step.topology["kinds"]) == {"kernel"}, step.topology
    for k, v in a.state_dict().items():
        assert torch.equal(v, before[k]), k
    inside = _prefixes(4, head)
    for x, t in zip(xs, ts):
        outs_g, loss_g = step(x, t)
        outs_e, loss_e = train_step(b, ob, _crit(), x, t, head=head)
        assert float(loss_g) == float(loss_e)
        assert len(outs_g) == len(outs_e) == head and all(torch.equal(p, q) for p, q in zip(outs_g, outs_e))
        for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            assert torch.equal(p, q), k
            if k.startswith(inside):
                assert p.grad is not None and torch.equal(p.grad, q.grad), k
            else:
                assert p.grad is None and q.grad is None and torch.equal(p, before[k]), k
        for (k, p), (_, q) in zip(a.named_buffers(), b.named_buffers()):
            assert torch.equal(p, q), k


# ------------------------------------------------------------------------------------------------ data parallel
DP_CTOR = dict(in_channels=1, n_classes=4, feature_scale=8)
DP_HEAD = 2


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, state, out_dir):
    import os

    import torch.distributed as dist

    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet_Nested, dp, pruned_parameters, train_step
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        dev = torch.device("cuda:0")
        torch.manual_seed(50 + rank)              # ranks start from different weights: the broadcast must fix it
        m = UNet_Nested(**DP_CTOR)
        if rank == 0:
            m.load_state_dict(state)
        m = m.to(dev).train()
        m.drop_out.eval()
        avg = dp.make_data_parallel(m, bucket_bytes=4 << 10, head=DP_HEAD)
        g = torch.Generator().manual_seed(200 + rank)
        x = torch.randn(2, 1, 32, 32, generator=g).to(dev)
        t = torch.rand(2, 4, 32, 32, generator=g).to(dev)
        opt = torch.optim.SGD(m.parameters(), lr=0.05)
        train_step(m, opt, FocalLoss_BCE_2d(gamma=3, size_average=False), x, t, head=DP_HEAD)
        torch.cuda.synchronize()
        refused = False
        try:
            m(x)[0].sum().backward()              # the whole network's gradients do not fit a cut's averager
        except RuntimeError as e:
            refused = "cut at head %d" % DP_HEAD in str(e)
        torch.save({"params": {k: p.detach().cpu() for k, p in m.named_parameters()},
                    "grads": {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in m.named_parameters()},
                    "buckets": len(avg.buckets_last_step), "flat": avg.flat.numel(), "refused": refused,
                    "cut": sum(p.numel() for p in pruned_parameters(m, DP_HEAD))}, os.path.join(out_dir, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_rank_pruned_step_delivers_the_mean_gradient(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import torch.multiprocessing as mp

    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(7)
    state = {k: v.clone() for k, v in UNet_Nested(**DP_CTOR).state_dict().items()}
    mp.spawn(_dp_worker, args=(2, _free_port(), state, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert r0["flat"] == r0["cut"] and r0["buckets"] >= 2          # the flat buffer holds the cut's gradients only
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), k    # replicas stay bit-identical
    # expected: the mean of the two ranks' gradients, each from the same HIP path run single-process (exact up to the order
    # of one addition)
    grads = []
    for rank in range(2):
        m = UNet_Nested(**DP_CTOR)
        m.load_state_dict(state)
        m = m.cuda().train()
        m.drop_out.eval()
        g = torch.Generator().manual_seed(200 + rank)
        x = torch.randn(2, 1, 32, 32, generator=g).cuda()
        t = torch.rand(2, 4, 32, 32, generator=g).cuda()
        _loss(m.forward_pruned(x, DP_HEAD), t).backward()
        grads.append({k: (None if p.grad is None else p.grad.cpu()) for k, p in m.named_parameters()})
    prefixes = _prefixes(4, DP_HEAD)
    for k, p0 in state.items():
        if k not in grads[0]:
            continue
        if not k.startswith(prefixes):
            assert r0["grads"][k] is None and grads[0][k] is None, k
            assert torch.equal(r0["params"][k], p0), k
            continue
        mean = (grads[0][k] + grads[1][k]) / 2
        scale = float(mean.abs().max()) + 1e-12
        for r in (r0, r1):
            assert float((r["grads"][k] - mean).abs().max()) <= 1e-5 * scale + 1e-12, k
        want = p0 - 0.05 * mean
        assert float((r0["params"][k] - want).abs().max()) < 1e-5 * 0.05 * scale + 2.5e-7, k
    assert r0["refused"] and r1["refused"]
