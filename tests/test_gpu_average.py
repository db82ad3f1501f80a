"""Weight averaging on the device (averaging.py, csrc/average.hip), GPU only:
  (1) the kernel against float64 over segment sizes around the vector width and the chunk size, misaligned streams, copy
      segments and guard words, at the full grid and at a grid smaller than the chunk count;
  (2) the bit-exact facts (first update, vector == scalar path, swap);  (3) a captured update against the eager one;
  (4) WeightAverager on UNet_Nested and UNet through train_step;  (5) update_bn against torch's update_bn on the CPU
      oracle;  (6) checkpoints.

The element-wise bound of (1) and (4) is derived, not measured: one update d = s - a; a = a + w*d has three roundings of
values <= 2M plus the rounding of w, in all < 7 * 2^-24 * M < 2^-21 * M, and earlier error carries with factor
(1 - w) <= 1 -- so K updates stay within K * 2^-21 * M, M = max(|src|, |avg|) over the run."""

import pytest
import torch

from tests.helpers import load_golden, rel_err, seeded_state, usable_cus

pytestmark = pytest.mark.gpu

K = 5
GUARD = 4                     # guard words after (and so between) segments
GUARD_BITS = 0x7FC0BEEF       # a NaN payload no arithmetic here produces
SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8193]
BIG = 74 * 4096 + 3           # more chunks than an 8-CU grid has workgroups (8 * 8): the persistent loop takes a second lap


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _last_kernel():
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return _lib.lib().unetpp_last_kernel_name().decode()


class _Layout:
    """Segments inside two guarded buffers.  spec rows: (numel, src offset in floats past a 16-byte boundary, avg offset,
    copy flag)."""

    def __init__(self, spec, dev):
        self.spec, self.dev = spec, dev
        self.src_at, self.avg_at = [], []
        s = a = GUARD
        for n, so, ao, _ in spec:
            s, a = (s + 3) // 4 * 4 + so, (a + 3) // 4 * 4 + ao
            self.src_at.append(s)
            self.avg_at.append(a)
            s, a = s + n + GUARD, a + n + GUARD
        self.src = torch.empty(s + 4, dtype=torch.float32, device=dev)
        self.avg = torch.empty(a + 4, dtype=torch.float32, device=dev)
        self.src.view(torch.int32).fill_(GUARD_BITS)
        self.avg.view(torch.int32).fill_(GUARD_BITS)
        self.src_mask = torch.zeros(self.src.numel(), dtype=torch.bool, device=dev)   # True inside a segment
        self.avg_mask = torch.zeros(self.avg.numel(), dtype=torch.bool, device=dev)
        for (n, _, _, _), s0, a0 in zip(spec, self.src_at, self.avg_at):
            self.src_mask[s0:s0 + n] = True
            self.avg_mask[a0:a0 + n] = True
        assert self.src.data_ptr() % 16 == 0 and self.avg.data_ptr() % 16 == 0

    def srcs(self):
        return [self.src[s0:s0 + n] for (n, _, _, _), s0 in zip(self.spec, self.src_at)]

    def avgs(self):
        return [self.avg[a0:a0 + n] for (n, _, _, _), a0 in zip(self.spec, self.avg_at)]

    def table(self):
        from unet_nested4tiny_objects_keypoints_amd.averaging import SegmentTable
        return SegmentTable([(a, s, c) for a, s, (_, _, _, c) in zip(self.avgs(), self.srcs(), self.spec)])

    def set_sources(self, values):
        for s, v in zip(self.srcs(), values):
            s.copy_(v)

    def guards_intact(self):
        ok_s = bool((self.src.view(torch.int32)[~self.src_mask] == GUARD_BITS).all())
        ok_a = bool((self.avg.view(torch.int32)[~self.avg_mask] == GUARD_BITS).all())
        return ok_s and ok_a


def _spec(misalign_all=False):
    rows = [(n, 0, 0, 0) for n in SIZES]
    rows += [(4097, 1, 0, 0), (4097, 0, 1, 0), (8193, 3, 2, 0)]     # a stream off the 16-byte grid: the scalar path
    rows += [(5, 0, 0, 1), (4097, 0, 0, 1), (4097, 1, 0, 1)]        # carried, not averaged
    rows += [(BIG, 0, 0, 0)]
    if misalign_all:
        rows = [(n, 1, 1, c) for n, _, _, c in rows]
    return rows


def _sources(spec, seed):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(n, generator=g) for n, _, _, _ in spec] for _ in range(K)]


def _run_updates(lay, kind, decay, snaps):
    """K updates through the kernel -> (final averages on the CPU, element-wise M over the run per segment)."""
    from unet_nested4tiny_objects_keypoints_amd import _lib
    table = lay.table()
    M = [torch.zeros(n, dtype=torch.float64) for n, _, _, _ in lay.spec]
    for k in range(K):
        lay.set_sources([v.to(lay.dev) for v in snaps[k]])
        table.launch(kind, count=k, decay=decay)
        assert _last_kernel() == ("avg_mean" if kind == _lib.AVG_MEAN else "avg_ema")
        for i, a in enumerate(lay.avgs()):
            M[i] = torch.maximum(M[i], torch.maximum(a.double().cpu().abs(), snaps[k][i].double().abs()))
    torch.cuda.synchronize()
    return [a.cpu() for a in lay.avgs()], M


@pytest.mark.parametrize("cus", [None, 8], ids=["all-cus", "8-cus"])
@pytest.mark.parametrize("kind,decay", [("mean", 0.0), ("ema", 0.5), ("ema", 0.9)], ids=["mean", "ema0.5", "ema0.9"])
def test_kernel_against_float64(dev, kind, decay, cus):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    spec = _spec()
    snaps = _sources(spec, 11)
    lay = _Layout(spec, dev)
    with usable_cus(cus):
        got, M = _run_updates(lay, _lib.AVG_MEAN if kind == "mean" else _lib.AVG_EMA, decay, snaps)
    assert lay.guards_intact()
    worst = 0.0
    for i, (n, _, _, copy) in enumerate(spec):
        if copy:
            assert torch.equal(got[i].view(torch.int32), snaps[K - 1][i].view(torch.int32)), (i, n)
            continue
        if kind == "mean":
            want = torch.stack([s[i].double() for s in snaps]).mean(0)
        else:
            want = snaps[0][i].double()
            for k in range(1, K):
                want = want + (1.0 - decay) * (snaps[k][i].double() - want)
        err = (got[i].double() - want).abs()
        bound = K * 2.0 ** -21 * M[i]
        assert bool(torch.isfinite(got[i]).all()), (i, n)
        ratio = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), (i, n, ratio)
        # the average moved: a kernel that does nothing, or only copies, is nowhere near
        assert float((got[i].double() - snaps[K - 1][i].double()).abs().max()) > 0 or n < 4
    print("avg %s decay %s: worst err / bound %.3f" % (kind, decay, worst))


def test_first_update_copies_bit_for_bit(dev):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    spec = _spec()
    lay = _Layout(spec, dev)
    snaps = _sources(spec, 3)
    # sources with every kind of bit pattern: a plain float copy must keep them all
    weird = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-45, -1e-45, 3.4e38], dtype=torch.float32)
    for kind in (_lib.AVG_MEAN, _lib.AVG_EMA):
        lay.avg.view(torch.int32)[lay.avg_mask] = 0x3F800000
        vals = [v.clone() for v in snaps[0]]
        for v in vals:
            v[:min(v.numel(), weird.numel())] = weird[:v.numel()]
        lay.set_sources([v.to(dev) for v in vals])
        lay.table().launch(kind, count=0, decay=0.5)
        torch.cuda.synchronize()
        for a, v in zip(lay.avgs(), vals):
            assert torch.equal(a.cpu().view(torch.int32), v.view(torch.int32))
        assert lay.guards_intact()


@pytest.mark.parametrize("kind,decay", [("mean", 0.0), ("ema", 0.9)])
def test_vector_and_scalar_paths_give_the_same_bits(dev, kind, decay):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    k = _lib.AVG_MEAN if kind == "mean" else _lib.AVG_EMA
    snaps = _sources(_spec(), 5)
    vec, _ = _run_updates(_Layout(_spec(False), dev), k, decay, snaps)
    sca, _ = _run_updates(_Layout(_spec(True), dev), k, decay, snaps)
    for a, b in zip(vec, sca):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_swap_exchanges_and_two_swaps_restore(dev):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    spec = _spec()
    lay = _Layout(spec, dev)
    g = torch.Generator().manual_seed(9)
    s0 = [torch.randn(n, generator=g) for n, _, _, _ in spec]
    a0 = [torch.randn(n, generator=g) for n, _, _, _ in spec]
    lay.set_sources([v.to(dev) for v in s0])
    for a, v in zip(lay.avgs(), a0):
        a.copy_(v)
    table = lay.table()
    with usable_cus(8):
        table.launch(_lib.AVG_SWAP)
    assert _last_kernel() == "avg_swap"
    torch.cuda.synchronize()
    for a, s, av, sv in zip(lay.avgs(), lay.srcs(), a0, s0):      # copy segments are exchanged like the others
        assert torch.equal(a.cpu(), sv) and torch.equal(s.cpu(), av)
    assert lay.guards_intact()
    table.launch(_lib.AVG_SWAP)
    torch.cuda.synchronize()
    for a, s, av, sv in zip(lay.avgs(), lay.srcs(), a0, s0):
        assert torch.equal(a.cpu().view(torch.int32), av.view(torch.int32))
        assert torch.equal(s.cpu().view(torch.int32), sv.view(torch.int32))
    assert lay.guards_intact()


def test_overlapping_streams_are_refused(dev):
    from unet_nested4tiny_objects_keypoints_amd.averaging import SegmentTable
    t = torch.zeros(64, device=dev)
    with pytest.raises(ValueError, match="overlaps"):
        SegmentTable([(t[:32], t[16:48], 0)])
    with pytest.raises(ValueError):
        SegmentTable([(t[:32], t[32:48], 0)])


class _Params(torch.nn.Module):
    def __init__(self, sizes, dev, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=g).to(dev)) for n in sizes])


@pytest.mark.parametrize("kind", ["mean", "ema"])
def test_captured_update_equals_eager(dev, kind):
    """One eager update, then update() captured alone (a plain chain of one kernel) and replayed three times with the
    sources changed in place between replays."""
    from unet_nested4tiny_objects_keypoints_amd import WeightAverager
    mod = _Params([5, 4097, 8193, BIG], dev, 2)
    cap = WeightAverager(mod, kind=kind, decay=0.9, capturable=True)
    eag = WeightAverager(mod, kind=kind, decay=0.9)
    cap.update()
    eag.update()
    assert _last_kernel() == "avg_" + kind
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap.update()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert float(cap.n_averaged) == 1.0          # capturing launches nothing
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        with torch.no_grad():
            for p in mod.ps:
                p.copy_(torch.randn(p.shape, generator=g).to(dev))
        graph.replay()
        eag.update()
    torch.cuda.synchronize()
    n = cap.n_averaged
    assert torch.is_tensor(n) and n.is_cuda and n.dtype == torch.float32 and float(n) == 4.0
    assert eag.n_averaged == 4 and isinstance(eag.n_averaged, int)
    a, b = cap.averaged_state_dict(), eag.averaged_state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
        assert not torch.equal(a[k], mod.state_dict()[k]) or a[k].numel() < 2   # it is an average, not the last copy


def test_capture_needs_one_eager_update(dev, monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import WeightAverager
    cap = WeightAverager(_Params([5], dev, 1), capturable=True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)   # (no real capture is left half open)
    with pytest.raises(RuntimeError, match="run one eager update\\(\\) before capturing it"):
        cap.update()


class _WithBuffers(torch.nn.Module):
    def __init__(self, dev):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(37, device=dev))
        self.register_buffer("stat", torch.zeros(9, device=dev))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long, device=dev))
        self.register_buffer("scratch", torch.zeros(3, device=dev), persistent=False)    # not in the state_dict


@pytest.mark.parametrize("average_buffers", [False, True])
def test_buffers_are_carried_or_averaged(dev, average_buffers):
    from unet_nested4tiny_objects_keypoints_amd import WeightAverager
    mod = _WithBuffers(dev)
    wrapped = torch.nn.DataParallel(mod, device_ids=[0])
    avg = WeightAverager(wrapped, average_buffers=average_buffers)
    assert avg.model is mod                                   # the wrapper is unwrapped, as checkpoint._unwrap does
    for k in (1.0, 2.0, 6.0):
        with torch.no_grad():
            mod.w.fill_(k)
            mod.stat.fill_(k)
            mod.count.fill_(int(k))
        avg.update()
    sd = avg.averaged_state_dict()
    assert list(sd) == ["w", "stat", "count"]
    assert torch.equal(sd["w"], torch.full((37,), 3.0, device=dev))
    assert torch.equal(sd["stat"], torch.full((9,), 3.0 if average_buffers else 6.0, device=dev))
    assert sd["count"].dtype == torch.long and int(sd["count"]) == 6
    with avg.applied():
        assert int(mod.count) == 6 and float(mod.w.detach()[0]) == 3.0
        mod.count.fill_(11)                                   # what the block writes stays with the averager
    assert int(mod.count) == 6 and float(mod.w.detach()[0]) == 6.0 and int(avg.averaged_state_dict()["count"]) == 11


# ---------------------------------------------------------------------------------------------------------------------
def _bits_equal(a, b):
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def _model_level(model, make_peer, x, t, dev):
    from unet_nested4tiny_objects_keypoints_amd import AdamW, FocalLoss_BCE_2d, WeightAverager, train_step
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    opt = AdamW(model.parameters(), lr=1e-2, weight_decay=1e-4)
    avg = WeightAverager(model)
    versions = [p._version for p in model.parameters()]
    snaps = []
    for _ in range(4):
        train_step(model, opt, crit, x, t)
        avg.update()
        snaps.append({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    assert avg.n_averaged == 4
    assert [p._version for p in model.parameters()] == versions
    asd = avg.averaged_state_dict()
    assert list(asd) == list(model.state_dict())
    params = {k for k, _ in model.named_parameters()}
    moved = 0
    for k, got in asd.items():
        assert got.shape == snaps[0][k].shape and got.dtype == snaps[0][k].dtype and got.device.type == "cuda", k
        if k not in params:            # buffers are carried: the last snapshot, bit for bit
            assert _bits_equal(got.cpu(), snaps[-1][k]), k
            continue
        want = torch.stack([s[k].double() for s in snaps]).mean(0)
        M = max(float(torch.stack([s[k] for s in snaps]).abs().max()), float(got.abs().max()))
        err = float((got.double().cpu() - want).abs().max())
        assert err <= 4 * 2.0 ** -21 * M, (k, err, M)
        moved += int(not torch.equal(got.cpu(), snaps[-1][k]))
    assert moved > len(params) // 2       # the parameters trained, so their mean is not their last value

    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    peer = make_peer().to(dev)
    peer.load_state_dict(asd, strict=True)
    peer.eval()
    with torch.no_grad():
        want_out = peer(x)
    with avg.applied() as inner:
        assert inner is model
        for k, v in model.state_dict().items():
            assert _bits_equal(v, asd[k]), k
        model.eval()
        with torch.no_grad():
            got_out = model(x)
        model.train()
        with pytest.raises(RuntimeError, match="nest"):
            with avg.applied():
                pass
        with pytest.raises(RuntimeError, match="inside applied"):
            avg.update()
    got_out = got_out if isinstance(got_out, tuple) else (got_out,)
    want_out = want_out if isinstance(want_out, tuple) else (want_out,)
    assert len(got_out) == len(want_out) and all(torch.equal(a, b) for a, b in zip(got_out, want_out))
    for k, v in model.state_dict().items():
        assert _bits_equal(v, before[k]), k
    for k, v in avg.averaged_state_dict().items():     # and the average is what it was
        assert _bits_equal(v, asd[k]), k
    _, loss = train_step(model, opt, crit, x, t)
    assert bool(torch.isfinite(loss))
    avg.update()
    assert avg.n_averaged == 5
    return avg


def test_unet_nested_average_of_four_steps(dev):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(31)
    ctor = dict(in_channels=1, n_classes=4, feature_scale=8)
    model = UNet_Nested(**ctor).to(dev).train()
    x, t = torch.randn(2, 1, 32, 32, device=dev), torch.rand(2, 4, 32, 32, device=dev)
    _model_level(model, lambda: UNet_Nested(**ctor), x, t, dev)


def test_plain_unet_average_of_four_steps(dev):
    from unet_nested4tiny_objects_keypoints_amd import UNet
    z, ctor = load_golden("unet_w8_rgb5_32x48_b2")
    torch.manual_seed(32)
    model = UNet(**ctor).to(dev).train()
    x, t = torch.from_numpy(z["x"]).to(dev), torch.from_numpy(z["target"]).to(dev)
    avg = _model_level(model, lambda: UNet(**ctor), x, t, dev)
    # a plain U-Net has BatchNorm everywhere: update_bn is a whole training-mode forward, with torch's semantics
    from oracle.unet_plain_oracle import UNetOracle
    batches = [x.cpu(), torch.randn(x.shape, generator=torch.Generator().manual_seed(1))]
    own = {k: v.detach().clone() for k, v in model.state_dict().items()}
    avg.update_bn([b.to(dev) for b in batches])
    ref = UNetOracle(**ctor)
    ref.load_state_dict({k: v.cpu() for k, v in avg.averaged_state_dict().items()}, strict=True)
    torch.optim.swa_utils.update_bn(batches, ref)
    got = avg.averaged_state_dict()
    for k, v in ref.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            assert rel_err(got[k].cpu(), v) <= 1e-4, k
        elif k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(v) == 2, k
    for k, v in model.state_dict().items():
        assert _bits_equal(v, own[k]), k
    assert model.training and all(m.training for m in model.modules())


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(dev):
    """A small UNet_Nested two steps into training with an averager that has seen both: (ctor, model, averager, optimizer)."""
    from oracle.unet_nested_oracle import UNetNestedOracle
    from unet_nested4tiny_objects_keypoints_amd import AdamW, FocalLoss_BCE_2d, UNet_Nested, WeightAverager, train_step
    torch.manual_seed(41)
    ctor = dict(in_channels=1, n_classes=4, feature_scale=8)
    model = UNet_Nested(**ctor)
    model.load_state_dict(seeded_state(UNetNestedOracle(**ctor), 7))
    model = model.to(dev).train()
    opt = AdamW(model.parameters(), lr=1e-2, weight_decay=1e-4)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    avg = WeightAverager(model)
    x, t = torch.randn(2, 1, 32, 32, device=dev), torch.rand(2, 4, 32, 32, device=dev)
    for _ in range(2):
        train_step(model, opt, crit, x, t)
        avg.update()
    return ctor, model, avg, opt


def test_update_bn_against_torch_on_the_oracle(dev, trained, monkeypatch):
    from oracle.unet_nested_oracle import UNetNestedOracle
    from unet_nested4tiny_objects_keypoints_amd import engine, ops
    from unet_nested4tiny_objects_keypoints_amd.unet import BatchNormParams
    ctor, model, avg, _ = trained
    g = torch.Generator().manual_seed(17)
    batches = [torch.randn(2, 1, 32, 32, generator=g) for _ in range(3)]
    layers = [m for m in model.modules() if isinstance(m, BatchNormParams)]
    assert len(layers) == 8
    layers[3].momentum = 0.25                      # per-layer settings must come back as they were
    torch.nn.Module.train(layers[5], False)
    own = {k: v.detach().clone() for k, v in model.state_dict().items()}
    flags = [(m.training, getattr(m, "momentum", None)) for m in model.modules()]
    weights = avg.averaged_state_dict()

    def no_heads(*a, **kw):
        raise AssertionError("the statistics pass ran a head")

    monkeypatch.setattr(ops, "head_fwd", no_heads)
    monkeypatch.setattr(ops, "heads_mean_fwd", no_heads)
    monkeypatch.setattr(engine, "_up_fwd", no_heads)          # ... or a decoder node
    monkeypatch.setattr(engine, "_dropout_config", no_heads)  # ... or drew a dropout seed
    timer = ops.LaunchTimer()
    ops.set_timer(timer)
    try:
        avg.update_bn([b.to(dev) for b in batches])
        after = [(m.training, getattr(m, "momentum", None)) for m in model.modules()]
    finally:
        ops.set_timer(None)
        layers[3].momentum = 0.1
        torch.nn.Module.train(layers[5], True)
    torch.cuda.synchronize()
    assert [r[0] for r in timer.regions] == ["X%d0.stats" % i for i in range(4)] * 3
    assert len(timer.launches) == 3 * 2 * 4        # two convolutions per encoder node and nothing else from the GEMMs
    assert _last_kernel() == "avg_swap"            # the swap back out of applied()

    assert after == flags and (False, 0.1) in flags and (True, 0.25) in flags
    for k, v in model.state_dict().items():        # the model's own statistics (and everything else) are untouched
        assert _bits_equal(v, own[k]), k

    ref = UNetNestedOracle(**ctor)
    ref.load_state_dict({k: v.cpu() for k, v in weights.items()}, strict=True)
    torch.optim.swa_utils.update_bn(batches, ref)
    got = avg.averaged_state_dict()
    seen = 0
    for k, v in ref.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            assert rel_err(got[k].cpu(), v) <= 1e-4, (k, rel_err(got[k].cpu(), v))
            assert not torch.equal(got[k], own[k])
            seen += 1
        elif k.endswith("num_batches_tracked"):
            assert int(got[k]) == 3 and int(v) == 3, k
        else:
            assert _bits_equal(got[k].cpu(), weights[k].cpu()), k
    assert seen == 16


def test_update_bn_without_batchnorm_runs_nothing(dev, monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, WeightAverager, engine
    model = UNet_Nested(in_channels=1, n_classes=4, feature_scale=8, is_batchnorm=False).to(dev)
    avg = WeightAverager(model)
    avg.update()

    def never(*a, **kw):
        raise AssertionError("update_bn ran a pass on a model without BatchNorm")

    monkeypatch.setattr(engine, "stats_pass", never)
    monkeypatch.setattr(engine, "forward_impl", never)
    monkeypatch.setattr(avg, "_swap", never)
    avg.update_bn([torch.randn(2, 1, 32, 32, device=dev)])
    # and the engine piece itself returns before its first launch
    monkeypatch.undo()
    monkeypatch.setattr(engine, "_pair_fwd", never)
    engine.stats_pass(model, torch.randn(2, 1, 32, 32, device=dev))


def test_checkpoints(dev, trained, tmp_path):
    from oracle.unet_nested_oracle import UNetNestedOracle
    from unet_nested4tiny_objects_keypoints_amd import AdamW, UNet_Nested, WeightAverager, checkpoint
    ctor, model, avg, opt = trained
    want = avg.averaged_state_dict()
    path = checkpoint.save_average(avg, str(tmp_path), 3, 0.25, 1.5)
    assert path.endswith("average_epoch_3_heatmaploss_0.25_landmarkloss_1.5.pth")
    fresh = UNet_Nested(**ctor)
    assert checkpoint.resume(fresh, path) == 0                       # a plain .pth, loaded strictly
    ref = UNetNestedOracle(**ctor)
    ref.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
    for k, v in want.items():
        assert _bits_equal(fresh.state_dict()[k], v.cpu()) and _bits_equal(ref.state_dict()[k], v.cpu()), k

    tar = checkpoint.save_checkpoint(model, opt, 3, str(tmp_path / "with.tar"), averager=avg)
    assert list(torch.load(tar, map_location="cpu")) == ["model_state_dict", "optimizer_state_dict", "epoch",
                                                         "average_state_dict"]
    for capturable in (False, True):
        m2 = UNet_Nested(**ctor).to(dev)
        opt2 = AdamW(m2.parameters(), lr=1e-2, weight_decay=1e-4)
        avg2 = WeightAverager(m2, capturable=capturable)
        assert checkpoint.resume(m2, tar, optimizer=opt2, resume_opt=True, averager=avg2) == 4
        assert int(avg2.n_averaged) == avg.n_averaged == int(avg.state_dict()["n_averaged"])
        for k, v in avg2.averaged_state_dict().items():
            assert _bits_equal(v, want[k]), k
        for k, v in m2.state_dict().items():
            assert _bits_equal(v, model.state_dict()[k]), k
        cont = WeightAverager(model)                                 # the resumed averager continues as the saved one would
        cont.load_state_dict(avg.state_dict())
        cont.update()
        avg2.update()
        assert int(avg2.n_averaged) == cont.n_averaged == avg.n_averaged + 1
        for k, v in avg2.averaged_state_dict().items():
            assert _bits_equal(v, cont.averaged_state_dict()[k]), k

    plain = checkpoint.save_checkpoint(model, opt, 3, str(tmp_path / "without.tar"))
    assert list(torch.load(plain, map_location="cpu")) == ["model_state_dict", "optimizer_state_dict", "epoch"]
    with pytest.raises(KeyError, match="average_state_dict"):
        checkpoint.resume(UNet_Nested(**ctor).to(dev), plain, optimizer=AdamW(model.parameters()), resume_opt=True,
                          averager=avg)
    ema = WeightAverager(model, kind="ema")
    with pytest.raises(ValueError, match="kind"):
        ema.load_state_dict(avg.state_dict())
