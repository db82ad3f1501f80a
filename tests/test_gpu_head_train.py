"""unetpp_head_train -- one head of a training step in one pass (forward, gradient of the mean focal loss, backward) --
against the three launches it replaces, bit for bit, and against float64.

(a) Kernel: ops.head_train on the operands of the composition
        unetpp_head_fwd -> unetpp_focal_bce_heads (gradients of the mean over the heads) -> unetpp_head_bwd + unetpp_sum_partials
    must give the same bits in the map, dx, every partial row, dW and db.  C in {16, 32, 64} x n_cls in {3, 4, 5} (padded
    classes 4 and 8; and 128 channels, whose pieces of x do not stay in registers); per pair every dropout mode (none,
    counter hash with a seed_dev offset, mask tensor) on every shape:
    1x8x8 (one tile), 2x8x24 (several tiles across an image edge), 1x5x7 (a partial tile) and the smallest shape with more
    64-pixel tiles than unetpp_head_bwd_blocks returns (a workgroup walks a second tile); gate_x and 1..3 heads (the
    1/heads scaling) alternate over those runs so that each value meets each dropout mode.  Targets hold exact hits
    (gradient exactly 0), zeros and ones.  What the streaming forward does not take (C = 16 with 5 classes: 8 padded
    classes on 4 lanes) must be refused before anything is written; the caller's fallback is (b)'s business.
    Beside the bits: the float64 restatement under the bounds of tests/test_gpu_heads.py (its helpers, unchanged), with
    dl taken from the kernel's own map and the composition's d_out, as there.
(b) Whole step: a tiny network (feature_scale 4, 32x32, batch 2; whole and cut at head 1 and 2), two train_steps on the new
    path and under UNETPP_NO_FUSED_HEAD_TRAIN=1: outputs, loss, every p.grad and the BatchNorm buffers bit for bit.  At
    feature_scale 4 level 0 has 8 channels, which the library refuses (the forward there is the tiled kernel), so that
    network checks the fallback; the same at feature_scale 2 (16 channels) runs the new kernel for every head.  A
    criterion subclass with its own forward takes the old path, and so do ignore_negative and a class count the library
    refuses.  A GraphedTrainStep replay (seed through seed_dev) equals the eager step."""
import ctypes
import importlib

import pytest
import torch

from oracle.dropout_oracle import keep_mask
from tests.helpers import bound_ratio, gamma, rel_err
from tests.test_gpu_heads import (MASK64, P_DROP, TOL, head_seed, keep_scale, out_bound, ref_backward, ref_forward, run_bwd,
                                  run_fwd)

pytestmark = pytest.mark.gpu

WORD = 0x0123456789ABCDEF    # the device word of the D = 1 runs: seed = by-value part + word


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _blocks(pixels):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    return int(_lib.lib().unetpp_head_bwd_blocks(pixels))


def _shapes():
    """1x8x8, 2x8x24, 1x5x7 and the smallest N x H x W (one image, 64-pixel rows) with more tiles than workgroups."""
    cap = _blocks(1 << 40)                      # the count stops growing: every workgroup has a tile
    assert _blocks(64 * cap) == cap and _blocks(64 * cap + 1) == cap
    return [(1, 8, 8), (2, 8, 24), (1, 5, 7), (1, cap + 1, 64)]


def _bwd_rows(d_out, out, x, wt, p, seed, mask, gate, seed_dev):
    """unetpp_head_bwd (accumulate = 0) with the partial rows kept: -> (dx, rows [blocks, n_cls*C + n_cls])"""
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    n, h, w, c = x.shape
    k = wt.shape[0]
    rows = torch.full((_blocks(n * h * w), k * c + k), float("nan"), device=x.device)
    dx = torch.full_like(x, float("nan"))
    _lib.check(_lib.lib().unetpp_head_bwd(ops._ptr(d_out), ops._ptr(out), ops._ptr(x), ops._ptr(wt), n, h, w, c, k, float(p),
                                          ctypes.c_uint64(seed), ops._ptr(mask), ops._ptr(seed_dev), ops._ptr(dx), 0, int(gate),
                                          ops._ptr(rows), ops._stream()), "unetpp_head_bwd")
    return dx, rows


def _target(out, g):
    """random targets in [0, 1] with exact hits (target == the map: gradient exactly 0), zeros and ones"""
    t = torch.rand(out.shape, generator=g, device=out.device)
    pick = torch.rand(out.shape, generator=g, device=out.device)
    t = torch.where(pick < 0.15, out, t)
    t = torch.where((pick >= 0.15) & (pick < 0.30), torch.zeros_like(t), t)
    t = torch.where((pick >= 0.30) & (pick < 0.45), torch.ones_like(t), t)
    return t.contiguous()


CASES = [(c, k) for c in (16, 32, 64) for k in (3, 4, 5)] + [(128, 3), (128, 5)]   # (128 channels: the small shapes only)


@pytest.mark.parametrize("c,n_cls", CASES, ids=["C%d-k%d" % ck for ck in CASES])
def test_head_train_equals_the_three_launches(dev, c, n_cls):
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    idx = CASES.index((c, n_cls))
    refused = (4 if n_cls <= 4 else 8) > c // 4      # head_fwd takes its tiled kernel there: other bits
    run = 0
    zero_grads = 0
    for si, (n, h, w) in enumerate(_shapes()[:3 if c == 128 else 4]):
        big = si == 3
        g = torch.Generator(device=dev).manual_seed(7000 + 10 * idx + si)
        x = torch.randn(n, h, w, c, generator=g, device=dev)
        wt = torch.randn(n_cls, c, generator=g, device=dev) * (2.0 / c) ** 0.5
        bias = torch.randn(n_cls, generator=g, device=dev) * 0.5
        seed = head_seed(0x7EA10000 + idx, si)
        seed_dev = torch.tensor([WORD], dtype=torch.int64, device=dev)
        # the large shape once per (C, n_cls): the modes rotate over the nine pairs
        wanted = (idx % 3,) if big else (0, 1, 2)
        km = mask = None
        if wanted != (0,):
            km = torch.from_numpy(keep_mask(seed, n, h, w, c, P_DROP)).to(dev)
            mask = km.to(torch.uint8).contiguous()
        modes = ((0, 0.0, seed, None, None), (1, P_DROP, (seed - WORD) & MASK64, None, seed_dev), (2, P_DROP, seed, mask, None))
        for d, p, sd, mk, sdev in [modes[m] for m in wanted]:
            gate, heads = bool((run + idx) & 1), 1 + (run + idx // 3) % 3
            gam = (3.0, 3.0, 2.0, 0.5)[(run + idx) % 4]     # the cube, powf and the gamma < 1 instantiation of focal_element
            run += 1
            out_ref, fname = run_fwd(x, wt, bias, p, sd, mk, seed_dev=sdev)
            target = _target(out_ref, g)
            others = [torch.rand(out_ref.shape, generator=g, device=dev) for _ in range(heads - 1)]
            preds = others[:1] + [out_ref] + others[1:]      # this head is not always the first of the mean
            rows_div = n * n_cls
            _, grads = ops.focal_bce_heads(preds, target, rows_div, gam)
            d_out = grads[len(others[:1])]
            zero_grads += int((d_out == 0).sum())
            out = torch.full_like(out_ref, float("nan"))
            dx = torch.full_like(x, float("nan"))
            part = torch.full((_blocks(n * h * w) * (n_cls * c + n_cls),), float("nan"), device=dev)
            got = ops.head_train(x, wt, bias, target, rows_div, gam, heads, p, sd, mk, out, dx, gate_x=gate, seed_dev=sdev,
                                 partial=part)
            what = (c, n_cls, (n, h, w), "D%d" % d, "gate" if gate else "-", heads, gam)
            if refused:
                assert not fname.startswith("head_fwd_stream"), what
                torch.cuda.synchronize()
                assert got is None and bool(torch.isnan(out).all()) and bool(torch.isnan(dx).all()) and bool(
                    torch.isnan(part).all()), what
                continue
            assert got is not None, what
            name = _lib.lib().unetpp_last_kernel_name().decode()
            assert name == "head_train_pow2<%d,%d,%d>" % ((c // 4).bit_length() - 1, d, 4 if n_cls <= 4 else 8), what
            assert fname.startswith("head_fwd_stream"), what
            dw, db = got
            dx_ref, rows_ref = _bwd_rows(d_out, out_ref, x, wt, p, sd, mk, gate, sdev)
            dx_ref2, dw_ref, db_ref, bname = run_bwd(d_out, out_ref, x, wt, p, sd, mk, None, False, gate, seed_dev=sdev)
            assert bname.startswith("head_bwd_pow2"), what
            torch.cuda.synchronize()
            for label, a, b in (("map", out, out_ref), ("dx", dx, dx_ref), ("dx (ops.head_bwd)", dx, dx_ref2),
                                ("partial rows", part.view_as(rows_ref), rows_ref), ("dW", dw.reshape(n_cls, c), dw_ref),
                                ("db", db, db_ref)):
                # bit for bit: the same NaNs too, and -0.0 is not +0.0
                differ = int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())
                assert differ == 0, what + (label, "%d of %d elements differ" % (differ, a.numel()))
            # float64 restatement, the bounds of tests/test_gpu_heads.py
            ms = None if d == 0 else km.double() * keep_scale(P_DROP)
            x64, wt64 = x.double(), wt.double()
            z, mag = ref_forward(x64, wt64, bias.double(), ms)
            r = bound_ratio(out, torch.sigmoid(z), out_bound(z, gamma(c + 2) * mag))
            print("head_train %s: out ratio %.3f" % (what, r))
            assert r <= 1.0, what + (r,)
            want_dx, dmag, want_dw, want_db = ref_backward(d_out.double(), out.double(), x64, wt64, ms, None, gate)
            r = bound_ratio(dx, want_dx, gamma(n_cls + 5) * dmag)
            print("head_train %s: dx ratio %.3f" % (what, r))
            assert r <= 1.0, what + (r,)
            assert rel_err(dx.cpu(), want_dx.cpu()) < TOL, what
            assert rel_err(dw.reshape(n_cls, c).cpu(), want_dw.cpu()) < TOL, what + ("dW",)
            assert rel_err(db.cpu(), want_db.cpu()) < TOL, what + ("db",)
    if not refused:
        assert zero_grads > 0, "no exact hit met the kernel"


def test_head_train_refuses_what_it_cannot_take(dev):
    """bf16 storage, a head count outside 1..8, rows < 1, channel counts off 4 * 2^k: None, and nothing is launched"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    x = torch.randn(1, 8, 8, 32, device=dev)
    wt, bias = torch.randn(4, 32, device=dev), torch.randn(4, device=dev)
    t = torch.rand(1, 4, 8, 8, device=dev)

    def call(xx=x, ww=wt, heads=3, rows=4):
        out, dx = torch.full_like(t, float("nan")), torch.full_like(xx, float("nan"))
        got = ops.head_train(xx, ww, bias, t, rows, 3.0, heads, 0.0, 0, None, out, dx)
        torch.cuda.synchronize()
        return got, bool(torch.isnan(out).all())

    assert call()[0] is not None
    for kw in (dict(heads=0), dict(heads=9), dict(rows=0), dict(xx=torch.randn(1, 8, 8, 24, device=dev), ww=torch.randn(4, 24, device=dev)),
               dict(xx=torch.randn(1, 8, 8, 8, device=dev), ww=torch.randn(4, 8, device=dev))):
        got, untouched = call(**kw)
        assert got is None and untouched, kw
    assert ops.head_train(x.to(torch.bfloat16), wt, bias, t, 4, 3.0, 3, 0.0, 0, None, torch.empty_like(t),
                          torch.empty_like(x).to(torch.bfloat16)) is None


# --------------------------------------------------------------------------------------------- (b) the whole step
def _step_module(monkeypatch, old_path):
    """the package's step module as the environment selects it"""
    from unet_nested4tiny_objects_keypoints_amd import step
    if old_path:
        monkeypatch.setenv("UNETPP_NO_FUSED_HEAD_TRAIN", "1")
    else:
        monkeypatch.delenv("UNETPP_NO_FUSED_HEAD_TRAIN", raising=False)
    return importlib.reload(step)


def _run_steps(dev, monkeypatch, old_path, head, criterion, feature_scale=2, n_classes=4, steps=2):
    """-> (per step: outputs, loss, gradients, buffers; the ops.head_train calls of the run as `launched?` flags)"""
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, ops
    step = _step_module(monkeypatch, old_path)
    assert step._FUSED_HEAD_TRAIN is (not old_path)
    calls = []
    real = ops.head_train

    def counted(*a, **k):
        got = real(*a, **k)
        calls.append(got is not None)
        return got

    monkeypatch.setattr(ops, "head_train", counted)
    torch.manual_seed(11)
    model = UNet_Nested(in_channels=1, n_classes=n_classes, feature_scale=feature_scale).to(dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    g = torch.Generator().manual_seed(5)
    record = []
    for s in range(steps):
        x = torch.randn(2, 1, 32, 32, generator=g).to(dev)
        t = torch.rand(2, n_classes, 32, 32, generator=g).to(dev)
        torch.manual_seed(100 + s)       # the dropout seeds of the step
        outs, loss = step.train_step(model, opt, criterion, x, t, head=head)
        torch.cuda.synchronize()
        record.append(([o.detach().clone() for o in outs], loss.detach().clone(),
                       {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()},
                       {k: b.clone() for k, b in model.named_buffers()}))
    monkeypatch.setattr(ops, "head_train", real)
    return record, calls


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    assert torch.equal(a, b), what


def _same_steps(new, old, n_heads):
    assert len(new) == len(old)
    for s, ((o1, l1, g1, b1), (o2, l2, g2, b2)) in enumerate(zip(new, old)):
        assert len(o1) == len(o2) == n_heads
        for j, (a, b) in enumerate(zip(o1, o2)):
            _same_bits(a, b, ("output", s, j))
        _same_bits(l1.reshape(()), l2.reshape(()), ("loss", s))
        assert g1.keys() == g2.keys() and any(v is not None for v in g1.values())
        for k in g1:
            assert (g1[k] is None) == (g2[k] is None), ("grad", s, k)
            if g1[k] is not None:
                _same_bits(g1[k], g2[k], ("grad", s, k))
        assert b1.keys() == b2.keys() and any("running_mean" in k for k in b1)
        for k in b1:
            _same_bits(b1[k], b2[k], ("buffer", s, k))


# feature_scale 4 is 8 channels at level 0: four padded classes on two lanes, which unetpp_head_fwd gives to its tiled
# kernel -- unetpp_head_train refuses the first head and the step runs the three launches (one refused call per step).
# feature_scale 2 is 16 channels: the new kernel takes every head.
STEP_CASES = [(fs, head) for fs in (4, 2) for head in (None, 1, 2)]


@pytest.mark.parametrize("fs,head", STEP_CASES, ids=["fs%d-%s" % (fs, "whole" if h is None else "cut%d" % h) for fs, h in STEP_CASES])
def test_train_step_with_head_train_equals_the_three_launch_step(dev, monkeypatch, fs, head):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d
    try:
        new, new_calls = _run_steps(dev, monkeypatch, False, head, FocalLoss_BCE_2d(gamma=3, size_average=False), fs)
        old, old_calls = _run_steps(dev, monkeypatch, True, head, FocalLoss_BCE_2d(gamma=3, size_average=False), fs)
    finally:
        _step_module(monkeypatch, False)
    n_heads = 3 if head is None else head
    assert old_calls == []
    assert new_calls == ([True] * (2 * n_heads) if fs == 2 else [False, False]), new_calls
    _same_steps(new, old, n_heads)


def test_other_criteria_and_refused_heads_take_the_old_path(dev, monkeypatch):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d

    class Halved(FocalLoss_BCE_2d):
        def forward(self, input, target):
            return 0.5 * super().forward(input, target)

    try:
        _, calls = _run_steps(dev, monkeypatch, False, None, Halved(gamma=3, size_average=False), steps=1)
        assert calls == []
        _, calls = _run_steps(dev, monkeypatch, False, None, FocalLoss_BCE_2d(gamma=3, ignore_negative=True), steps=1)
        assert calls == []
        # 5 classes on 16 channels: the library refuses the first head, the step runs the three launches and still agrees
        new, calls = _run_steps(dev, monkeypatch, False, None, FocalLoss_BCE_2d(gamma=3), n_classes=5, steps=1)
        assert calls == [False]
        old, _ = _run_steps(dev, monkeypatch, True, None, FocalLoss_BCE_2d(gamma=3), n_classes=5, steps=1)
    finally:
        _step_module(monkeypatch, False)
    _same_steps(new, old, 3)


def test_graphed_step_takes_the_new_path_and_replays_the_eager_bits(dev, monkeypatch):
    """GraphedTrainStep captures forward_loss_backward: the head_train launches are in the graph, the dropout seed reaches
    them through seed_dev, and a replay equals the eager step of the same seed bit for bit."""
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, GraphedTrainStep, UNet_Nested, ops, step
    calls = []
    real = ops.head_train

    def counted(*a, **k):
        got = real(*a, **k)
        calls.append((got is not None, k.get("seed_dev") is not None))
        return got

    monkeypatch.setattr(ops, "head_train", counted)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    torch.manual_seed(3)
    model = UNet_Nested(in_channels=1, n_classes=4, feature_scale=2).to(dev).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    x, t = torch.randn(2, 1, 32, 32, device=dev), torch.rand(2, 4, 32, 32, device=dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    graphed = GraphedTrainStep(model, opt, crit, x, t, check_topology=True)
    assert calls and all(launched and by_word for launched, by_word in calls), calls
    assert graphed.topology["chain"] and set(graphed.topology["kinds"]) == {"kernel"}, graphed.topology
    torch.manual_seed(77)
    outs, loss = graphed(x, t)
    torch.cuda.synchronize()
    outs, loss = [o.clone() for o in outs], loss.clone()
    grads = {k: p.grad.clone() for k, p in model.named_parameters()}
    seed = int(graphed._seed.item())
    # the eager step whose by-value seed is the replay's device word
    model.load_state_dict(state)
    monkeypatch.setattr(torch, "randint", lambda *a, **k: torch.tensor([seed]))
    outs2, loss2 = step.train_step(model, opt, crit, x, t)
    torch.cuda.synchronize()
    for a, b in zip(outs, outs2):
        _same_bits(a, b, "output")
    _same_bits(loss.reshape(()), loss2.detach().reshape(()), "loss")
    for k, p in model.named_parameters():
        _same_bits(grads[k], p.grad, ("grad", k))
