"""unetpp_gemm_plan against what runs: ops.gemm_fwd returns the library's plan of its launch, and the kernel the launch
names afterwards (unetpp_last_kernel_name) is the planned one -- per kernel and form, at the smallest shapes that reach
it (rows of tests/test_gemm_plan.py's table, whose labels were recorded from the library before the plan existed).
Two rows carry a fused BatchNorm finalize: it reads plan.bn_rows rows, and what it leaves is held against float64
statistics of the stored output (tests/test_gpu_persistent.py's check and tolerance for the same quantities)."""
import json

import pytest
import torch

from tests.helpers import rel_err
from tests.test_gemm_plan import CASES, GOLDEN

pytestmark = pytest.mark.gpu

# (row of CASES, switch to set or None)
ROWS = [("wino-32-32", None), ("wino-32-32-w32", None), ("wino-64+32-64", None), ("wino-fold", None), ("wino-strided", None),
        ("direct-32-32", None), ("pw-64-32", None), ("pw-deconv-64-4x32", None), ("1x1-w24", None),
        ("generic-unaligned-30-32", None), ("generic-gate-on-load", None), ("first-layer-cin1", None),
        ("bf16-first-layer-cin3", None), ("bf16-32-64-small", None), ("bf16-32-32-one-chunk-one-tile", None),
        ("bf16-32-64-16-units", ("BF16_DMA_MIN8", 0)), ("bf16-stats", None), ("bf16-fold", None),
        ("bf16-pointwise-w24-plain", None), ("bf16-pw-64-4x32", None), ("bf16-pw-dgrad-4x32-64", None)]
BN_ROWS = ["wino-32-32-w32", "first-layer-cin1"]


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as entry
    entry.build()
    return torch.device("cuda:0")


def _launch(dev, args, bn=False):
    """the row's launch through ops.gemm_fwd on random data -> (plan, label the launch left, output tensors, finalize)"""
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    n, h, w, taps = args["n"], args["h"], args["w"], args["taps"]
    bf = "bf16" in args.get("flags", "")
    g = torch.Generator().manual_seed(5)

    def views(specs, is_out):
        out = []
        for s in specs:
            # bf16 storage: every activation is bf16 but the network input of the first layer
            dt = torch.bfloat16 if bf and (is_out or s["c"] > 4) else torch.float32
            t = torch.randn(n, h * s["up"], w * s["up"], s["c"], generator=g).to(dev, dt)
            kw = dict(c_off=s["c_off"], c_len=s["c_len"], sy=s["up"], sx=s["up"], oy=s["oy"], ox=s["ox"],
                      relu=s["relu"] or s["fold"], accumulate=s["accumulate"])
            if s["fold"]:
                kw.update(scale=torch.rand(s["c_len"], generator=g).to(dev) + 0.5, shift=torch.randn(s["c_len"], generator=g).to(dev))
            if s["gate"]:
                kw.update(gate=torch.randn(t.shape, generator=g).to(dev, dt))
            out.append(ops.V(t, **kw))
        return out

    ins, outs = views(args["ins"], False), views(args["outs"], True)
    k, nc = sum(s["c_len"] for s in args["ins"]), sum(s["c_len"] for s in args["outs"])
    weight = (0.1 * torch.randn(taps * k * nc, generator=g)).to(dev)
    fin, part = None, None
    if bn or args.get("stats"):
        rows = ops.gemm_stats_rows(n, h, w) if bn else ops.gemm_pixel_blocks(n, h, w)
        part = torch.full((rows * nc * 2,), float("nan"), device=dev)
    if bn:
        fin = ops.BatchNormFinish(torch.rand(nc, generator=g).to(dev) + 0.5, torch.randn(nc, generator=g).to(dev),
                                  torch.zeros(nc, device=dev), torch.ones(nc, device=dev), 1e-5, 0.1, n * h * w)
    plan = ops.gemm_fwd(n, h, w, taps, ins, outs, weight, None, part, direct="direct" in args.get("flags", ""), bn=fin)
    label = _lib.lib().unetpp_last_kernel_name().decode()
    torch.cuda.synchronize()
    return plan, label, [v.t for v in outs], fin, part


@pytest.mark.parametrize("case,switch", ROWS, ids=[r[0] for r in ROWS])
def test_launch_runs_the_planned_kernel(dev, case, switch):
    from unet_nested4tiny_objects_keypoints_amd import _lib
    with open(GOLDEN) as f:
        rec = json.load(f)["rows"][case]
    want = rec["base"]["label"]
    if switch is None:
        plan, label, outs, _, _ = _launch(dev, CASES[case])
    else:
        with _lib.debug_switch(*switch):
            plan, label, outs, _, _ = _launch(dev, CASES[case])
        assert plan.threads == 512   # the 8-wave LDS-DMA form, reached at this size by lowering its unit threshold
    assert plan.kernel.decode() == label == want, (case, plan.kernel, label, want)
    assert (plan.image_floats > 0) == CASES[case].get("image", True) and plan.image_floats in (0, rec["image_floats"])
    if switch is None and _lib.lib().unetpp_usable_cus(None) == 256:   # the record's grids are those of 256 CUs
        assert (plan.workgroups, plan.threads) == (rec["base"]["workgroups"], rec["base"]["threads"])
    assert all(bool(torch.isfinite(t.float()).all()) for t in outs), case


@pytest.mark.parametrize("case", BN_ROWS)
def test_fused_finalize_reads_the_planned_rows(dev, case):
    from tests.test_gpu_persistent import check_bn_finish
    args = CASES[case]
    plan, label, outs, fin, part = _launch(dev, args, bn=True)
    assert plan.kernel.decode() == label
    nc = outs[0].shape[3]
    # one row per workgroup, and exactly those rows were written
    assert plan.bn_rows == plan.workgroups > 0, (plan.bn_rows, plan.workgroups)
    written = ~torch.isnan(part.view(-1, nc * 2)).all(dim=1)
    assert int(written.sum()) == plan.bn_rows and bool(written[:plan.bn_rows].all())
    y = outs[0].float().cpu().permute(0, 3, 1, 2)
    check_bn_finish(case, 0, fin, y, torch.zeros(nc, dtype=torch.float64), torch.ones(nc, dtype=torch.float64), 0.1, 1e-5)
    yd = y.double().permute(0, 2, 3, 1).reshape(-1, nc)   # shift = beta - mean * scale, to the same relative 1e-5
    scale = fin.gamma.double().cpu() / (yd.var(0, unbiased=False) + 1e-5).sqrt()
    assert rel_err(fin.shift.cpu(), fin.beta.double().cpu() - yd.mean(0) * scale) < 1e-5, case
