"""CPU-only checks of the host side that mirrors the reference's module API (models/unet.py:204-300):
constructor defaults, attributes, state-dict contract, initialisation statistics, loss and step helpers."""
import math

import pytest
import torch

from oracle.step_oracle import focal_bce_2d_oracle
from oracle.unet_nested_oracle import UNetNestedOracle
from tests.helpers import GOLDEN_CASES, load_golden, sub
from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet_Nested, count_param


def test_zero_arg_constructor_matches_reference_defaults():
    m = UNet_Nested()  # trainer/trainer.py:337 builds it with no arguments
    assert (m.in_channels, m.feature_scale, m.is_deconv, m.is_batchnorm, m.is_ds) == (3, 2, True, True, True)
    assert count_param(m) == 553260          # the "2.2MB" weights file of README.md:12
    assert count_param(UNet_Nested(1, 4, feature_scale=1)) == 2207244
    assert count_param(UNet_Nested(1, 4, feature_scale=4)) == 138828
    assert isinstance(m.drop_out, torch.nn.Dropout) and m.drop_out.p == 0.4


@pytest.mark.parametrize("kw", [dict(), dict(is_deconv=False), dict(is_batchnorm=False), dict(in_channels=1, n_classes=5),
                                dict(depth=5, feature_scale=4), dict(depth=2), dict(feature_scale=0.5, depth=3)])
def test_state_dict_contract_equals_oracle(kw):
    a, b = UNet_Nested(**kw).state_dict(), UNetNestedOracle(**kw).state_dict()
    assert list(a.keys()) == list(b.keys())
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_reference_checkpoints_load_strictly(name):
    z, ctor = load_golden(name)
    m = UNet_Nested(**ctor)
    missing, unexpected = m.load_state_dict(sub(z, "state0"), strict=True)
    assert not missing and not unexpected
    # and back: the oracle (== reference layout) accepts what the HIP module saves
    UNetNestedOracle(**ctor).load_state_dict(m.state_dict(), strict=True)


def test_initialisation_statistics():
    torch.manual_seed(0)
    m = UNet_Nested(in_channels=1, n_classes=4, feature_scale=1)
    w = m.up_concat03.conv.conv1[0].weight if hasattr(m.up_concat03.conv.conv1, "__getitem__") else \
        getattr(m.up_concat03.conv.conv1, "0").weight
    fan_in = w.shape[1] * 9
    assert abs(float(w.std()) - math.sqrt(2.0 / fan_in)) < 0.05 * math.sqrt(2.0 / fan_in)   # kaiming normal, fan_in
    bn = getattr(m.conv00.conv1, "1")
    assert abs(float(bn.weight.mean()) - 1.0) < 0.02 and float(bn.bias.abs().max()) == 0.0
    assert float(bn.running_var.min()) == 1.0 and int(bn.num_batches_tracked) == 0
    up = m.up_concat01.up.weight
    assert abs(float(up.std()) - math.sqrt(2.0 / (up.shape[1] * 4))) < 0.05


def test_loss_matches_oracle_and_trainer_semantics():
    torch.manual_seed(1)
    p, t = torch.rand(3, 4, 8, 8), torch.rand(3, 4, 8, 8)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    assert torch.allclose(crit(p, t), focal_bce_2d_oracle(p, t), rtol=1e-6)
    # sum over everything / (N*C): doubling the batch with the same content keeps the value
    assert torch.allclose(crit(torch.cat([p, p]), torch.cat([t, t])), crit(p, t), rtol=1e-6)


def test_invalid_arguments():
    with pytest.raises(ValueError):
        UNet_Nested(depth=1)
    with pytest.raises(ValueError):
        UNet_Nested(feature_scale=64)
    m = UNet_Nested(in_channels=1, feature_scale=8)
    m.dropout_masks = [None]
    with pytest.raises(RuntimeError):   # CPU tensor: no fallback
        m(torch.randn(1, 1, 16, 16))


def test_bench_spawns_its_ranks_and_propagates_failure():
    """`python bench.py --gpus 2` without a launcher starts two rank processes itself (it used to run one GPU
    silently).  Without a GPU every rank refuses to run, and the parent must report that with a non-zero exit code --
    which exercises the spawn path, the environment it hands to the ranks and the failure propagation on CPU."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("CPU-only check (on a GPU box the ranks would run the benchmark)")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "rank exit codes" in r.stderr and "bench.py needs a GPU" in r.stderr
    assert r.stderr.count("bench.py needs a GPU") == 2   # both ranks were started


def test_graphed_train_step_refuses_cpu_tensors_and_eval_models():
    """graph.GraphedTrainStep has no CPU form (this path has no CPU fallback): CPU tensors and eval-mode models are
    refused up front, before anything touches the library."""
    import torch

    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, GraphedTrainStep, UNet_Nested
    m = UNet_Nested(in_channels=1, n_classes=4, feature_scale=8).train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    x, t = torch.randn(1, 1, 32, 32), torch.rand(1, 4, 32, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        GraphedTrainStep(m, opt, crit, x, t)


def test_bench_other_configs_name_the_baseline_configurations():
    """`bench.py --full` attaches BASELINE.json's configs[3] and configs[4] (as single-GPU geometries) to the headline
    line; the table that says which is host logic."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    names = [n for n, _ in bench.OTHER_CONFIGS]
    assert names[0].startswith("configs[3]") and names[1].startswith("configs[4]")
    c3, c4 = bench.OTHER_CONFIGS[0][1], bench.OTHER_CONFIGS[1][1]
    assert (c3["dtype"], c3["size"], c3["depth"], c3["in_channels"], c3["n_classes"]) == ("bf16", 512, 4, 1, 4)
    assert (c4["dtype"], c4["size"], c4["depth"], c4["in_channels"], c4["n_classes"], c4["feature_scale"]) == ("bf16", 384, 5, 3, 5, 0.5)
    base = json.load(open(os.path.join(root, "BASELINE.json")))["configs"]
    assert "512" in base[3] and "bf16" in base[3] and "384" in base[4] and "depth=5" in base[4]
    import argparse
    ns = argparse.Namespace(dtype="f32", size=256, batch=32, feature_scale=1, depth=4, in_channels=1, n_classes=4)
    assert bench.is_headline(ns)
    ns.batch = 8
    assert not bench.is_headline(ns)     # other shapes asked for on the command line stay single-configuration runs


def test_bench_live_pmc_falls_back_without_a_gpu(tmp_path):
    """bench.live_pmc() starts children of bench.py under `rocprofv3 --pmc` before the benchmark touches the GPU.  Whatever goes
    wrong there (here: no GPU, so the first child exits non-zero; elsewhere: no rocprofv3, a timeout) must cost only the
    live counters -- the function returns None, leaves no scratch directory behind, and pmc_counters() then serves the
    committed summary if and only if it was made from this build."""
    import argparse
    import glob
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module_pmc", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    ns = argparse.Namespace(dtype="f32", size=256, batch=32, feature_scale=1, depth=4, in_channels=1, n_classes=4)
    before = set(glob.glob("/tmp/unetpp_pmc_*"))
    os.environ["UNETPP_BENCH_PMC_TIMEOUT"] = "120"
    try:
        assert bench.live_pmc(ns) is None
    finally:
        os.environ.pop("UNETPP_BENCH_PMC_TIMEOUT", None)
    assert set(glob.glob("/tmp/unetpp_pmc_*")) == before
    key = bench.config_key(ns)
    assert key == "f32_d4_fs1_s256_b32_i1_c4"
    assert bench.pmc_counters("gemm_wino_kernel", "not-a-build-hash", key) == (None, None, None)
    bench._LIVE_PMC[key] = {"build_hash": "h", "kernels": [
        {"kernel": "gemm_wino_kernel<5, 2, 1, false>", "launches": 3, "fetch_bytes_x2_per_launch": 100, "write_bytes_per_launch": 20,
         "sq": {"mfma_busy": 0.5, "avg_us": 10.0, "dispatches": 3}},
        {"kernel": "gemm_wino_kernel<5, 2, 2, true>", "launches": 1, "fetch_bytes_x2_per_launch": 60, "write_bytes_per_launch": 20,
         "sq": {"mfma_busy": 0.25, "avg_us": 10.0, "dispatches": 1}}]}
    traffic, busy, source = bench.pmc_counters("gemm_wino_kernel", "h", key)
    assert traffic == round((120 * 3 + 80) / 4) and abs(busy - (0.5 * 30 + 0.25 * 10) / 40) < 1e-4 and source.startswith("live")
    assert bench.pmc_counters("gemm_wino_kernel", "other", key) == (None, None, None)   # a live summary of another build: refused too


def test_bench_dump_outputs_is_complete_bounded_and_repeatable(tmp_path):
    """bench.dump_outputs (`--dump-outputs DIR`): one float32 / float64 .npy per array of the last step (loss, heads, state
    after the optimizer step, gradients), exact while everything fits; over the budget the long arrays shrink to the same
    seeded sample on every call, and the files stay within the budget."""
    import importlib.util
    import os

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module_dump", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    torch.manual_seed(0)
    m = UNet_Nested(in_channels=1, n_classes=4, feature_scale=8)
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    heads = tuple(torch.rand(2, 4, 32, 32) for _ in range(3))
    loss = torch.tensor(0.75)
    state = m.state_dict()

    full = tmp_path / "full"
    bench.dump_outputs(str(full), heads, loss, m)
    names = {f[:-4] for f in os.listdir(full)}
    assert names == {"loss", "head0", "head1", "head2"} | {"state." + k for k in state} | \
        {"grad." + n for n, _ in m.named_parameters()}
    for k, v in state.items():
        a = np.load(full / ("state.%s.npy" % k))
        assert a.dtype == (np.float32 if v.is_floating_point() else np.float64) and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.double().numpy())
    assert np.array_equal(np.load(full / "head1.npy"), heads[1].numpy())
    assert float(np.load(full / "loss.npy")) == 0.75

    budget = 4 * heads[0].numel()   # less than the three heads alone: they must be sampled
    small = []
    for run in ("a", "b"):
        d = tmp_path / run
        written = bench.dump_outputs(str(d), heads, loss, m, budget=budget)
        assert written <= budget
        small.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert sum(a.nbytes for a in small[0].values()) <= budget
    assert small[0].keys() == small[1].keys() and all(np.array_equal(small[0][f], small[1][f]) for f in small[0])
    h0 = small[0]["head0.npy"]
    assert h0.ndim == 1 and h0.size < heads[0].numel()
    idx = np.sort(np.random.default_rng(0).choice(heads[0].numel(), h0.size, replace=False))
    assert np.array_equal(h0, heads[0].numpy().reshape(-1)[idx])


def test_bench_refuses_zero_steps():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def test_bench_plain_run_leaves_the_extras_to_full(monkeypatch, capsys):
    """A plain `bench.py` run measures the configuration named on the command line and nothing else: no rocprofv3 --pmc
    passes, no `other_configs`, no CPU baseline.  `--full` adds all three.  The GPU side (build, measure) is stubbed, so
    this is the run's plan only."""
    import argparse
    import importlib.util
    import json
    import os
    import sys

    import __graft_entry__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_module_plan", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    calls = {"pmc": [], "measure": [], "cpu": 0}

    def fake_measure(args, ctx):
        calls["measure"].append(bench.config_key(args))
        return {"peak_mem_gb": 1.0, "step_runner": "eager", "host_enqueue_ms": 1.0, "host_enqueue_ms_min": 1.0,
                "value": 1000.0, "ms_per_step": 32.0, "fwd_ms_per_img": 0.2 if args.full else None, "roofline": None,
                "roofline_x00": None, "kernels": None, "dp": None, "replicas_identical": None, "n_cls": args.n_classes,
                "fs": args.feature_scale}

    def fake_cpu(args, n_cls):
        calls["cpu"] += 1
        return {"value": 2.0}

    monkeypatch.setattr(bench, "live_pmc", lambda cfg: calls["pmc"].append(bench.config_key(cfg)))   # None: no profiler
    monkeypatch.setattr(bench, "measure", fake_measure)
    monkeypatch.setattr(bench, "cpu_baseline", fake_cpu)
    monkeypatch.setattr(__graft_entry__, "build", lambda: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda index: None)
    for k in list(os.environ):
        if k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "UNETPP_BENCH_LIVE_PMC", "UNETPP_BENCH_OTHERS_FIRST") or \
                k.startswith(("ROCPROF", "ROCP_")):
            monkeypatch.delenv(k)
    monkeypatch.setenv("UNETPP_BENCH_NO_SWEEP", "1")
    headline = bench.config_key(argparse.Namespace(dtype="f32", size=256, batch=32, feature_scale=1, depth=4,
                                                   in_channels=1, n_classes=4))

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--warmup", "1"])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert calls == {"pmc": [], "measure": [headline], "cpu": 0}
    assert line["full"] is False and line["cpu_baseline"] is None and line["other_configs"] is None
    assert line["fwd_ms_per_img"] is None and "speedup_vs_cpu_baseline" not in line
    assert (line["value"], line["ms_per_step"], line["steps"], line["warmup"]) == (1000.0, 32.0, 2, 1)

    calls.update(pmc=[], measure=[], cpu=0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--warmup", "1", "--full"])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    others = [bench.config_key(argparse.Namespace(**dict(vars(bench.parse()), **over))) for _, over in bench.OTHER_CONFIGS]
    assert calls == {"pmc": [headline], "measure": [headline] + others, "cpu": 1}
    assert line["full"] is True and line["cpu_baseline"] == {"value": 2.0} and line["fwd_ms_per_img"] == 0.2
    assert [o["config"] for o in line["other_configs"]] == [n for n, _ in bench.OTHER_CONFIGS]
