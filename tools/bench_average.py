"""Time weight averaging: WeightAverager.update() / a swap against torch.optim.swa_utils.AveragedModel, and update_bn's
encoder-only statistics pass against a whole training-mode forward.

    python tools/bench_average.py [--reps 7] [--steps 50] [--bn-steps 10] [--out profiles/average/bench_average_mi355x.json]

Parts (each runs in a child process of its own under a time limit; a part that fails or overruns ends the run, nothing
more is started on the GPU after it):
  update:headline   UNet_Nested(1, 4, feature_scale=1): 2 207 244 parameters
  update:configs4   depth 5, base 64 (in 3, 5 maps): 36 167 124 parameters
  bn                headline network, batch 32, 256x256
Contenders of an update part, all in the same process, alternating inside every repetition:
  fused_mean / fused_ema      WeightAverager.update() (one launch; parameters averaged, buffers copied)
  swap_kernel_pair            the swap launch alone, twice (so the state is restored)
  applied_enter_exit          `with avg.applied(): pass` -- two swaps with their counter copies and invalidations
  torch_swa_mean / torch_swa_ema   AveragedModel(model).update_parameters(model): foreach over the parameters, one
                              copy per buffer
Per contender and repetition: `steps` calls between two HIP events (device ms per call: the stream's time from the first
launch to the last, host-induced gaps included) and the host wall time of the calls (the queue drained before and
after); after a warm-up, medians over the repetitions.  Bytes are the algorithm's: every element of every stream read
or written once.  The bn part times engine.stats_pass and model(x) (training mode, no_grad) the same way.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAM_SETS = {
    "headline": dict(in_channels=1, n_classes=4, feature_scale=1),
    "configs4": dict(in_channels=3, n_classes=5, feature_scale=0.5, depth=5),
}
PARTS = {"update:headline": 300, "update:configs4": 300, "bn": 420}   # part -> its time limit in seconds
DEFAULT_OUT = os.path.join(ROOT, "profiles", "average", "bench_average_mi355x.json")


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h0 = time.perf_counter()
    for _ in range(steps):
        fn()
    h1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (h1 - h0) * 1e3 / steps


def launches_of(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def alternate(contenders, reps, steps, warmup=3):
    samples = {k: ([], []) for k in contenders}
    for fn in contenders.values():
        for _ in range(warmup):
            fn()
    for _ in range(reps):
        for k, fn in contenders.items():
            d, h = timed(fn, steps)
            samples[k][0].append(d)
            samples[k][1].append(h)
    return {k: {"device_ms_per_call": statistics.median(s[0]), "host_ms_per_call": statistics.median(s[1]),
                "device_ms_samples": s[0]} for k, s in samples.items()}


def part_update(name, args):
    import torch
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, WeightAverager, _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = UNet_Nested(**PARAM_SETS[name]).to(dev)
    n_param = sum(p.numel() for p in model.parameters())
    n_buf = sum(b.numel() for b in model.buffers() if b.is_floating_point())
    mean, ema = WeightAverager(model, kind="mean"), WeightAverager(model, kind="ema", decay=0.999)
    swa = AveragedModel(model)
    swa_ema = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.999))
    table = mean._table()

    def swap_pair():
        table.launch(_lib.AVG_SWAP)
        table.launch(_lib.AVG_SWAP)

    def enter_exit():
        with mean.applied():
            pass

    contenders = {
        "fused_mean": mean.update,
        "fused_ema": ema.update,
        "swap_kernel_pair": swap_pair,
        "applied_enter_exit": enter_exit,
        "torch_swa_mean": lambda: swa.update_parameters(model),
        "torch_swa_ema": lambda: swa_ema.update_parameters(model),
    }
    res = alternate(contenders, args.reps, args.steps)
    for k, fn in contenders.items():
        res[k]["launches_per_call"] = launches_of(fn)
    update_bytes = 12 * n_param + 8 * n_buf        # avg and src read, avg written; buffers copied
    swap_bytes = 2 * 16 * (n_param + n_buf)        # a pair: both streams read and written, twice
    torch_bytes = update_bytes                     # lerp over the parameters, one copy_ per buffer
    for k, b in (("fused_mean", update_bytes), ("fused_ema", update_bytes), ("swap_kernel_pair", swap_bytes),
                 ("torch_swa_mean", torch_bytes), ("torch_swa_ema", torch_bytes)):
        res[k]["bytes_per_call"] = b
        res[k]["GBps"] = b / (res[k]["device_ms_per_call"] * 1e-3) / 1e9
    return {"tensors": len(mean._float_names), "params": n_param, "float_buffer_elements": n_buf, "contenders": res,
            "fused_mean_over_torch_swa_mean": res["fused_mean"]["device_ms_per_call"] / res["torch_swa_mean"]["device_ms_per_call"],
            "fused_ema_over_torch_swa_ema": res["fused_ema"]["device_ms_per_call"] / res["torch_swa_ema"]["device_ms_per_call"]}


def part_bn(args):
    import torch

    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, WeightAverager, engine
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = UNet_Nested(**PARAM_SETS["headline"]).to(dev).train()
    x = torch.randn(32, 1, 256, 256, device=dev)
    avg = WeightAverager(model)
    avg.update()
    batches = [x] * 4

    def whole():
        with torch.no_grad():
            model(x)

    contenders = {
        "stats_pass_encoder_only": lambda: engine.stats_pass(model, x),
        "whole_training_forward_no_grad": whole,
        "update_bn_4_batches": lambda: avg.update_bn(batches),
    }
    res = alternate(contenders, args.reps, args.bn_steps)
    res["update_bn_4_batches"]["device_ms_per_batch"] = res["update_bn_4_batches"]["device_ms_per_call"] / len(batches)
    return {"batch": 32, "height": 256, "width": 256, "contenders": res,
            "stats_pass_over_whole_forward": res["stats_pass_encoder_only"]["device_ms_per_call"] /
            res["whole_training_forward_no_grad"]["device_ms_per_call"]}


def run_part(part, args):
    import torch

    import __graft_entry__ as entry
    entry.build()
    if not torch.cuda.is_available():
        raise SystemExit("bench_average: no GPU (this tool measures on the device only)")
    res = part_bn(args) if part == "bn" else part_update(part.split(":", 1)[1], args)
    res["device"] = torch.cuda.get_device_name(0)
    with open(args.part_out, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--bn-steps", type=int, default=10)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)        # child mode
    ap.add_argument("--part-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part is not None:
        run_part(args.part, args)
        return
    res = {"reps": args.reps, "steps": args.steps, "bn_steps": args.bn_steps, "parts": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for part in args.parts.split(","):
            if part not in PARTS:
                raise SystemExit("unknown part %r (known: %s)" % (part, ", ".join(PARTS)))
            out = os.path.join(tmp, part.replace(":", "_") + ".json")
            cmd = ["timeout", "-k", "10", str(PARTS[part]), sys.executable, os.path.abspath(__file__), "--part", part,
                   "--part-out", out, "--reps", str(args.reps), "--steps", str(args.steps), "--bn-steps", str(args.bn_steps)]
            print("bench_average:", part, flush=True)
            status = subprocess.run(cmd).returncode
            if status != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
                raise SystemExit("bench_average: part %s ended with status %d; stopping" % (part, status))
            with open(out) as f:
                res["parts"][part] = json.load(f)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
