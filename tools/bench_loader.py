"""Time the device input pipeline: DeviceLoader.batch() (draw + warp) against the same batch built from torch ops on the
same GPU, and the warp launch alone.

    python tools/bench_loader.py [--reps 7] [--steps 50] [--out profiles/loader/bench_loader_mi355x.json]

Parts (each runs in a child process of its own under a time limit; a part that fails or overruns ends the run, nothing
more is started on the GPU after it):
  headline        uint8 store [4096, 256, 256, 1] (268 MB), batch 32 -> [32, 1, 256, 256]; the exact family (flips,
                  quarter turns, whole-pixel shifts of up to 16 px), contrast and brightness
  headline:rot    the same with rotation (+-30 degrees) and scale (0.75 .. 1.33) switched on
  rgb512          uint8 store [1024, 512, 512, 3] (805 MB), batch 32 -> [32, 3, 512, 512]
  rgb512:rot      the same with rotation and scale
Every part carries 6 labels per sample.  Contenders, all in the same process, alternating inside every repetition:
  device_loader   DeviceLoader.batch(index): a seed from the host generator, the draw launch, the warp launch
  warp_alone      the warp launch with rows drawn beforehand
  torch_path      store[index] -> permute / float -> F.affine_grid + F.grid_sample (bilinear, zeros, align_corners=True)
                  from the same matrices -> normalise, gain, bias -> labels[index] through a batched matmul and the frame
                  test.  Its normalised matrices are prepared outside the timed region (in its favour).
Per contender and repetition: `steps` calls between two HIP events (device ms per call: the stream's time from the first
launch to the last, host-induced gaps included) and the host wall time of the calls (the queue drained before and
after); after a warm-up, medians over the repetitions.  Bytes are the algorithm's: the gathered samples read once, the
batch written once.  GB/s is set against the 6.29 TB/s a device copy reaches on an MI355X.  max_abs_diff is the largest
difference between the torch path's batch and the warp's, as a check that both computed the same thing.
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

SHAPES = {
    "headline": dict(M=4096, side=256, C=1),
    "rgb512": dict(M=1024, side=512, C=3),
}
PARTS = {"headline": 240, "headline:rot": 240, "rgb512": 300, "rgb512:rot": 300}   # part -> its time limit in seconds
BATCH, LABELS = 32, 6
COPY_GBPS = 6290.0
DEFAULT_OUT = os.path.join(ROOT, "profiles", "loader", "bench_loader_mi355x.json")


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


def run_shape(name, rot, args):
    import torch
    import torch.nn.functional as F

    from unet_nested4tiny_objects_keypoints_amd import Augment, DeviceLoader, ops
    dev = torch.device("cuda:0")
    shape = SHAPES[name]
    M, side, C = shape["M"], shape["side"], shape["C"]
    g = torch.Generator(device=dev).manual_seed(0)
    store = torch.randint(0, 256, (M, side, side, C), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.rand(M, LABELS, 2, device=dev, generator=g) * (side - 1)
    aug = Augment(translate=(16, 16), contrast=(0.8, 1.25), brightness=0.1,
                  rotate=30.0 if rot else 0.0, scale=(0.75, 4.0 / 3.0) if rot else (1.0, 1.0))
    mul, add = [1.0 / 255.0] * C, [-0.5] * C
    loader = DeviceLoader(store, labels, (side, side), mul=mul, add=add, fill=0.0, augment=aug, seed=0)
    index = torch.randint(0, M, (BATCH,), device=dev, generator=g)
    rows = aug.draw(BATCH, 1234, (side, side), (side, side), dev)

    # the torch path's matrices: the inverse map in normalised coordinates (align_corners=True), the forward map as is
    m = rows[:, :6].double()
    s = float(side - 1)
    theta = torch.stack([m[:, 0], m[:, 1], (m[:, 0] * s + m[:, 1] * s + 2 * m[:, 2]) / s - 1,
                         m[:, 3], m[:, 4], (m[:, 3] * s + m[:, 4] * s + 2 * m[:, 5]) / s - 1], dim=1).float().view(BATCH, 2, 3)
    fwd = rows[:, 6:12].view(BATCH, 2, 3)
    fwd_lin_t, fwd_off = fwd[:, :, :2].transpose(1, 2).contiguous(), fwd[:, :, 2].unsqueeze(1).contiguous()
    gain, bias = rows[:, 12].view(BATCH, 1, 1, 1), rows[:, 13].view(BATCH, 1, 1, 1)
    mul_t, add_t = loader.mul.view(1, C, 1, 1), loader.add.view(1, C, 1, 1)

    def torch_path():
        x = store[index].permute(0, 3, 1, 2).float()
        grid = F.affine_grid(theta, (BATCH, C, side, side), align_corners=True)
        y = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        y = gain * (y * mul_t + add_t) + bias
        src = labels[index]
        pts = torch.bmm(src, fwd_lin_t) + fwd_off
        none = (src < 0).any(dim=2, keepdim=True)
        pts = torch.where(none, torch.full_like(pts, -1.0), pts)
        inside = ((pts >= 0) & (pts <= s)).all(dim=2) & ~none.squeeze(2)
        return y, pts, inside.to(torch.uint8)

    def warp_alone():
        return ops.warp_batch(store, index, rows, (side, side), loader.mul, loader.add, 0.0, labels)

    contenders = {
        "device_loader": lambda: loader.batch(index),
        "warp_alone": warp_alone,
        "torch_path": torch_path,
    }
    ours, theirs = warp_alone(), torch_path()
    diff = float((ours[0] - theirs[0]).abs().max())
    label_diff = float((ours[1] - theirs[1]).abs().max())
    inside_differ = int((ours[2] != theirs[2]).sum())
    res = alternate(contenders, args.reps, args.steps)
    for k, fn in contenders.items():
        res[k]["launches_per_call"] = launches_of(fn)
    nbytes = BATCH * C * side * side * (1 + 4) + BATCH * LABELS * (8 + 8 + 1)
    for k in contenders:
        res[k]["bytes_per_call"] = nbytes
        res[k]["GBps"] = nbytes / (res[k]["device_ms_per_call"] * 1e-3) / 1e9
        res[k]["fraction_of_copy_rate"] = res[k]["GBps"] / COPY_GBPS
    return {"store": [M, side, side, C], "batch": BATCH, "labels_per_sample": LABELS, "augment": repr(aug),
            "contenders": res, "max_abs_diff_vs_torch": diff, "max_label_diff_vs_torch": label_diff,
            "inside_flags_that_differ": inside_differ,
            "device_loader_over_torch_path": res["device_loader"]["device_ms_per_call"] / res["torch_path"]["device_ms_per_call"],
            "torch_path_over_device_loader": res["torch_path"]["device_ms_per_call"] / res["device_loader"]["device_ms_per_call"]}


def run_part(part, args):
    import torch

    import __graft_entry__ as entry
    entry.build()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader: no GPU (this tool measures on the device only)")
    name, _, mode = part.partition(":")
    res = run_shape(name, mode == "rot", args)
    res["device"] = torch.cuda.get_device_name(0)
    with open(args.part_out, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)        # child mode
    ap.add_argument("--part-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part is not None:
        run_part(args.part, args)
        return
    res = {"reps": args.reps, "steps": args.steps, "copy_rate_GBps": COPY_GBPS, "parts": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for part in args.parts.split(","):
            if part not in PARTS:
                raise SystemExit("unknown part %r (known: %s)" % (part, ", ".join(PARTS)))
            out = os.path.join(tmp, part.replace(":", "_") + ".json")
            cmd = ["timeout", "-k", "10", str(PARTS[part]), sys.executable, os.path.abspath(__file__), "--part", part,
                   "--part-out", out, "--reps", str(args.reps), "--steps", str(args.steps)]
            print("bench_loader:", part, flush=True)
            status = subprocess.run(cmd).returncode
            if status != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
                raise SystemExit("bench_loader: part %s ended with status %d; stopping" % (part, status))
            with open(out) as f:
                res["parts"][part] = json.load(f)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
