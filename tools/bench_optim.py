"""Time optimizer.step() in isolation, and a headline train_step with the unfused and the fused AdamW.

    python tools/bench_optim.py [--reps 5] [--steps 20] [--train-steps 10] [--out profiles/optim_bench.json]

Parameter sets: the headline network (UNet_Nested(1, 4, feature_scale=1): 74 tensors, 2 207 244 parameters) and
configs[4] (in 3, 5 maps, depth 5, base 64: 108 tensors, 36 167 124 parameters), random gradients.  Contenders:
  fused_*      this package's AdamW / AdaBound / SGDW (optim.py: one launch per step);
  unfused_*    the reference's op sequence per tensor with torch ops (restated below: what tools/optimizers/*.py launch);
  torch_adam_fused  torch.optim.Adam(fused=True), for scale.
Per contender and repetition: `steps` steps between two HIP events (device ms per step) and the host wall time of
enqueueing them (host ms per step, the queue is drained before and after); contenders alternate inside every
repetition, the medians over repetitions are reported.  Launches per step come from a torch.profiler run of one step.
The train_step part times whole headline steps (batch 32, 256x256, fp32) with the unfused and the fused AdamW.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAM_SETS = {
    "headline": dict(in_channels=1, n_classes=4, feature_scale=1),
    "configs4": dict(in_channels=3, n_classes=5, feature_scale=0.5, depth=5),
}


class UnfusedAdamW(torch.optim.Optimizer):
    """The reference AdamW's per-tensor op sequence in torch ops (one small kernel per op, as the reference launches)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                m, v, g = st["exp_avg"], st["exp_avg_sq"], p.grad
                st["step"] += 1
                m.mul_(b1).add_(g, alpha=1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                denom = v.sqrt().add_(group["eps"])
                step_size = group["lr"] * math.sqrt(1 - b2 ** st["step"]) / (1 - b1 ** st["step"])
                if group["weight_decay"] != 0:
                    d = torch.mul(p, group["weight_decay"])
                    p.addcdiv_(m, denom, value=-step_size)
                    p.sub_(d)
                else:
                    p.addcdiv_(m, denom, value=-step_size)


class UnfusedAdaBound(torch.optim.Optimizer):
    """The reference AdaBound's per-tensor op sequence in torch ops."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), final_lr=0.1, gamma=1e-3, eps=1e-8, weight_decay=0):
        super().__init__(params, dict(lr=lr, betas=betas, final_lr=final_lr, gamma=gamma, eps=eps,
                                      weight_decay=weight_decay))
        self.base_lrs = [g["lr"] for g in self.param_groups]

    @torch.no_grad()
    def step(self):
        for group, base_lr in zip(self.param_groups, self.base_lrs):
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                m, v, g = st["exp_avg"], st["exp_avg_sq"], p.grad
                st["step"] += 1
                if group["weight_decay"] != 0:
                    g = g.add(p, alpha=group["weight_decay"])
                m.mul_(b1).add_(g, alpha=1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                denom = v.sqrt().add_(group["eps"])
                step_size = group["lr"] * math.sqrt(1 - b2 ** st["step"]) / (1 - b1 ** st["step"])
                f = group["final_lr"] * group["lr"] / base_lr
                lo, hi = f * (1 - 1 / (group["gamma"] * st["step"] + 1)), f * (1 + 1 / (group["gamma"] * st["step"]))
                s = torch.full_like(denom, step_size)
                s.div_(denom).clamp_(lo, hi).mul_(m)
                p.add_(-s)


class UnfusedSGDW(torch.optim.Optimizer):
    """The reference SGDW with the trainer's call (momentum 0): p = p - wd*p per tensor."""

    def __init__(self, params, lr, weight_decay=0):
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self):
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None and group["weight_decay"] != 0:
                    p.add_(p, alpha=-group["weight_decay"])


def contenders(params):
    from unet_nested4tiny_objects_keypoints_amd import AdaBound, AdamW, SGDW
    return {
        "fused_adamw": lambda: AdamW(params, lr=1e-3, weight_decay=1e-4),
        "unfused_adamw": lambda: UnfusedAdamW(params, lr=1e-3, weight_decay=1e-4),
        "fused_adabound": lambda: AdaBound(params, lr=1e-3, weight_decay=1e-4),
        "unfused_adabound": lambda: UnfusedAdaBound(params, lr=1e-3, weight_decay=1e-4),
        "fused_sgdw": lambda: SGDW(params, lr=1e-3, weight_decay=1e-4),
        "unfused_sgdw": lambda: UnfusedSGDW(params, lr=1e-3, weight_decay=1e-4),
        "torch_adam_fused": lambda: torch.optim.Adam(params, lr=1e-3, weight_decay=1e-4, fused=True),
    }


def launches_per_step(opt):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        opt.step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def time_steps(opt, steps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    h1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (h1 - h0) * 1e3 / steps


def bench_param_set(name, ctor, args, dev):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(0)
    model = UNet_Nested(**ctor).to(dev)
    params = list(model.parameters())
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    opts = {k: make() for k, make in contenders(params).items()}
    out = {"tensors": len(params), "params": sum(p.numel() for p in params), "contenders": {}}
    samples = {k: ([], []) for k in opts}
    for k, opt in opts.items():          # warm-up: state, tables, caches
        for _ in range(3):
            opt.step()
    for _ in range(args.reps):           # alternating repetitions
        for k, opt in opts.items():
            d, h = time_steps(opt, args.steps)
            samples[k][0].append(d)
            samples[k][1].append(h)
    for k, opt in opts.items():
        out["contenders"][k] = {"device_ms_per_step": statistics.median(samples[k][0]),
                                "host_ms_per_step": statistics.median(samples[k][1]),
                                "launches_per_step": launches_per_step(opt),
                                "device_ms_samples": samples[k][0]}
    n = out["params"]
    d = out["contenders"]["fused_adamw"]["device_ms_per_step"]
    out["fused_adamw_hbm_TBps"] = 28.0 * n / (d * 1e-3) / 1e12
    return out


def bench_train_step(args, dev):
    from unet_nested4tiny_objects_keypoints_amd import AdamW, FocalLoss_BCE_2d, UNet_Nested, train_step
    torch.manual_seed(0)
    model = UNet_Nested(in_channels=1, n_classes=4, feature_scale=1).to(dev).train()
    x = torch.randn(32, 1, 256, 256, device=dev)
    t = torch.rand(32, 4, 256, 256, device=dev)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    opts = {"unfused_adamw": UnfusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4),
            "fused_adamw": AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)}
    for opt in opts.values():
        for _ in range(3):
            train_step(model, opt, crit, x, t)
    samples = {k: [] for k in opts}
    for _ in range(args.reps):
        for k, opt in opts.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.train_steps):
                train_step(model, opt, crit, x, t)
            e1.record()
            torch.cuda.synchronize()
            samples[k].append(e0.elapsed_time(e1) / args.train_steps)
    res = {k: {"ms_per_step": statistics.median(v), "samples": v} for k, v in samples.items()}
    res["fused_minus_unfused_ms"] = res["fused_adamw"]["ms_per_step"] - res["unfused_adamw"]["ms_per_step"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--train-steps", type=int, default=10)
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.build()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "steps": args.steps, "param_sets": {}}
    for name, ctor in PARAM_SETS.items():
        res["param_sets"][name] = bench_param_set(name, ctor, args, dev)
    if not args.no_train_step:
        res["train_step_headline"] = bench_train_step(args, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
