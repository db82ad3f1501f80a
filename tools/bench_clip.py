"""Time gradient clipping inside the fused optimizer step against what a user did before it existed.

    python tools/bench_clip.py [--reps 7] [--steps 200] [--out profiles/clip/bench_clip_mi355x.json]

Parts (each runs in a child process of its own under a time limit; a part that fails or overruns ends the run, nothing
more is started on the GPU after it):
  headline   UNet_Nested(1, 4, feature_scale=1): 2 207 244 parameters
  configs4   depth 5, base 64 (in 3, 5 maps): 36 167 124 parameters
Contenders, all in the same process, alternating inside every repetition; every parameter has a seeded randn gradient
whose global norm is far above max_norm, so clipping is active in every call:
  fused_clip_step             AdamW(max_grad_norm=m).step(): norm launch + clipped update            (a)
  torch_clip_then_fused_step  torch.nn.utils.clip_grad_norm_(params, m), then the unclipped step()   (b) the baseline
  fused_step                  the unclipped AdamW.step() alone                                       (c)
  fused_clip_step_capturable  (a) with capturable=True, skip_nonfinite=True (no per-step host -> device copy)
  fused_step_capturable       (c) with capturable=True
  clip_fn_then_fused_step     the package's clip_grad_norm_(params, m_k), then the unclipped step(); m_k shrinks by
                              0.1 % per call so that the in-place scale really writes every time
Per contender and repetition: `steps` calls between two HIP events (device ms per call: the stream's time from the first
launch to the last, host-induced gaps included) and the host wall time of the calls (the queue drained before and
after); after a warm-up, medians over the repetitions.  Bytes are the algorithm's: every element of every stream read
or written once (AdamW: p, g, m, v read, p, m, v written; the norm pass reads g once more).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_average import PARAM_SETS, alternate, launches_of  # noqa: E402

PARTS = {"headline": 300, "configs4": 300}   # part -> its time limit in seconds
DEFAULT_OUT = os.path.join(ROOT, "profiles", "clip", "bench_clip_mi355x.json")
MAX_NORM = 1.0


def part(name, args):
    import torch

    from unet_nested4tiny_objects_keypoints_amd import AdamW, UNet_Nested, clip_grad_norm_
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in UNet_Nested(**PARAM_SETS[name]).parameters()]
    n_param = sum(int(torch.Size(s).numel()) for s in shapes)

    def make(**kw):
        """every contender its own parameters and gradients: none sees what another did to them"""
        g = torch.Generator(device=dev).manual_seed(1)
        params = [torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.05) for s in shapes]
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=g)
        return params, AdamW(params, lr=1e-6, weight_decay=1e-4, **kw)

    pa, a = make(max_grad_norm=MAX_NORM)
    pb, b = make()
    pc, c = make()
    pac, ac = make(max_grad_norm=MAX_NORM, capturable=True, skip_nonfinite=True)
    pcc, cc = make(capturable=True)
    pd, d = make()
    shrink = {"m": 1.0e3}

    def torch_clip_then_step():
        torch.nn.utils.clip_grad_norm_(pb, MAX_NORM)
        b.step()

    def clip_fn_then_step():
        shrink["m"] *= 0.999
        clip_grad_norm_(pd, shrink["m"])
        d.step()

    contenders = {
        "fused_clip_step": a.step,
        "torch_clip_then_fused_step": torch_clip_then_step,
        "fused_step": c.step,
        "fused_clip_step_capturable": ac.step,
        "fused_step_capturable": cc.step,
        "clip_fn_then_fused_step": clip_fn_then_step,
    }
    res = alternate(contenders, args.reps, args.steps)
    for k, fn in contenders.items():
        res[k]["launches_per_call"] = launches_of(fn)
    step_bytes, norm_bytes = 28 * n_param, 4 * n_param
    for k, bts in (("fused_clip_step", step_bytes + norm_bytes), ("fused_step", step_bytes),
                   ("fused_clip_step_capturable", step_bytes + norm_bytes), ("fused_step_capturable", step_bytes),
                   ("torch_clip_then_fused_step", step_bytes + norm_bytes + 8 * n_param),
                   ("clip_fn_then_fused_step", step_bytes + norm_bytes + 8 * n_param)):
        res[k]["bytes_per_call"] = bts
        res[k]["GBps"] = bts / (res[k]["device_ms_per_call"] * 1e-3) / 1e9
    torch.cuda.synchronize()
    dms = {k: v["device_ms_per_call"] for k, v in res.items()}
    return {"tensors": len(shapes), "params": n_param, "max_norm": MAX_NORM,
            "grad_norm_seen": float(a.last_grad_norm), "skipped_steps": int(ac.skipped_steps), "contenders": res,
            "fused_clip_minus_fused_step_us": 1e3 * (dms["fused_clip_step"] - dms["fused_step"]),
            "fused_clip_capturable_minus_fused_step_capturable_us":
                1e3 * (dms["fused_clip_step_capturable"] - dms["fused_step_capturable"]),
            "torch_clip_then_fused_step_over_fused_clip_step": dms["torch_clip_then_fused_step"] / dms["fused_clip_step"]}


def run_part(name, args):
    import torch

    import __graft_entry__ as entry
    entry.build()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip: no GPU (this tool measures on the device only)")
    res = part(name, args)
    res["device"] = torch.cuda.get_device_name(0)
    with open(args.part_out, "w") as f:
        json.dump(res, f)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--part", default=None, help=argparse.SUPPRESS)        # child mode
    ap.add_argument("--part-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part is not None:
        run_part(args.part, args)
        return
    res = {"reps": args.reps, "steps": args.steps, "parts": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.parts.split(","):
            if name not in PARTS:
                raise SystemExit("unknown part %r (known: %s)" % (name, ", ".join(PARTS)))
            out = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(PARTS[name]), sys.executable, os.path.abspath(__file__), "--part", name,
                   "--part-out", out, "--reps", str(args.reps), "--steps", str(args.steps)]
            print("bench_clip:", name, flush=True)
            status = subprocess.run(cmd).returncode
            if status != 0:      # a fault, an abort or the time limit: nothing more is started on the GPU
                raise SystemExit("bench_clip: part %s ended with status %d; stopping" % (name, status))
            with open(out) as f:
                res["parts"][name] = json.load(f)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
