"""Penalty-reduced focal loss on the GPU box: the fused heads call against its torch composition and against the plain
focal heads call.

Workload: 3 heads of [32, 4, 256, 256] (the head shape of the headline training step), a target with 0.1 % positives
(exactly 1.0) and random values below 1 elsewhere, alpha 2, beta 4, eps 1e-4, positive 1.0.
Contenders, warmed up, then alternating in one process round after round until each has at least ``--window`` seconds
(default 0.5) of device-event time; medians over the rounds:

  (a) ``ops.pr_focal_heads``: the count pass, value, mean over heads and the gradients to every head -- three launches;
  (b) the torch composition of the rule with autograd backward to the heads (``clamp``, ``pow``, ``log``, ``log1p``,
      ``where``, ``sum``, the count, the mean over heads, ``backward()``);
  (c) ``ops.focal_bce_heads`` on the same tensors: it reads every head and the target once and writes every gradient
      once -- the same bytes except for the count pass's second read of the target, hence the floor.

(a) closes every round as well as opening it: the distance between its two medians is the spread of the measurement.
Expectation from the bytes moved: (a) / (c) = (2 heads + 2) / (2 heads + 1) = 8 / 7 at three heads, plus one launch.

    python tools/bench_prfocal.py [--out profiles/prfocal/bench_prfocal_mi355x.json] [--window 0.5]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.bench_crops import Variant, alternate  # noqa: E402

HEADS, SHAPE, POSITIVES = 3, (32, 4, 256, 256), 0.001
ALPHA, BETA, EPS, POSITIVE, GAMMA = 2.0, 4.0, 1e-4, 1.0, 3.0


def torch_composition(preds, target):
    """the loop body of the trainer with the rule written in torch ops -> (avg, [grad])"""
    lo = float(torch.tensor(EPS, dtype=torch.float32))
    hi = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(EPS, dtype=torch.float32))
    leaves = [p.detach().requires_grad_(True) for p in preds]
    avg = 0
    for p in leaves:
        q = p.clamp(lo, hi)
        pos = target >= POSITIVE
        at_centre = -1 * (1 - q) ** ALPHA * torch.log(q)
        elsewhere = -1 * (1 - target) ** BETA * q ** ALPHA * torch.log1p(-q)
        total = torch.where(pos, at_centre, elsewhere).sum()
        avg = avg + total * (1.0 / pos.sum().clamp(min=1).to(total.dtype))
    avg = 1.0 * avg / len(leaves)
    avg.backward()
    return avg.detach(), [p.grad for p in leaves]


def measure(preds, target, rows, window):
    from unet_nested4tiny_objects_keypoints_amd import ops
    fused = lambda: ops.pr_focal_heads(preds, target, ALPHA, BETA, EPS, POSITIVE)  # noqa: E731
    contenders = [
        Variant("(a) pr_focal_heads", fused),
        Variant("(b) torch composition", lambda: torch_composition(preds, target)),
        Variant("(c) focal_bce_heads", lambda: ops.focal_bce_heads(preds, target, rows, GAMMA)),
        Variant("(a) again, closing the round", fused),
    ]
    times, rounds = alternate(contenders, window)
    med = {name: t[len(t) // 2] for name, t in times.items()}
    a, a2 = med["(a) pr_focal_heads"], med["(a) again, closing the round"]
    return {
        "rounds": rounds,
        "contenders": [{"name": name, "ms_median": med[name], "ms_min": t[0], "ms_max": t[-1], "samples": len(t)}
                       for name, t in times.items()],
        "spread_of_a": abs(a - a2) / min(a, a2),
        "ratio_a_over_c": a / med["(c) focal_bce_heads"],
        "ratio_b_over_a": med["(b) torch composition"] / a,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "prfocal", "bench_prfocal_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_prfocal.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    rows = SHAPE[0] * SHAPE[1]
    g = torch.Generator().manual_seed(0)
    target = torch.rand(SHAPE, generator=g) * 0.999
    target[torch.rand(SHAPE, generator=g) < POSITIVES] = 1.0
    target = target.to(dev)
    preds = [(torch.rand(SHAPE, generator=g) * 0.98 + 0.01).to(dev) for _ in range(HEADS)]
    loss, grads, n_pos = ops.pr_focal_heads(preds, target, ALPHA, BETA, EPS, POSITIVE)
    c_loss, c_grads = torch_composition(preds, target)
    agree = {"n_pos": int(n_pos), "n_pos_of_the_composition": int((target >= POSITIVE).sum()),
             "loss_relative_difference": float((c_loss - loss[0]).abs() / loss[0].abs()),
             "gradient_max_relative_difference": max(float(((a - b).abs() / b.abs().clamp(min=1e-30)).max())
                                                     for a, b in zip(grads, c_grads))}
    timing = measure(preds, target, rows, args.window)
    expected = (2 * HEADS + 2) / (2 * HEADS + 1)
    result = {
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
        "timing": "HIP events on the launching stream around chunks of calls; all contenders alternate in one process; "
                  "median over the rounds; (a) opens and closes every round",
        "workload": {"heads": HEADS, "shape": list(SHAPE), "positives": POSITIVES, "alpha": ALPHA, "beta": BETA, "eps": EPS,
                     "positive": POSITIVE, "gamma_of_c": GAMMA, "rows_of_c": rows},
        "composition_agrees": agree,
        "measured": timing,
        "ratio_a_over_c_expected_from_bytes": expected,
        "ratio_a_over_c_measured": timing["ratio_a_over_c"],
        "excess_over_expected": timing["ratio_a_over_c"] / expected - 1.0,
        "bytes_of_a": (2 * HEADS + 2) * target.numel() * 4,
        "bytes_of_c": (2 * HEADS + 1) * target.numel() * 4,
    }
    for r in timing["contenders"]:
        print("  %-30s %9.4f ms  (min %.4f, max %.4f, %d samples)" % (r["name"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                     r["samples"]))
    print("  (a) / (c) = %.3f (expected from bytes %.3f)   (b) / (a) = %.2f   spread of (a) %.3f" % (
        timing["ratio_a_over_c"], expected, timing["ratio_b_over_a"], timing["spread_of_a"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out, "composition_agrees": agree}))


if __name__ == "__main__":
    main()
