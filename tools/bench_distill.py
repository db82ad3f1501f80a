"""Self-distillation across the heads on the GPU box: the fused call against the composition of the existing entry
points and against the plain focal heads call.

Workload: 3 heads of [32, 4, 256, 256] (the head shape of the headline training step), a random target, weight 0.5,
teacher "last", gamma 3.  Contenders, warmed up, then alternating in one process round after round until each has at
least ``--window`` seconds (default 0.5) of device-event time; medians over the rounds:

  (a) ``ops.distill_heads``: S_j, D_j, L_j, the mean over heads and the gradients to every head -- two launches;
  (b) the composition: ``ops.focal_bce_heads``, ``ops.focal_bce(p_j, p_3)`` for the two students, and the float32 tensor
      arithmetic that joins them (per student a scale, a product with w and an add; the loss values on 0-dim tensors);
  (c) ``ops.focal_bce_heads`` on the same tensors: it reads every head and the target once and writes every gradient
      once -- the same bytes as (a), half its logarithms per student element, hence the floor;
  (d) (a) with gate "teacher_better" and the ignore rule on a target with 10 % ignored elements.

(a) closes every round as well as opening it: the distance between its two medians is the spread of the measurement.
Byte model, in map-sized float32 streams at three heads: (a) and (c) move 7 (the target, three heads, three gradients);
(b) moves 7 in focal_bce_heads, 2 x 3 in the focal_bce calls and 2 x (2 + 2 + 3) in the six elementwise launches = 27 if
nothing stays in a cache, about 23 with the product and the add reading what was just written.  (a) / (c) near 1 says the
pass stays bound by bytes; clearly above 1, that the second logf per student element is what it waits for.

    python tools/bench_distill.py [--out profiles/distill/bench_distill_mi355x.json] [--window 0.5]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.bench_crops import Variant, alternate  # noqa: E402

HEADS, SHAPE, GAMMA, WEIGHT, IGNORED = 3, (32, 4, 256, 256), 3.0, 0.5, 0.10
STREAMS_FUSED, STREAMS_COMPOSITION = 2 * HEADS + 1, 23


def composition(preds, target, rows, w32):
    """the loss with existing calls -> (avg, [grad]): one focal_bce_heads, a focal_bce per student, six elementwise
    launches on maps and a few on 0-dim tensors"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    heads = len(preds)
    inv_heads = 1.0 / heads
    plain, grads = ops.focal_bce_heads(preds, target, rows, GAMMA)
    avg = 0
    for j in range(heads - 1):
        d, gd = ops.focal_bce(preds[j], preds[heads - 1], rows, GAMMA)
        grads[j] = grads[j] + w32 * (gd * inv_heads)
        avg = avg + (plain[1 + j] + w32 * d)
    avg = 1.0 * (avg + plain[heads]) / heads
    return avg, grads


def measure(preds, target, ignored_target, rows, weight_dev, window):
    from unet_nested4tiny_objects_keypoints_amd import ops
    fused = lambda: ops.distill_heads(preds, target, rows, GAMMA, weight_dev)  # noqa: E731
    contenders = [
        Variant("(a) distill_heads", fused),
        Variant("(b) composition", lambda: composition(preds, target, rows, WEIGHT)),
        Variant("(c) focal_bce_heads", lambda: ops.focal_bce_heads(preds, target, rows, GAMMA)),
        Variant("(d) distill_heads, gate and ignore", lambda: ops.distill_heads(
            preds, ignored_target, rows, GAMMA, weight_dev, gate="teacher_better", ignore=True)),
        Variant("(a) again, closing the round", fused),
    ]
    times, rounds = alternate(contenders, window)
    med = {name: t[len(t) // 2] for name, t in times.items()}
    a, a2 = med["(a) distill_heads"], med["(a) again, closing the round"]
    return {
        "rounds": rounds,
        "contenders": [{"name": name, "ms_median": med[name], "ms_min": t[0], "ms_max": t[-1], "samples": len(t)}
                       for name, t in times.items()],
        "spread_of_a": abs(a - a2) / min(a, a2),
        "ratio_a_over_c": a / med["(c) focal_bce_heads"],
        "ratio_b_over_a": med["(b) composition"] / a,
        "ratio_d_over_a": med["(d) distill_heads, gate and ignore"] / a,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "distill", "bench_distill_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_distill.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    rows = SHAPE[0] * SHAPE[1]
    g = torch.Generator().manual_seed(0)
    target = torch.rand(SHAPE, generator=g)
    ignored_target = target.clone()
    ignored_target[torch.rand(SHAPE, generator=g) < IGNORED] = -1.0
    target, ignored_target = target.to(dev), ignored_target.to(dev)
    preds = [(torch.rand(SHAPE, generator=g) * 0.98 + 0.01).to(dev) for _ in range(HEADS)]
    weight_dev = torch.full((1,), WEIGHT, dtype=torch.float32, device=dev)
    loss, grads, sup, dis = ops.distill_heads(preds, target, rows, GAMMA, weight_dev)
    c_loss, c_grads = composition(preds, target, rows, WEIGHT)
    agree = {"loss_bits_equal": bool(torch.equal(loss[0].view(torch.int32), c_loss.view(torch.int32))),
             "loss_relative_difference": float((c_loss - loss[0]).abs() / loss[0].abs()),
             "gradient_bits_equal": all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
                                        for a, b in zip(grads, c_grads))}
    timing = measure(preds, target, ignored_target, rows, weight_dev, args.window)
    med = {r["name"]: r["ms_median"] for r in timing["contenders"]}
    map_bytes = target.numel() * 4
    a, c = med["(a) distill_heads"], med["(c) focal_bce_heads"]
    margin = max(0.05, 2.0 * timing["spread_of_a"])
    result = {
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
        "timing": "HIP events on the launching stream around chunks of calls; all contenders alternate in one process; "
                  "median over the rounds; (a) opens and closes every round",
        "workload": {"heads": HEADS, "shape": list(SHAPE), "gamma": GAMMA, "weight": WEIGHT, "teacher": "last",
                     "rows": rows, "ignored_share_of_d": IGNORED},
        "composition_agrees": agree,
        "measured": timing,
        "ms_fused": a, "ms_composition": med["(b) composition"], "ms_plain": c,
        "byte_model": {"map_bytes": map_bytes, "streams_fused": STREAMS_FUSED, "streams_plain": STREAMS_FUSED,
                       "streams_composition": STREAMS_COMPOSITION,
                       "ratio_b_over_a_predicted": STREAMS_COMPOSITION / STREAMS_FUSED, "ratio_a_over_c_predicted": 1.0},
        "bytes_per_second_fused": STREAMS_FUSED * map_bytes / (a * 1e-3),
        "bytes_per_second_plain": STREAMS_FUSED * map_bytes / (c * 1e-3),
        "fused_faster_than_composition": med["(b) composition"] > a,
        "ratio_to_plain": timing["ratio_a_over_c"],
        "bound_by": "bytes" if timing["ratio_a_over_c"] <= 1.0 + margin else "arithmetic: the second logf per student element",
        "bound_by_margin": margin,
    }
    for r in timing["contenders"]:
        print("  %-38s %9.4f ms  (min %.4f, max %.4f, %d samples)" % (r["name"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                     r["samples"]))
    print("  (a) / (c) = %.3f (bytes alone: 1.000)   (b) / (a) = %.2f (bytes alone: %.2f)   spread of (a) %.3f   bound by %s" % (
        timing["ratio_a_over_c"], timing["ratio_b_over_a"], STREAMS_COMPOSITION / STREAMS_FUSED, timing["spread_of_a"],
        result["bound_by"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out, "composition_agrees": agree, "fused_faster_than_composition":
                      result["fused_faster_than_composition"]}))
    if not result["fused_faster_than_composition"]:
        raise SystemExit("the fused call is not faster than the composition")


if __name__ == "__main__":
    main()
