"""Top-k focal loss on the GPU box: the fused heads call against its torch composition and against the plain focal
heads call, on random heads and on saturated ones.

Workload: the head shape of the headline training step -- batch 32, 256x256, the model's ``n_classes`` maps, its
number of deep-supervision heads -- ``fraction = 0.01`` (k = 656 of 65 536 pixels per map), gamma 3, the sum convention.
Contenders, warmed up, then alternating in one process round after round until each has at least ``--window`` seconds
(default 0.5) of device-event time; medians over the rounds:

  (a) ``ops.topk_focal_heads``: selection, value, mean over heads and the gradients to every head -- two launches;
  (b) the torch composition with autograd backward to the heads: per head ``|p - t|``, ``topk`` over the pixel axis,
      ``gather``, the focal formula on the gathered values, the mean over heads, ``backward()`` (its ties fall as
      ``topk`` lets them);
  (c) ``ops.focal_bce_heads`` on the same tensors: one streaming pass over every pixel, the floor.

(a) closes every round as well as opening it: the distance between its two medians is the spread of the measurement.
Second shape: the same with every pred saturated to 0 against a target of 0.25, so that all keys of a row are equal --
one histogram bin takes every element, the worst case for the LDS atomics, and all 656 selected pixels are ties.

    python tools/bench_topk.py [--out profiles/topk/bench_topk_mi355x.json] [--window 0.5]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.bench_crops import Variant, alternate  # noqa: E402

BATCH, SIDE, FRACTION, GAMMA = 32, 256, 0.01, 3.0


def torch_composition(preds, target, k, rows):
    """the loop body of the trainer with a top-k criterion written in torch ops -> (avg, [grad])"""
    leaves = [p.detach().requires_grad_(True) for p in preds]
    avg = 0
    for p in leaves:
        d = (p - target).flatten(2)
        idx = torch.topk(d.detach().abs(), k, dim=2).indices
        err = 1 - torch.gather(d, 2, idx).abs() + 1e-20
        avg = avg + (-1 * (1 - err) ** GAMMA * torch.log(err)).sum() / rows
    avg = 1.0 * avg / len(leaves)
    avg.backward()
    return avg.detach(), [p.grad for p in leaves]


def measure(preds, target, k, rows, window):
    from unet_nested4tiny_objects_keypoints_amd import ops
    contenders = [
        Variant("(a) topk_focal_heads", lambda: ops.topk_focal_heads(preds, target, k, rows, GAMMA)),
        Variant("(b) torch composition", lambda: torch_composition(preds, target, k, rows)),
        Variant("(c) focal_bce_heads", lambda: ops.focal_bce_heads(preds, target, rows, GAMMA)),
        Variant("(a) again, closing the round", lambda: ops.topk_focal_heads(preds, target, k, rows, GAMMA)),
    ]
    times, rounds = alternate(contenders, window)
    med = {name: t[len(t) // 2] for name, t in times.items()}
    a, a2 = med["(a) topk_focal_heads"], med["(a) again, closing the round"]
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
                                                  "profiles", "topk", "bench_topk_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_topk.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, _lib, ops
    model = UNet_Nested()
    classes, heads = model.n_classes, model.depth - 1
    shape = (BATCH, classes, SIDE, SIDE)
    rows, pixels = BATCH * classes, SIDE * SIDE
    k = max(1, math.ceil(FRACTION * pixels))
    g = torch.Generator().manual_seed(0)
    target = torch.rand(shape, generator=g).to(dev)
    preds = [(torch.rand(shape, generator=g) * 0.98 + 0.01).to(dev) for _ in range(heads)]
    # the composition is the same loss: random keys have no ties at the threshold (checked), so the selections agree
    loss, grads, kth = ops.topk_focal_heads(preds, target, k, rows, GAMMA)
    c_loss, c_grads = torch_composition(preds, target, k, rows)
    agree = {"loss_relative_difference": float((c_loss - loss[0]).abs() / loss[0].abs()),
             "selections_equal": all(bool(torch.equal(a != 0, b != 0)) for a, b in zip(grads, c_grads)),
             "gradient_max_abs_difference": max(float((a - b).abs().max()) for a, b in zip(grads, c_grads))}
    random_shape = measure(preds, target, k, rows, args.window)
    flat_target = torch.full(shape, 0.25, device=dev)
    flat_preds = [torch.zeros(shape, device=dev) for _ in range(heads)]
    _, flat_grads, flat_kth = ops.topk_focal_heads(flat_preds, flat_target, k, rows, GAMMA)
    first = (flat_grads[0].flatten(2) != 0)
    flat_ok = bool(first[:, :, :k].all()) and not bool(first[:, :, k:].any()) and bool((flat_kth == 0.25).all())
    equal_shape = measure(flat_preds, flat_target, k, rows, args.window)
    a_rand = random_shape["contenders"][0]["ms_median"]
    a_flat = equal_shape["contenders"][0]["ms_median"]
    result = {
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
        "timing": "HIP events on the launching stream around chunks of calls; all contenders alternate in one process; "
                  "median over the rounds; (a) opens and closes every round",
        "workload": {"heads": heads, "shape": list(shape), "rows": rows, "pixels": pixels, "fraction": FRACTION, "k": k,
                     "gamma": GAMMA, "denom": rows},
        "composition_agrees": agree,
        "random": random_shape,
        "all_equal": dict(equal_shape, first_k_indices_selected=flat_ok),
        "ratio_all_equal_over_random": a_flat / a_rand,
        "bytes_one_pass": (2 * heads + 1) * rows * pixels * 4,
    }
    for name in ("random", "all_equal"):
        print(name)
        for r in result[name]["contenders"]:
            print("  %-30s %9.4f ms  (min %.4f, max %.4f, %d samples)" % (r["name"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                         r["samples"]))
        print("  (a) / (c) = %.2f   (b) / (a) = %.2f   spread of (a) %.3f" % (
            result[name]["ratio_a_over_c"], result[name]["ratio_b_over_a"], result[name]["spread_of_a"]))
    print("  all-equal / random = %.2f" % result["ratio_all_equal_over_random"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out, "composition_agrees": agree, "all_equal_ok": flat_ok}))


if __name__ == "__main__":
    main()
