"""Distillation from an external map on the GPU box: the fused call against the composition of the existing entry
points and against the plain focal heads call, each as a graph replay.

Workload: 3 heads of [32, 4, 256, 256] (the head shape of the headline training step), a random target, a random
teacher map of the same shape, weight 0.5, gamma 3.  Every contender is captured once into a graph of its own and
replayed; the contenders are warmed up, then alternate in one process round after round until each has at least
``--window`` seconds (default 0.5) of device-event time; medians over the rounds:

  (a) ``ops.teacher_heads``: S_h, D_h, L_h, the mean over heads and the gradients to every head -- two launches;
  (b) the composition: ``ops.focal_bce_heads``, ``ops.focal_bce(p_h, q)`` for each of the three heads, and the float32
      tensor arithmetic that joins them (per head a scale, a product with w and an add; the loss values on 0-dim tensors);
  (c) ``ops.focal_bce_heads`` on the same tensors: the floor -- it reads every head and the target once and writes every
      gradient once, 1 + 2 J map-sized streams where (a) moves 2 + 2 J (the teacher's map is the one more), with half of
      (a)'s logarithms per element;
  (d) (a) with gate "teacher_better" and the ignore rule, 10 % of the target ignored and a third of the teacher void.

(a) closes every round as well as opening it: the distance between its two medians is the spread of the measurement.
Byte model, in map-sized float32 streams at three heads: (a) moves 8, (c) moves 7, so bytes alone predict (a) / (c) =
8 / 7; (b) moves 7 in focal_bce_heads, 3 x 3 in the focal_bce calls and 3 x (2 + 2 + 3) in the nine elementwise launches
= 37 if nothing stays in a cache.  (a) / (c) near 8 / 7 says the pass stays bound by bytes; clearly above, that the second
logf per element is what it waits for.  No ratio is asserted beyond (a) being faster than (b).

    python tools/bench_teacher.py [--out profiles/teacher/bench_teacher_mi355x.json] [--window 0.5]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.bench_crops import Variant, alternate  # noqa: E402

HEADS, SHAPE, GAMMA, WEIGHT, IGNORED, VOID = 3, (32, 4, 256, 256), 3.0, 0.5, 0.10, 1.0 / 3.0
STREAMS_FUSED, STREAMS_PLAIN, STREAMS_COMPOSITION = 2 + 2 * HEADS, 1 + 2 * HEADS, (1 + 2 * HEADS) + 3 * HEADS + 7 * HEADS


def composition(preds, target, teacher, rows, w32):
    """the loss with existing calls -> (avg, [grad]): one focal_bce_heads, a focal_bce per head, nine elementwise
    launches on maps and a few on 0-dim tensors"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    heads = len(preds)
    inv_heads = 1.0 / heads
    plain, grads = ops.focal_bce_heads(preds, target, rows, GAMMA)
    avg = 0
    for j in range(heads):
        d, gd = ops.focal_bce(preds[j], teacher, rows, GAMMA)
        grads[j] = grads[j] + w32 * (gd * inv_heads)
        avg = avg + (plain[1 + j] + w32 * d)
    avg = 1.0 * avg / heads
    return avg, grads


def graphed(fn):
    """fn captured into a graph of its own (after a warm-up on a side stream) -> (replay, what the captured call returned)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph.replay, out


def measure(contenders, window):
    times, rounds = alternate([Variant(name, fn) for name, fn in contenders], window)
    med = {name: t[len(t) // 2] for name, t in times.items()}
    a, a2 = med["(a) teacher_heads"], med["(a) again, closing the round"]
    return {
        "rounds": rounds,
        "contenders": [{"name": name, "ms_median": med[name], "ms_min": t[0], "ms_max": t[-1], "samples": len(t)}
                       for name, t in times.items()],
        "spread_of_a": abs(a - a2) / min(a, a2),
        "ratio_a_over_c": a / med["(c) focal_bce_heads"],
        "ratio_b_over_a": med["(b) composition"] / a,
        "ratio_d_over_a": med["(d) teacher_heads, gate, ignore and void"] / a,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "teacher", "bench_teacher_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_teacher.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    rows = SHAPE[0] * SHAPE[1]
    g = torch.Generator().manual_seed(0)
    target = torch.rand(SHAPE, generator=g)
    ignored_target = target.clone()
    ignored_target[torch.rand(SHAPE, generator=g) < IGNORED] = -1.0
    teacher = torch.rand(SHAPE, generator=g)
    void_teacher = teacher.clone()
    void_teacher[torch.rand(SHAPE, generator=g) < VOID] = -1.0
    target, ignored_target, teacher, void_teacher = (t.to(dev) for t in (target, ignored_target, teacher, void_teacher))
    preds = [(torch.rand(SHAPE, generator=g) * 0.98 + 0.01).to(dev) for _ in range(HEADS)]
    weight_dev = torch.full((1,), WEIGHT, dtype=torch.float32, device=dev)

    fused, (loss, grads, sup, dis) = graphed(lambda: ops.teacher_heads(preds, target, teacher, rows, GAMMA, weight_dev))
    comp, (c_loss, c_grads) = graphed(lambda: composition(preds, target, teacher, rows, WEIGHT))
    plain, _ = graphed(lambda: ops.focal_bce_heads(preds, target, rows, GAMMA))
    masked, _ = graphed(lambda: ops.teacher_heads(preds, ignored_target, void_teacher, rows, GAMMA, weight_dev,
                                                  gate="teacher_better", ignore=True))
    fused(), comp()
    torch.cuda.synchronize()
    agree = {"loss_bits_equal": bool(torch.equal(loss[0].view(torch.int32), c_loss.view(torch.int32))),
             "loss_relative_difference": float((c_loss - loss[0]).abs() / loss[0].abs()),
             "gradient_bits_equal": all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
                                        for a, b in zip(grads, c_grads))}
    timing = measure([("(a) teacher_heads", fused), ("(b) composition", comp), ("(c) focal_bce_heads", plain),
                      ("(d) teacher_heads, gate, ignore and void", masked), ("(a) again, closing the round", fused)],
                     args.window)
    med = {r["name"]: r["ms_median"] for r in timing["contenders"]}
    map_bytes = target.numel() * 4
    a, c = med["(a) teacher_heads"], med["(c) focal_bce_heads"]
    predicted = STREAMS_FUSED / STREAMS_PLAIN
    margin = max(0.05, 2.0 * timing["spread_of_a"])
    result = {
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
        "timing": "HIP events on the launching stream around chunks of graph replays, one captured graph per contender; "
                  "all contenders alternate in one process; median over the rounds; (a) opens and closes every round",
        "workload": {"heads": HEADS, "shape": list(SHAPE), "gamma": GAMMA, "weight": WEIGHT, "rows": rows,
                     "ignored_share_of_d": IGNORED, "void_share_of_d": VOID},
        "composition_agrees": agree,
        "measured": timing,
        "ms_fused": a, "ms_composition": med["(b) composition"], "ms_plain": c,
        "byte_model": {"map_bytes": map_bytes, "streams_fused": STREAMS_FUSED, "streams_plain": STREAMS_PLAIN,
                       "streams_composition": STREAMS_COMPOSITION,
                       "ratio_b_over_a_predicted": STREAMS_COMPOSITION / STREAMS_FUSED, "ratio_a_over_c_predicted": predicted},
        "bytes_per_second_fused": STREAMS_FUSED * map_bytes / (a * 1e-3),
        "bytes_per_second_plain": STREAMS_PLAIN * map_bytes / (c * 1e-3),
        "fused_faster_than_composition": med["(b) composition"] > a,
        "ratio_to_plain": timing["ratio_a_over_c"],
        "bound_by": "bytes" if timing["ratio_a_over_c"] <= predicted * (1.0 + margin) else "arithmetic: the second logf per element",
        "bound_by_margin": margin,
    }
    for r in timing["contenders"]:
        print("  %-42s %9.4f ms  (min %.4f, max %.4f, %d samples)" % (r["name"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                     r["samples"]))
    print("  (a) / (c) = %.3f (bytes alone: %.3f)   (b) / (a) = %.2f (bytes alone: %.2f)   spread of (a) %.3f   bound by %s" % (
        timing["ratio_a_over_c"], predicted, timing["ratio_b_over_a"], STREAMS_COMPOSITION / STREAMS_FUSED,
        timing["spread_of_a"], result["bound_by"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out, "composition_agrees": agree, "fused_faster_than_composition":
                      result["fused_faster_than_composition"]}))
    if not result["fused_faster_than_composition"]:
        raise SystemExit("the fused call is not faster than the composition")


if __name__ == "__main__":
    main()
