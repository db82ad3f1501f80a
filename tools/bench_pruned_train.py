"""Training the network cut at a head on the GPU box: the train step at heads 1, 2 and depth - 1 against ``train_step`` of
the whole network in the same process, and the backward of the ensemble mean against three ``unetpp_head_bwd`` calls.

Geometry: the headline workload of bench.py -- UNet_Nested(in_channels=1, n_classes=4, feature_scale=1), depth 4, base
width 32, 256x256, batch 32, fp32 storage, fused Adam -- one model and one optimizer per contender (a cut's optimizer is
built over ``pruned_parameters``).  The contenders alternate in one process round after round (the method of
tools/bench_detect.py: HIP events on the launching stream around chunks of calls, medians over the rounds; the first
contender runs at the start AND at the end of every round, and the distance between its two placements is the run's own
spread).

  (a) train_step(model, ...)                      the whole network
  (b) train_step(model, ..., head=1)              X_00, X_10, X_01 and final_1
  (c) train_step(model, ..., head=2)
  (d) train_step(model, ..., head=depth - 1)      the full cut: the launches of (a)
  (e) ops.heads_mean_bwd, 3 heads at [32, 256, 256, 32], n_cls 4 (the mean's backward: no `out` read, C * n_cls more FMAs
      per pixel for the recomputed logits)
  (f) three ops.head_bwd calls at that shape (p_drop 0)

The derived expectation for (b) / (a) and (c) / (a) is the forward FLOP share of the cut (README: 0.20 and 0.51) plus the
per-launch floor; the ratios are recorded, no pass/fail number is set on them.

    python tools/bench_pruned_train.py [--out profiles/pruned_train/bench_pruned_train_mi355x.json] [--window 1.0]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

CTOR = dict(in_channels=1, n_classes=4, feature_scale=1)
BATCH, SIZE = 32, 256
HEAD_SHAPE, HEAD_CLS, HEADS = (32, 256, 256, 32), 4, 3
README_FORWARD_FLOP_SHARE = {1: 0.20, 2: 0.51}


class Contender:
    def __init__(self, name, fn):
        self.name, self.fn, self.pairs, self.inner = name, fn, [], 1

    def chunk(self):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(self.inner):
            self.fn()
        e.record()
        self.pairs.append((s, e, self.inner))

    def drain(self):
        out = [s.elapsed_time(e) / n for s, e, n in self.pairs]
        self.pairs = []
        return out


def step_contender(name, dev, head, x, target):
    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet_Nested, pruned_parameters, train_step
    torch.manual_seed(0)
    model = UNet_Nested(**CTOR).to(dev).train()
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    params = list(model.parameters()) if head is None else pruned_parameters(model, head)
    opt = torch.optim.Adam(params, lr=1e-3, fused=True)
    c = Contender(name, lambda: train_step(model, opt, crit, x, target, head=head))
    c.parameters = sum(p.numel() for p in params)
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "pruned_train", "bench_pruned_train_mi355x.json"))
    ap.add_argument("--window", type=float, default=1.0, help="device-event seconds per contender (at least)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_pruned_train.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    depth = 4
    torch.manual_seed(1000)
    x = torch.randn(BATCH, CTOR["in_channels"], SIZE, SIZE, device=dev)
    target = torch.rand(BATCH, CTOR["n_classes"], SIZE, SIZE, device=dev)
    first = step_contender("(a) train_step, whole network [start of round]", dev, None, x, target)
    last = step_contender("(a) train_step, whole network [end of round]", dev, None, x, target)
    cuts = {h: step_contender("(%s) train_step(head=%d)" % ("bcd"[h - 1], h), dev, h, x, target) for h in range(1, depth)}

    g = torch.Generator(device=dev).manual_seed(2)
    n, hh, ww, c = HEAD_SHAPE
    xs = [torch.randn(HEAD_SHAPE, generator=g, device=dev).relu_() for _ in range(HEADS)]
    wts = [torch.randn(HEAD_CLS, c, generator=g, device=dev) * (2.0 / c) ** 0.5 for _ in range(HEADS)]
    bs = [torch.randn(HEAD_CLS, generator=g, device=dev) * 0.5 for _ in range(HEADS)]
    d_out = torch.randn(n, HEAD_CLS, hh, ww, generator=g, device=dev)
    outs = [torch.empty(n, HEAD_CLS, hh, ww, device=dev) for _ in range(HEADS)]
    for xh, wt, b, o in zip(xs, wts, bs, outs):
        ops.head_fwd(xh, wt, b, 0.0, 0, None, o)
    dxs = [torch.empty_like(xh) for xh in xs]

    def mean_bwd():
        return ops.heads_mean_bwd(xs, wts, bs, d_out, dxs, [False] * HEADS, [True] * HEADS)

    def three_bwd():
        return [ops.head_bwd(d_out, o, xh, wt, 0.0, 0, None, dx, False, gate_x=True)
                for o, xh, wt, dx in zip(outs, xs, wts, dxs)]

    mean_bwd()
    mean_kernel = _lib.lib().unetpp_last_kernel_name().decode()
    three_bwd()
    single_kernel = _lib.lib().unetpp_last_kernel_name().decode()
    k_first, k_last = Contender("(e) heads_mean_bwd, 3 heads [start of round]", mean_bwd), Contender("(e) heads_mean_bwd, 3 heads [end of round]", mean_bwd)
    k_three = Contender("(f) 3 x head_bwd", three_bwd)

    contenders = [first] + [cuts[h] for h in sorted(cuts)] + [k_first, k_three, k_last, last]
    for v in contenders:
        for _ in range(12 if v.fn not in (mean_bwd, three_bwd) else 5):   # allocator growth, code objects, weight-image plans
            v.fn()
    torch.cuda.synchronize()
    for v in contenders:
        v.chunk()
    torch.cuda.synchronize()
    for v in contenders:
        v.inner = max(1, min(64, int(40.0 / max(v.drain()[0], 1e-3))))
    total = {v.name: [] for v in contenders}
    rounds = 0
    while rounds < 5 or min(sum(total[v.name]) * v.inner for v in contenders) < args.window * 1e3:
        for v in contenders:
            v.chunk()
        torch.cuda.synchronize()
        for v in contenders:
            total[v.name] += v.drain()
        rounds += 1
        if rounds >= 200:
            break
    med, rows = {}, []
    for v in contenders:
        t = sorted(total[v.name])
        med[v.name] = t[len(t) // 2]
        rows.append({"contender": v.name, "ms_median": t[len(t) // 2], "ms_min": t[0], "ms_max": t[-1], "calls": len(t) * v.inner})

    def both(a, b):
        pooled = sorted(total[a.name] + total[b.name])
        spread = max(abs(med[a.name] - med[b.name]), pooled[(9 * len(pooled)) // 10] - pooled[len(pooled) // 10])
        return 0.5 * (med[a.name] + med[b.name]), spread

    whole, spread = both(first, last)
    mean_ms, mean_spread = both(k_first, k_last)
    three = sorted(total[k_three.name])
    three_ms, three_spread = med[k_three.name], three[(9 * len(three)) // 10] - three[len(three) // 10]
    pixels = n * hh * ww
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
              "timing": "HIP events on the launching stream around chunks of calls; the contenders alternate in one process; "
                        "median over the rounds; at least 5 rounds",
              "workload": "UNet_Nested(in=1,n_classes=4,base=32,depth=4) 256x256 train step, batch 32, fp32 storage, fused Adam",
              "rounds": rounds, "contenders": rows,
              "whole_step_ms_median_of_both_placements": whole, "whole_step_spread_ms": spread,
              "cut_steps": {str(h): {"ms": med[cuts[h].name], "ratio_to_whole_step": med[cuts[h].name] / whole,
                                     "parameters": cuts[h].parameters,
                                     "readme_forward_flop_share": README_FORWARD_FLOP_SHARE.get(h, 1.0)}
                            for h in sorted(cuts)},
              "heads_mean_bwd": {"shape_nhwc": list(HEAD_SHAPE), "n_cls": HEAD_CLS, "heads": HEADS, "kernel": mean_kernel,
                                 "ms_median_of_both_placements": mean_ms, "spread_ms": mean_spread,
                                 "three_head_bwd_kernel": single_kernel, "three_head_bwd_ms": three_ms,
                                 "three_head_bwd_spread_ms": three_spread, "ratio_to_three_head_bwd": mean_ms / three_ms,
                                 "slower_than_three_calls_by_more_than_their_spread": mean_ms > three_ms + three_spread,
                                 # x read + dx written per head, d_out read per head (one launch per head); no `out` read
                                 "algorithmic_bytes": HEADS * pixels * 4 * (2 * c + HEAD_CLS),
                                 "algorithmic_TB_per_s": HEADS * pixels * 4 * (2 * c + HEAD_CLS) / (mean_ms * 1e-3) / 1e12,
                                 "three_head_bwd_algorithmic_bytes": HEADS * pixels * 4 * (2 * c + 2 * HEAD_CLS)}}
    for r in rows:
        print("  %-52s %9.3f ms  (min %.3f, max %.3f, %d calls)" % (r["contender"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                    r["calls"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out, "whole_step_ms": whole, "spread_ms": spread,
                      "cut_ratios": {h: v["ratio_to_whole_step"] for h, v in result["cut_steps"].items()},
                      "heads_mean_bwd_ms": mean_ms, "three_head_bwd_ms": three_ms}))


if __name__ == "__main__":
    main()
