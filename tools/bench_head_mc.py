"""Monte-Carlo dropout at the heads on the GPU box: the fused launch (``unetpp_head_mc``) against its fallback
composition (K ``head_fwd`` launches and the fold in torch elementwise ops), with one plain ``head_fwd`` as the floor --
the cost of reading ``X_0J`` once and writing one map.

Shape ``[32, 256, 256]``, C = 32, 4 classes, K in {4, 8, 16, 32}.  The method of ``tools/bench_infer.py``: per K the
contenders are warmed up and then alternate in one process, round after round, until each has at least ``--window``
seconds of HIP-event time; medians over the rounds; the first contender (the fused launch) is timed at both ends of a
round and the distance between the two placements is the run's own spread.  Also whole ``infer_mc(x, 3, K)`` against
``infer(x, 3)`` on the headline network.  No ratio is asserted: the numbers are the result.

    python tools/bench_head_mc.py [--out profiles/head_mc/bench_head_mc_mi355x.json] [--window 0.5] [--samples 4,8,16,32]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

MIB = float(1 << 20)


class Variant:
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


def alternate(variants, window_s):
    """-> {name: median ms per call}, rounds.  variants[0] and variants[-1] are the two placements of one contender."""
    for v in variants:
        for _ in range(3):
            v.fn()
    torch.cuda.synchronize()
    for v in variants:
        v.chunk()
    torch.cuda.synchronize()
    for v in variants:
        v.inner = max(1, min(64, int(10.0 / max(v.drain()[0], 1e-3))))     # chunks of about 10 ms
    total = {v.name: [] for v in variants}
    rounds = 0
    while rounds < 5 or min(sum(total[v.name]) * v.inner for v in variants) < window_s * 1e3:
        for v in variants:
            v.chunk()
        torch.cuda.synchronize()
        for v in variants:
            total[v.name] += v.drain()
        rounds += 1
        if rounds >= 200:
            break
    return {name: sorted(t)[len(t) // 2] for name, t in total.items()}, rounds


def run_kernels(dev, k, window_s, batch=32, size=256, c=32, n_cls=4, p=0.4):
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(batch, size, size, c, device=dev, generator=g)
    wt = torch.randn(n_cls, c, device=dev, generator=g) * 0.2
    bias = torch.randn(n_cls, device=dev, generator=g) * 0.5
    mean = torch.empty(batch, n_cls, size, size, device=dev)
    var, one = torch.empty_like(mean), torch.empty_like(mean)

    def fused():
        ops.head_mc(x, wt, bias, p, 1, k, mean, var)

    def composition():
        fused_flag, ops._FUSED_HEAD_MC = ops._FUSED_HEAD_MC, False
        try:
            ops.head_mc(x, wt, bias, p, 1, k, mean, var)
        finally:
            ops._FUSED_HEAD_MC = fused_flag

    def floor():
        ops.head_fwd(x, wt, bias, p, 1, None, one)

    fused()
    label = _lib.lib().unetpp_last_kernel_name().decode()
    if not label.startswith("head_mc<"):
        raise SystemExit("the fused launch did not run (%s): nothing to compare" % label)
    med, rounds = alternate([Variant("fused [start of round]", fused), Variant("composition", composition),
                             Variant("head_fwd (floor)", floor), Variant("fused [end of round]", fused)], window_s)
    a, b = med["fused [start of round]"], med["fused [end of round]"]
    ms = 0.5 * (a + b)
    x_mib, map_mib = x.numel() * 4 / MIB, mean.numel() * 4 / MIB
    # composition: K (x read + map written); a copy (2 maps moved) and K - 1 adds (3 each), a division (2), K subtractions
    # (3), K squares (2), K - 1 adds (3), a division (2) -- every operand element read or written once per op
    comp_mib = k * (x_mib + map_mib) + (2 + 3 * (k - 1) + 2 + 3 * k + 2 * k + 3 * (k - 1) + 2) * map_mib
    r = {"samples": k, "kernel": label, "shape": [batch, size, size, c], "classes": n_cls, "p_drop": p, "rounds": rounds,
         "fused_ms": ms, "spread_ms_between_placements": abs(a - b), "composition_ms": med["composition"],
         "head_fwd_floor_ms": med["head_fwd (floor)"], "fused_over_floor": ms / med["head_fwd (floor)"],
         "composition_over_fused": med["composition"] / ms, "fused_ms_per_sample_above_floor": (ms - med["head_fwd (floor)"]) / k,
         "fused_algorithmic_MiB": x_mib + 2 * map_mib, "composition_algorithmic_MiB": comp_mib,
         "fused_algorithmic_TB_per_s": (x_mib + 2 * map_mib) * MIB / (ms * 1e-3) / 1e12}
    print("== K = %2d  %s: fused %.3f ms (spread %.3f), composition %.3f ms (x %.2f), head_fwd floor %.3f ms (fused / floor "
          "%.2f)" % (k, label, ms, abs(a - b), med["composition"], r["composition_over_fused"], med["head_fwd (floor)"],
                     r["fused_over_floor"]))
    sys.stdout.flush()
    return r


def run_model(dev, ks, window_s, batch=32, size=256):
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested
    torch.manual_seed(0)
    m = UNet_Nested(in_channels=1, n_classes=4, feature_scale=1, depth=4).to(dev).eval()
    x = torch.randn(batch, 1, size, size, device=dev)
    variants = [Variant("infer(x, 3) [start of round]", lambda: m.infer(x, 3))]
    variants += [Variant("infer_mc(x, 3, %d)" % k, lambda k=k: m.infer_mc(x, 3, samples=k, seed=1)) for k in ks]
    variants.append(Variant("infer(x, 3) [end of round]", lambda: m.infer(x, 3)))
    med, rounds = alternate(variants, window_s)
    a, b = med["infer(x, 3) [start of round]"], med["infer(x, 3) [end of round]"]
    base = 0.5 * (a + b)
    rows = [{"samples": k, "infer_mc_ms": med["infer_mc(x, 3, %d)" % k], "over_infer": med["infer_mc(x, 3, %d)" % k] / base,
             "ms_above_infer": med["infer_mc(x, 3, %d)" % k] - base} for k in ks]
    print("== headline network, batch %d: infer(x, 3) %.3f ms (spread %.3f); infer_mc %s" % (
        batch, base, abs(a - b), ", ".join("K = %d: %.3f ms" % (r["samples"], r["infer_mc_ms"]) for r in rows)))
    return {"batch": batch, "size": size, "rounds": rounds, "infer_ms": base, "spread_ms_between_placements": abs(a - b),
            "infer_mc": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "head_mc", "bench_head_mc_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    ap.add_argument("--samples", default="4,8,16,32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_head_mc.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib
    ks = [int(k) for k in args.samples.split(",")]
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
              "timing": "HIP events on the launching stream around chunks of calls; the contenders of a case alternate in "
                        "one process; median over the rounds; the fused launch at both ends of a round",
              "kernels": [run_kernels(dev, k, args.window) for k in ks]}
    result["model"] = run_model(dev, ks, args.window)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
