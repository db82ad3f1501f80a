"""Inference modes of UNet_Nested on the GPU box: the eval forward against ``infer`` cut at every head, the one-kernel
ensemble mean against its composition, and the HIP-graph forms at batch 1.

Geometries: the headline (fp32 storage, base 32, 1 -> 4 channels, 256x256) and ``bench.py --dtype bf16``'s (bf16
storage, 512x512), each at batch 1, 8 and 32.  Per (geometry, batch) every variant is warmed up, then all variants
alternate in one process, round after round, until each has at least ``--window`` seconds (default 0.5) of device-event
time; the full forward is timed at the start AND at the end of every round, and the difference between the two is the
run's own spread.  Next to each time: the algorithmic GFLOP per image of the nodes the variant runs
(``engine.needed_nodes`` over the per-node counts of SURVEY.md section 8a, recomputed here from the shapes).

The ensemble kernel is also timed by itself at the headline batch (3 x [32, 256, 256, 32] features -> [32, 4, 256, 256]):
its algorithmic bytes over its time, against the HBM peak of MI355X_MICROARCH.md, labelled as that.

    python tools/bench_infer.py [--out profiles/infer/bench_infer_mi355x.json] [--window 0.5] [--batches 1,8,32]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

HBM_PEAK_SPEC_TBS = 8.0        # MI355X_MICROARCH.md: HBM3E peak bandwidth (spec)
HBM_COPY_MEASURED_TBS = 6.29   # same table: float4 copy, measured

GEOMETRIES = [
    ("headline f32 256x256", dict(dtype="f32", size=256, feature_scale=1, depth=4, in_channels=1, n_classes=4)),
    ("bf16 512x512", dict(dtype="bf16", size=512, feature_scale=1, depth=4, in_channels=1, n_classes=4)),
]


def node_gflop(filters, in_channels, i, j, size):
    """forward GFLOP per image of node X_ij (two 3x3 convolutions, plus the 2x2 transposed convolution of a decoder node)"""
    px = (size >> i) ** 2
    f = filters[i]
    if j == 0:
        cin = in_channels if i == 0 else filters[i - 1]
        return 2.0 * 9 * (cin * f + f * f) * px / 1e9
    return (2.0 * filters[i + 1] * f * px + 2.0 * 9 * ((j + 1) * f * f + f * f) * px) / 1e9


def variant_gflop(model, size, head, n_heads):
    from unet_nested4tiny_objects_keypoints_amd.engine import needed_nodes
    nodes = sum(node_gflop(model.filters, model.in_channels, i, j, size) for (i, j) in needed_nodes(model.depth, head))
    return nodes + n_heads * 2.0 * model.filters[0] * model.n_classes * size * size / 1e9


class Variant:
    def __init__(self, name, fn, gflop):
        self.name, self.fn, self.gflop = name, fn, gflop
        self.pairs, self.calls, self.inner = [], 0, 1

    def chunk(self):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(self.inner):
            self.fn()
        e.record()
        self.pairs.append((s, e, self.inner))

    def drain(self):
        """-> per-call milliseconds of the chunks recorded since the last drain (after a synchronise)"""
        out = [s.elapsed_time(e) / n for s, e, n in self.pairs]
        self.pairs = []
        return out


def run_case(label, cfg, batch, window_s, dev):
    from unet_nested4tiny_objects_keypoints_amd import GraphedForward, UNet_Nested
    torch.manual_seed(0)
    m = UNet_Nested(in_channels=cfg["in_channels"], n_classes=cfg["n_classes"], feature_scale=cfg["feature_scale"],
                    depth=cfg["depth"]).to(dev).eval()
    if cfg["dtype"] == "bf16":
        m.set_activation_dtype(torch.bfloat16)
    size, d = cfg["size"], cfg["depth"]
    x = torch.randn(batch, cfg["in_channels"], size, size, device=dev)
    full_gflop = variant_gflop(m, size, d - 1, d - 1)

    def full():
        with torch.no_grad():
            return m(x)

    def composition():
        with torch.no_grad():
            return sum(m(x)) / (d - 1)

    first = Variant("model(x) [start of round]", full, full_gflop)
    variants = [first]
    for head in range(1, d):
        variants.append(Variant("infer(head=%d)" % head, lambda head=head: m.infer(x, head), variant_gflop(m, size, head, 1)))
    variants.append(Variant("infer(head=%d, ensemble=True)" % (d - 1), lambda: m.infer(x, d - 1, ensemble=True), full_gflop))
    variants.append(Variant("sum(model(x)) / %d" % (d - 1), composition, full_gflop))
    if batch == 1:
        gf, g1 = GraphedForward(m, x), GraphedForward(m, x, head=1)
        variants.append(Variant("GraphedForward(model)", lambda: gf(x), full_gflop))
        variants.append(Variant("GraphedForward(model, head=1)", lambda: g1(x), variant_gflop(m, size, 1, 1)))
    last = Variant("model(x) [end of round]", full, full_gflop)
    variants.append(last)
    # warm-up of every shape and variant, and a calibration: chunks of about 20 ms
    for v in variants:
        for _ in range(3):
            v.fn()
    torch.cuda.synchronize()
    for v in variants:
        v.chunk()
    torch.cuda.synchronize()
    for v in variants:
        ms = v.drain()[0]
        v.inner = max(1, min(64, int(20.0 / max(ms, 1e-3))))
    total = {v.name: [] for v in variants}
    rounds = 0
    while rounds < 5 or min(sum(t) * v.inner for v, t in ((v, total[v.name]) for v in variants)) < window_s * 1e3:
        for v in variants:
            v.chunk()
        torch.cuda.synchronize()
        for v in variants:
            total[v.name] += v.drain()
        rounds += 1
        if rounds >= 400:
            break
    rows = []
    for v in variants:
        t = sorted(total[v.name])
        med = t[len(t) // 2]
        rows.append({"variant": v.name, "ms_per_call_median": med, "ms_per_call_min": t[0], "ms_per_call_max": t[-1],
                     "ms_per_image": med / batch, "images_per_s": batch / med * 1e3, "gflop_per_image_algorithmic": v.gflop,
                     "tflops_algorithmic": v.gflop * batch / med, "calls": len(t) * v.inner,
                     "window_s": sum(t) * v.inner / 1e3})
    a, b = rows[0]["ms_per_call_median"], rows[-1]["ms_per_call_median"]
    base = 0.5 * (a + b)
    # the run's own spread: the distance between the two placements of the same full forward, or the 10 % .. 90 % range of
    # its samples over the rounds (both placements pooled), whichever is larger
    pooled = sorted(total[first.name] + total[last.name])
    spread = max(abs(a - b), pooled[(9 * len(pooled)) // 10] - pooled[len(pooled) // 10])
    for r in rows:
        r["time_ratio_to_full"] = r["ms_per_call_median"] / base
        r["gflop_share_of_full"] = r["gflop_per_image_algorithmic"] / full_gflop
    out = {"geometry": label, "batch": batch, "rounds": rounds, "full_ms_median_of_both_placements": base,
           "spread_ms": spread, "spread_ms_between_placements": abs(a - b), "variants": rows}
    print("== %s, batch %d (%d rounds; full forward %.3f ms, spread %.3f ms)" % (label, batch, rounds, base, spread))
    for r in rows:
        print("  %-34s %9.3f ms  %7.3f ms/img  %6.2f GFLOP/img (share %.2f)  time ratio %.2f" % (
            r["variant"], r["ms_per_call_median"], r["ms_per_image"], r["gflop_per_image_algorithmic"],
            r["gflop_share_of_full"], r["time_ratio_to_full"]))
    sys.stdout.flush()
    del m, x
    torch.cuda.empty_cache()
    return out


def run_kernel(dev, window_s, dtype=torch.float32, batch=32, size=256, c=32, n_cls=4, heads=3):
    """the ensemble kernel by itself against its composition ``sum(heads) / n`` on the head kernels"""
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    g = torch.Generator(device=dev).manual_seed(1)
    xs = [torch.randn(batch, size, size, c, device=dev, generator=g).to(dtype) for _ in range(heads)]
    ws = [torch.randn(n_cls, c, device=dev, generator=g) * 0.2 for _ in range(heads)]
    bs = [torch.randn(n_cls, device=dev, generator=g) * 0.5 for _ in range(heads)]
    out = torch.empty(batch, n_cls, size, size, device=dev)
    outs = [torch.empty_like(out) for _ in range(heads)]

    def one():
        ops.heads_mean_fwd(xs, ws, bs, out)

    def comp():
        for x, w, b, o in zip(xs, ws, bs, outs):
            ops.head_fwd(x, w, b, 0.0, 0, None, o)
        return sum(outs) / heads

    one()
    name = _lib.lib().unetpp_last_kernel_name().decode()
    res = {}
    for label, fn in (("heads_mean_fwd", one), ("3 x head_fwd + sum / 3", comp)):
        v = Variant(label, fn, 0.0)
        for _ in range(3):
            fn()
        v.inner = 20
        times = []
        while len(times) < 5 or sum(times) * v.inner < window_s * 1e3:
            v.chunk()
            torch.cuda.synchronize()
            times += v.drain()
        times.sort()
        res[label] = times[len(times) // 2]
    in_bytes = sum(x.numel() * x.element_size() for x in xs)
    alg = in_bytes + out.numel() * 4
    # head maps written; Python's sum() starts with 0 + o_1 (1 read, 1 write), then heads - 1 adds (2 reads, 1 write), then / n
    comp_bytes = in_bytes + (heads + 2 + 3 * (heads - 1) + 2) * out.numel() * 4
    tbs = alg / (res["heads_mean_fwd"] * 1e-3) / 1e12
    r = {"kernel": name, "storage": str(dtype).replace("torch.", ""), "shape": [batch, size, size, c], "classes": n_cls,
         "heads": heads, "ms": res["heads_mean_fwd"], "algorithmic_bytes": alg,
         "achieved_algorithmic_TB_per_s": tbs,
         "share_of_hbm_peak_spec_8.0_TB_per_s": tbs / HBM_PEAK_SPEC_TBS,
         "share_of_measured_copy_rate_6.29_TB_per_s": tbs / HBM_COPY_MEASURED_TBS,
         "composition_ms": res["3 x head_fwd + sum / 3"], "composition_algorithmic_bytes": comp_bytes,
         "composition_launches": 2 * heads + 1, "speedup_over_composition": res["3 x head_fwd + sum / 3"] / res["heads_mean_fwd"]}
    print("== ensemble kernel %s (%s): %.3f ms, %.2f TB/s algorithmic = %.2f of the 8.0 TB/s HBM peak (spec); composition "
          "%.3f ms" % (name, r["storage"], r["ms"], tbs, r["share_of_hbm_peak_spec_8.0_TB_per_s"], r["composition_ms"]))
    sys.stdout.flush()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "infer", "bench_infer_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per variant (at least)")
    ap.add_argument("--batches", default="1,8,32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_infer.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
              "timing": "HIP events on the launching stream around chunks of calls; all variants of a case alternate in "
                        "one process; median over the rounds",
              "cases": [], "ensemble_kernel": []}
    for label, cfg in GEOMETRIES:
        for batch in [int(b) for b in args.batches.split(",")]:
            result["cases"].append(run_case(label, cfg, batch, args.window, dev))
    result["ensemble_kernel"].append(run_kernel(dev, args.window, torch.float32))
    result["ensemble_kernel"].append(run_kernel(dev, args.window, torch.bfloat16))
    # the conditions the timings are read against
    checks = []
    for c in result["cases"]:
        v = {r["variant"]: r for r in c["variants"]}
        d = 4
        full, spread = c["full_ms_median_of_both_placements"], c["spread_ms"]
        checks.append({"geometry": c["geometry"], "batch": c["batch"],
                       "infer_last_head_within_spread_of_full": v["infer(head=%d)" % (d - 1)]["ms_per_call_median"] <= full + spread,
                       "every_earlier_head_faster_than_full": all(v["infer(head=%d)" % h]["ms_per_call_median"] < full
                                                                  for h in range(1, d - 1)),
                       "ensemble_not_slower_than_composition":
                           v["infer(head=%d, ensemble=True)" % (d - 1)]["ms_per_call_median"]
                           <= v["sum(model(x)) / %d" % (d - 1)]["ms_per_call_median"]})
    result["checks"] = checks
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out, "checks": checks}))


if __name__ == "__main__":
    main()
