"""The one-pass backward of a frozen BatchNorm layer against the training-mode trio, on the GPU box.

Per geometry, on the same tensors and in one process, alternating round after round until every variant has at least
``--window`` seconds (default 0.5) of device-event time:

    trio            ops.bn_backward: reduce, finalize, apply (unchanged) -- timed at the start AND at the end of a round;
                    the distance between the two placements (or the 10 % .. 90 % range of their pooled samples, whichever
                    is larger) is the run's own spread
    frozen+sums     ops.bn_frozen_backward: one streaming launch plus the finalize of dgamma / dbeta
    frozen          the same without sums (gamma and beta frozen too): one launch

Geometries: the four BatchNorm shapes of the headline (fp32, batch 32, 256x256, base 32), each with and without the pooled
consumer's gradient routed inside the pass, and levels 0 and 1 of ``bench.py --dtype bf16`` (batch 8, 512x512) in bf16.
All out of place (the engine runs them in place: the same bytes).  Next to each time: the algorithmic bytes (every operand
read or written once per pass that touches it) over the time, against the 6.29 TB/s float4-copy rate of
MI355X_MICROARCH.md.  Last, informational (they compute different things): one whole ``train_step`` of the headline
with every BatchNorm frozen against the unfrozen one, alternating in the same run.

    python tools/bench_bn_frozen.py [--out profiles/bn_frozen/bench_bn_frozen_mi355x.json] [--window 0.5] [--no-step]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

HBM_COPY_MEASURED_TBS = 6.29   # MI355X_MICROARCH.md: float4 copy, measured

GEOMETRIES = [   # (label, dtype, N, H, W, C)
    ("headline level 0", "f32", 32, 256, 256, 32), ("headline level 1", "f32", 32, 128, 128, 64),
    ("headline level 2", "f32", 32, 64, 64, 128), ("headline level 3", "f32", 32, 32, 32, 256),
    ("bf16 512x512 level 0", "bf16", 8, 512, 512, 32), ("bf16 512x512 level 1", "bf16", 8, 256, 256, 64),
]


class Variant:
    def __init__(self, name, fn, nbytes=0.0):
        self.name, self.fn, self.nbytes = name, fn, nbytes
        self.pairs, self.inner = [], 1

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


def alternate(variants, window_s, chunk_ms=10.0):
    """Warm up, size the chunks, then round after round until every variant has window_s of device time.
    -> {name: sorted per-call ms of its chunks}, rounds"""
    for v in variants:
        for _ in range(3):
            v.fn()
    torch.cuda.synchronize()
    for v in variants:
        v.chunk()
    torch.cuda.synchronize()
    for v in variants:
        v.inner = max(1, min(256, int(chunk_ms / max(v.drain()[0], 1e-3))))
    total = {v.name: [] for v in variants}
    rounds = 0
    while rounds < 5 or min(sum(total[v.name]) * v.inner for v in variants) < window_s * 1e3:
        for v in variants:
            v.chunk()
        torch.cuda.synchronize()
        for v in variants:
            total[v.name] += v.drain()
        rounds += 1
        if rounds >= 2000:
            break
    return {k: sorted(t) for k, t in total.items()}, rounds


def spread_of(total, first, last):
    a, b = total[first][len(total[first]) // 2], total[last][len(total[last]) // 2]
    pooled = sorted(total[first] + total[last])
    return 0.5 * (a + b), max(abs(a - b), pooled[(9 * len(pooled)) // 10] - pooled[len(pooled) // 10])


def run_geometry(label, dtype, n, h, w, c, pool, window_s, dev):
    from unet_nested4tiny_objects_keypoints_amd import ops
    adt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator(device="cpu").manual_seed(7)
    y = (torch.randn(n, h, w, c, device=dev) * 1.5 + 0.2).to(adt)
    d_act = torch.randn(n, h, w, c, device=dev).to(adt)
    dy = torch.empty_like(d_act)
    rm, rv = 0.5 * torch.randn(c, generator=g), 0.5 + 1.5 * torch.rand(c, generator=g)
    gamma, beta = (1 + 0.1 * torch.randn(c, generator=g)).to(dev), (0.1 * torch.randn(c, generator=g)).to(dev)
    mean, invstd, scale, shift = ops.bn_eval_coeffs_stats(gamma, beta, rm.to(dev), rv.to(dev), 1e-5)
    dg, db = torch.empty(c, device=dev), torch.empty(c, device=dev)
    pg = None
    if pool:
        pg = (torch.randn(n, h // 2, w // 2, c, device=dev).to(adt),
              torch.randint(0, 4, (n, h // 2, w // 2, c), device=dev, dtype=torch.uint8))
    es = 2.0 if dtype == "bf16" else 4.0
    tensor = es * n * h * w * c
    routed = (es + 1.0) * n * h * w * c / 4 if pool else 0.0   # d_pooled and the winner bytes, per pass that reads d_act
    trio_bytes, frozen_bytes = 5 * tensor + 2 * routed, 3 * tensor + routed

    def trio():
        ops.bn_backward(d_act, y, scale, shift, mean, invstd, gamma, dy, dg, db, pool=pg)

    def frozen_sums():
        ops.bn_frozen_backward(d_act, y, scale, shift, mean, invstd, dy, dg, db, pool=pg)

    def frozen():
        ops.bn_frozen_backward(d_act, y, scale, shift, None, None, dy, pool=pg, want_sums=False)

    variants = [Variant("trio [start of round]", trio, trio_bytes), Variant("frozen+sums", frozen_sums, frozen_bytes),
                Variant("frozen", frozen, frozen_bytes), Variant("trio [end of round]", trio, trio_bytes)]
    total, rounds = alternate(variants, window_s)
    base, spread = spread_of(total, variants[0].name, variants[-1].name)
    rows = []
    for v in variants:
        t = total[v.name]
        med = t[len(t) // 2]
        rows.append({"variant": v.name, "ms_median": med, "ms_min": t[0], "ms_max": t[-1], "calls": len(t) * v.inner,
                     "window_s": sum(t) * v.inner / 1e3, "algorithmic_bytes": v.nbytes,
                     "algorithmic_tb_per_s": v.nbytes / med / 1e9,
                     "share_of_float4_copy_rate": v.nbytes / med / 1e9 / HBM_COPY_MEASURED_TBS,
                     "time_ratio_to_trio": med / base})
    worst = max(r["ms_median"] for r in rows[1:3])
    return {"geometry": label, "dtype": dtype, "shape_nhwc": [n, h, w, c], "pool_routing": bool(pool), "rounds": rounds,
            "trio_ms_median_of_both_placements": base, "spread_ms": spread,
            "frozen_not_slower_than_trio_beyond_spread": bool(worst <= base + spread), "variants": rows}


def run_step(window_s, dev):
    """train_step of the headline (fp32, base 32, 1 -> 4 channels, 256x256, batch 32, Adam, dropout on), every BatchNorm in
    training mode against every BatchNorm frozen (gamma and beta too); two models with the same initial state."""
    import copy

    from unet_nested4tiny_objects_keypoints_amd import FocalLoss_BCE_2d, UNet_Nested, train_step
    torch.manual_seed(0)
    a = UNet_Nested(in_channels=1, n_classes=4, feature_scale=1).to(dev).train()
    b = copy.deepcopy(a).train().freeze_batchnorm()
    x, t = torch.randn(32, 1, 256, 256, device=dev), torch.rand(32, 4, 256, 256, device=dev)
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)

    def opt(m):
        return torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    oa, ob = opt(a), opt(b)
    variants = [Variant("train_step [start of round]", lambda: train_step(a, oa, crit, x, t)),
                Variant("train_step, BatchNorm frozen", lambda: train_step(b, ob, crit, x, t)),
                Variant("train_step [end of round]", lambda: train_step(a, oa, crit, x, t))]
    total, rounds = alternate(variants, window_s, chunk_ms=60.0)
    base, spread = spread_of(total, variants[0].name, variants[-1].name)
    rows = [{"variant": v.name, "ms_median": total[v.name][len(total[v.name]) // 2], "ms_min": total[v.name][0],
             "ms_max": total[v.name][-1], "calls": len(total[v.name]) * v.inner} for v in variants]
    return {"geometry": "headline train_step, batch 32, 256x256, fp32 (informational: the two compute different things)",
            "rounds": rounds, "unfrozen_ms_median_of_both_placements": base, "spread_ms": spread, "variants": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join("profiles", "bn_frozen", "bench_bn_frozen_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bn_frozen.py needs a GPU: a timing taken anywhere else says nothing")
    from unet_nested4tiny_objects_keypoints_amd import _lib
    dev = torch.device("cuda:0")
    cases = []
    for label, dtype, n, h, w, c in GEOMETRIES:
        for pool in (False, True):
            r = run_geometry(label, dtype, n, h, w, c, pool, args.window, dev)
            cases.append(r)
            print("%-22s %-5s pool=%d  trio %.4f ms (spread %.4f)  frozen+sums %.4f  frozen %.4f  ratio %.2f / %.2f  %s" % (
                label, dtype, pool, r["trio_ms_median_of_both_placements"], r["spread_ms"], r["variants"][1]["ms_median"],
                r["variants"][2]["ms_median"], r["variants"][1]["time_ratio_to_trio"], r["variants"][2]["time_ratio_to_trio"],
                "ok" if r["frozen_not_slower_than_trio_beyond_spread"] else "SLOWER"), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
           "timing": "HIP events on the launching stream around chunks of calls; all variants of a case alternate in one "
                     "process; median over the chunks",
           "hbm_float4_copy_tb_per_s": HBM_COPY_MEASURED_TBS, "cases": cases}
    if not args.no_step:
        out["train_step"] = run_step(args.window, dev)
        print(json.dumps(out["train_step"]["variants"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
