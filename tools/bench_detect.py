"""Detection on the GPU box: the streaming peak pass against a torch composition of the same rule and against one plain
read of the same maps, and the matcher at 2000 predictions x 2000 labels per group.

Maps: float32 [1, 4, 4096, 4096] (256 MB) of seeded sparse blobs of the project's target shape, about 2000 per map.
Contenders, alternating in one process round after round (the method of tools/bench_infer.py: HIP events on the
launching stream around chunks of calls, medians over the rounds; the first contender runs at the start AND at the end
of every round, and the distance between its two placements is the run's own spread):

  (a) unetpp_peaks_detect (threshold 0.5, radius 2, refinement on, capacity 4096)
  (b) the torch composition of the rule without the tie-break: max_pool2d(2r+1, stride 1), ==, >=, nonzero, gather
      (nonzero reads a count back: this one synchronises)
  (c) maps.sum(): one plain read of the same bytes, the floor
  (d) unetpp_detect_match, 4 groups of 2000 predictions x 2000 labels (serial in the predictions by construction)

    python tools/bench_detect.py [--out profiles/detect/bench_detect_mi355x.json] [--window 0.5]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_COPY_MEASURED_TBS = 6.29   # float4 copy, measured

S, C, SIDE, BLOBS, THRESHOLD, RADIUS, CAP = 1, 4, 4096, 2000, 0.5, 2, 4096
MATCH_N = 2000


def sparse_blob_maps(dev, seed=0):
    """[S, C, SIDE, SIDE]: zero but for BLOBS patches of exp(-0.5 * dist / 3) per map at seeded sub-pixel centres"""
    g = torch.Generator().manual_seed(seed)
    maps = torch.zeros(S, C, SIDE, SIDE, device=dev)
    k = 12
    oy, ox = torch.meshgrid(torch.arange(-k, k + 1, dtype=torch.float64), torch.arange(-k, k + 1, dtype=torch.float64),
                            indexing="ij")
    oy, ox = oy.reshape(1, -1), ox.reshape(1, -1)
    for s in range(S):
        for c in range(C):
            centres = k + 1 + torch.rand(BLOBS, 2, generator=g, dtype=torch.float64) * (SIDE - 2 * k - 3)
            base = centres.round()
            frac = centres - base
            d = torch.sqrt((ox - frac[:, :1]) ** 2 + (oy - frac[:, 1:]) ** 2)
            patch = torch.exp(-0.5 * d / 3.0).float().to(dev)                                  # [BLOBS, (2k+1)^2]
            yy = (base[:, 1:].long() + oy.long()).to(dev)
            xx = (base[:, :1].long() + ox.long()).to(dev)
            flat = maps[s, c].view(-1)
            flat.scatter_reduce_(0, (yy * SIDE + xx).view(-1), patch.view(-1), reduce="amax")
    return maps


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "detect", "bench_detect_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_detect.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib, ops
    maps = sparse_blob_maps(dev)
    flat = maps.view(S * C, SIDE, SIDE)

    def detect():
        return ops.peaks_detect(flat, THRESHOLD, RADIUS, CAP, True)

    def composition():
        pooled = F.max_pool2d(maps, 2 * RADIUS + 1, stride=1, padding=RADIUS)   # pads with -inf: the clipped window
        idx = ((maps == pooled) & (maps >= THRESHOLD)).nonzero()
        return idx, maps[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]

    def floor():
        return maps.sum()

    g = torch.Generator(device=dev).manual_seed(1)
    pxy = torch.rand(1, C, MATCH_N, 2, device=dev, generator=g) * SIDE
    labels = (pxy + torch.randn(1, C, MATCH_N, 2, device=dev, generator=g)).reshape(1, C * MATCH_N, 2).contiguous()
    cls = torch.arange(C, device=dev, dtype=torch.int32).repeat_interleave(MATCH_N).view(1, -1).contiguous()
    n_pred = torch.full((1, C), MATCH_N, dtype=torch.int32, device=dev)
    order = torch.stack([torch.randperm(MATCH_N, device=dev, generator=g) for _ in range(C)]).view(1, C, MATCH_N).int()

    def match():
        return ops.detect_match(pxy, n_pred, order, labels, cls, 3.0)

    xy, score, count = detect()
    idx, _ = composition()
    stats = match()[2]
    torch.cuda.synchronize()
    first, last = Contender("(a) unetpp_peaks_detect [start of round]", detect), Contender("(a) unetpp_peaks_detect [end of round]", detect)
    contenders = [first, Contender("(b) max_pool2d, ==, >=, nonzero, gather", composition),
                  Contender("(c) maps.sum()", floor), Contender("(d) unetpp_detect_match", match), last]
    for v in contenders:
        for _ in range(3):
            v.fn()
    torch.cuda.synchronize()
    for v in contenders:
        v.chunk()
    torch.cuda.synchronize()
    for v in contenders:
        v.inner = max(1, min(64, int(20.0 / max(v.drain()[0], 1e-3))))
    total = {v.name: [] for v in contenders}
    rounds = 0
    while rounds < 5 or min(sum(total[v.name]) * v.inner for v in contenders) < args.window * 1e3:
        for v in contenders:
            v.chunk()
        torch.cuda.synchronize()
        for v in contenders:
            total[v.name] += v.drain()
        rounds += 1
        if rounds >= 400:
            break
    med = {}
    rows = []
    for v in contenders:
        t = sorted(total[v.name])
        med[v.name] = t[len(t) // 2]
        rows.append({"contender": v.name, "ms_median": t[len(t) // 2], "ms_min": t[0], "ms_max": t[-1],
                     "calls": len(t) * v.inner})
    a = 0.5 * (med[first.name] + med[last.name])
    pooled = sorted(total[first.name] + total[last.name])
    spread = max(abs(med[first.name] - med[last.name]), pooled[(9 * len(pooled)) // 10] - pooled[len(pooled) // 10])
    b, c, d = med[contenders[1].name], med[contenders[2].name], med[contenders[3].name]
    nbytes = maps.numel() * 4
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
              "timing": "HIP events on the launching stream around chunks of calls; the contenders alternate in one "
                        "process; median over the rounds",
              "maps": [S, C, SIDE, SIDE], "map_bytes": nbytes, "blobs_per_map": BLOBS, "threshold": THRESHOLD,
              "radius": RADIUS, "cap": CAP, "peaks_per_map": count.tolist(), "composition_peaks": int(idx.shape[0]),
              "match": {"groups": C, "predictions_per_group": MATCH_N, "labels_per_group": MATCH_N,
                        "stats_tp_fp_fn": stats.view(-1, 3).tolist()},
              "rounds": rounds, "contenders": rows, "detect_ms_median_of_both_placements": a, "spread_ms": spread,
              "detect_over_plain_read": a / c, "detect_over_composition": a / b,
              "detect_read_TB_per_s": nbytes / (a * 1e-3) / 1e12,
              "plain_read_TB_per_s": nbytes / (c * 1e-3) / 1e12,
              "plain_read_share_of_measured_copy_rate_6.29_TB_per_s": nbytes / (c * 1e-3) / 1e12 / HBM_COPY_MEASURED_TBS,
              "match_us_per_prediction": d * 1e3 / MATCH_N,
              "checks": {"detect_within_twice_the_plain_read": a <= 2.0 * c, "detect_beats_composition": a < b}}
    for r in rows:
        print("  %-46s %9.3f ms  (min %.3f, max %.3f, %d calls)" % (r["contender"], r["ms_median"], r["ms_min"],
                                                                    r["ms_max"], r["calls"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out, "detect_ms": a, "spread_ms": spread, "plain_read_ms": c, "composition_ms": b,
                      "match_ms": d, "checks": result["checks"]}))


if __name__ == "__main__":
    main()
