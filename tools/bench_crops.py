"""Training batches from large scenes on the GPU box: ``SceneCrops.batch`` against its torch composition, and the target
kernel by itself against the plain write of its output.

Workload: four 4096x4096 uint8 frames with 2000 labels each (uniform positions, 4 classes), batch 32, crop 256x256,
default ``Augment`` (flips and quarter turns), radius 3.  Contenders, warmed up, then alternating in one process round
after round until each has at least ``--window`` seconds (default 0.5) of device-event time; medians over the rounds:

  (a) ``crops.batch(32)``: draw, warp, targets -- three launches;
  (b) the torch composition of the same batch from windows drawn beforehand: per sample a slice, flips and a quarter
      turn, and per sample and class ``exp(-0.5 * cdist(pixels, labels).min() / radius)`` in float32;
  (c) ``unetpp_points_target`` alone on the rows of one draw;
  (d) ``out.zero_()`` on the same [32, 4, 256, 256] tensor: one plain write of (c)'s bytes, its floor.

(c) is then repeated with the first 1, 250 .. 2000 labels of every frame and with 8000 (the list tiled four times): one
label is the kernel without its label walk (launch, one sqrt and one exp per element in float64, the stores), and the
rest show where the walk begins to count.

    python tools/bench_crops.py [--out profiles/crops/bench_crops_mi355x.json] [--window 0.5]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

S, SIDE, LABELS, CLASSES, BATCH, CROP, RADIUS = 4, 4096, 2000, 4, 32, 256, 3.0


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
    """-> {name: sorted per-call milliseconds}: every variant warmed up, chunks of about 20 ms, all alternating"""
    for v in variants:
        for _ in range(3):
            v.fn()
    torch.cuda.synchronize()
    for v in variants:
        v.chunk()
    torch.cuda.synchronize()
    for v in variants:
        v.inner = max(1, min(4096, int(20.0 / max(v.drain()[0], 1e-3))))
    total = {v.name: [] for v in variants}
    rounds = 0
    while rounds < 5 or min(sum(total[v.name]) * v.inner for v in variants) < window_s * 1e3:
        for v in variants:
            v.chunk()
        torch.cuda.synchronize()
        for v in variants:
            total[v.name] += v.drain()
        rounds += 1
        if rounds >= 400:
            break
    return {k: sorted(t) for k, t in total.items()}, rounds


def torch_composition(frames, labels, classes, index, origin, rows, pixels):
    """the batch by torch ops from windows already drawn: index / origin / rows are host lists"""
    inputs, targets = [], []
    for f, (ox, oy), row in zip(index, origin, rows):
        w = frames[f, oy:oy + CROP, ox:ox + CROP, 0].float() * (1.0 / 255.0)
        # the forward matrix is D Q^q = [[dx qc, -dx qs], [dy qs, dy qc]]; (dx, dy, q) and (-dx, -dy, q + 2) are the same
        # map, so take dy = 1: a quarter turn count and a flip in x
        qc, qs = round(row[10]), round(row[9])
        q = {(1, 0): 0, (0, 1): 1, (-1, 0): 2, (0, -1): 3}[(qc, qs)]
        w = torch.rot90(w, -q, dims=(0, 1))
        if round(row[6]) * qc - round(row[7]) * qs < 0:
            w = torch.flip(w, dims=(1,))
        inputs.append(w)
        xy = labels[f]
        fwd = torch.tensor([[row[6], row[7]], [row[9], row[10]]], device=xy.device)
        pos = xy @ fwd.t() + torch.tensor([row[8], row[11]], device=xy.device)
        maps = [torch.exp(-0.5 * torch.cdist(pixels, pos[classes[f] == c]).min(dim=1).values / RADIUS).view(CROP, CROP)
                for c in range(CLASSES)]
        targets.append(torch.stack(maps))
    return torch.stack(inputs).unsqueeze(1), torch.stack(targets)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "crops", "bench_crops_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_crops.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import SceneCrops, _lib, ops
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (S, SIDE, SIDE, 1), dtype=torch.uint8, generator=g).to(dev)
    labels = (torch.rand(S, LABELS, 2, generator=g) * (SIDE - 1)).to(dev)
    classes = torch.randint(0, CLASSES, (S, LABELS), dtype=torch.int32, generator=g).to(dev)
    crops = SceneCrops(frames, labels, classes, CLASSES, crop=(CROP, CROP), radius=RADIUS, seed=1)
    _, target, _, _ = crops.batch(BATCH)
    rows, index, origin = crops.last
    h_rows, h_index, h_origin = rows.cpu().tolist(), index.cpu().tolist(), origin.cpu().tolist()
    ys, xs = torch.meshgrid(torch.arange(CROP, device=dev), torch.arange(CROP, device=dev), indexing="ij")
    pixels = torch.stack([xs.reshape(-1), ys.reshape(-1)], dim=1).float()
    # the composition is the same batch: its windows bit for bit, its targets to float32 rounding of the distances
    c_in, c_t = torch_composition(frames, labels, classes, h_index, h_origin, h_rows, pixels)
    fixed_in = ops.warp_batch(frames, index, rows, (CROP, CROP), crops.mul, crops.add, 0.0)
    agree = {"inputs_equal": bool(torch.equal(c_in, fixed_in)),
             "targets_max_abs_difference": float((c_t - target).abs().max())}
    out = torch.empty_like(target)

    def target_with(n_labels):
        reps = -(-n_labels // LABELS)
        lab = labels.repeat(1, reps, 1)[:, :n_labels].contiguous()
        cls = classes.repeat(1, reps)[:, :n_labels].contiguous()
        return lambda: ops.points_target(lab, cls, index, rows, CLASSES, (CROP, CROP), RADIUS, out=out)

    contenders = [
        Variant("(a) crops.batch(32)", lambda: crops.batch(BATCH)),
        Variant("(b) torch composition", lambda: torch_composition(frames, labels, classes, h_index, h_origin, h_rows, pixels)),
        Variant("(c) points_target", target_with(LABELS)),
        Variant("(d) out.zero_()", lambda: out.zero_()),
    ]
    times, rounds = alternate(contenders, args.window)
    med = {k: t[len(t) // 2] for k, t in times.items()}
    sweep_l = [1, 250, 500, 1000, 2000, 8000]
    sweep, _ = alternate([Variant("L = %d" % n, target_with(n)) for n in sweep_l] + [Variant("zero_", lambda: out.zero_())],
                         args.window / 2)
    nbytes = out.numel() * 4
    result = {
        "device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
        "timing": "HIP events on the launching stream around chunks of calls; all contenders alternate in one process; "
                  "median over the rounds",
        "workload": {"frames": [S, SIDE, SIDE, 1], "labels_per_frame": LABELS, "classes": CLASSES, "batch": BATCH,
                     "crop": [CROP, CROP], "radius": RADIUS},
        "rounds": rounds, "composition_agrees": agree,
        "contenders": [{"name": k, "ms_median": med[k], "ms_min": t[0], "ms_max": t[-1], "samples": len(t)}
                       for k, t in times.items()],
        "target_bytes": nbytes,
        "points_target_TB_per_s": nbytes / (med["(c) points_target"] * 1e-3) / 1e12,
        "zero_TB_per_s": nbytes / (med["(d) out.zero_()"] * 1e-3) / 1e12,
        "ratio_c_over_d": med["(c) points_target"] / med["(d) out.zero_()"],
        "ratio_b_over_a": med["(b) torch composition"] / med["(a) crops.batch(32)"],
        "label_sweep_ms_median": {k: t[len(t) // 2] for k, t in sweep.items()},
    }
    for r in result["contenders"]:
        print("  %-26s %9.4f ms  (min %.4f, max %.4f, %d samples)" % (r["name"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                     r["samples"]))
    print("  (c) / (d) = %.2f   (b) / (a) = %.1f   sweep %s" % (result["ratio_c_over_d"], result["ratio_b_over_a"],
                                                               json.dumps(result["label_sweep_ms_median"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out, "ratio_c_over_d": result["ratio_c_over_d"], "composition_agrees": agree}))


if __name__ == "__main__":
    main()
