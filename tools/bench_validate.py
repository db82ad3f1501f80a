"""Time one validation batch: validate_step against the per-head composition a user writes without it.

    python tools/bench_validate.py [--batches 32 1] [--reps 10] [--warmup 3] [--out profiles/validate/bench.json]

Headline geometry: UNet_Nested(in_channels=1, n_classes=4, feature_scale=1) (base width 32, depth 4, fp32), 256x256,
pattern [[0], [1, 2, 3], [4], [5, 6]] over 7 labels per image, seeded random weights and inputs, threshold 0.5.
Contenders, per batch size:
  validate_step  eval forward + one head-loss launch + one extraction over the stacked heads + one matcher launch;
  composed       eval forward + per head: criterion, transfer_points, greedy min-distance matching on the host
                 (NumPy, the same rule), torch.nn.MSELoss over the matched coordinates (trainer/trainer.py:209-223);
  forward        the eval forward alone, to give its share of each path.
Where the time goes after the forward, on the same batch:
  extract_stacked / extract_per_head   ops.keypoints_extract over the stacked heads / once per head, on the network's
                 heads (random weights: thresholded noise, large irregular regions, long convergence loops);
  outputs_validate / outputs_composed  everything after the forward (validate_outputs / the composition) on target-like
                 heads: create_heatmap of the labels shifted by (0, 0), (1, -2), (-3, 1) px, compact blobs as a trained
                 network's heads.
Every timed call starts and ends on a drained queue; HIP events around it give milliseconds per batch.  Contenders
alternate inside each repetition; medians over the repetitions are reported.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PATTERN = [[0], [1, 2, 3], [4], [5, 6]]


def host_match(points, found, labels, pattern):
    """points [N, C, K, 2], found [N, C], labels [N, S, 2] (NumPy) -> matched [N, S, 2], mask [N, S]: greedy global
    minimum of the squared distance, ties by label position then prediction index"""
    n_img, s = labels.shape[:2]
    matched = np.full((n_img, s, 2), -1.0, np.float32)
    mask = np.zeros((n_img, s), bool)
    for n in range(n_img):
        for c, labs in enumerate(pattern):
            p = int(found[n, c])
            if p == 0:
                continue
            d = ((points[n, c, None, :p, :] - labels[n, labs, None, :]).astype(np.float64) ** 2).sum(-1)
            for _ in range(min(len(labs), p)):
                i, j = np.unravel_index(int(np.argmin(d)), d.shape)
                matched[n, labs[i]] = points[n, c, j]
                mask[n, labs[i]] = True
                d[i, :] = np.inf
                d[:, j] = np.inf
    return matched, mask


def composed(model, crit, hm, x, labels, threshold):
    with torch.no_grad():
        return composed_outputs(model(x), crit, hm, labels, threshold)


def composed_outputs(outputs, crit, hm, labels, threshold):
    with torch.no_grad():
        target = hm.create_heatmap(labels)
        lab = labels.cpu().numpy()
        heat, land = [], []
        for o in outputs:
            heat.append(crit(o, target))
            points, found = hm.transfer_points(o, labels, threshold)
            matched, mask = host_match(points.cpu().numpy(), found.cpu().numpy(), lab, PATTERN)
            m = torch.from_numpy(mask).to(labels.device)
            land.append(torch.nn.MSELoss()(torch.from_numpy(matched).to(labels.device)[m], labels[m]))
    return heat, land


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_validate needs a GPU")
    from unet_nested4tiny_objects_keypoints_amd import (FocalLoss_BCE_2d, Heatmap, UNet_Nested, ops, validate_outputs,
                                                        validate_step)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = UNet_Nested(in_channels=1, n_classes=4, feature_scale=1).to(dev).eval()
    crit = FocalLoss_BCE_2d(gamma=3, size_average=False)
    hm = Heatmap(PATTERN, args.size, args.size)
    result = dict(device=torch.cuda.get_device_name(0), size=args.size, pattern=PATTERN, reps=args.reps,
                  warmup=args.warmup, threshold=args.threshold, batches={})
    for b in args.batches:
        g = torch.Generator().manual_seed(b)
        x = torch.randn(b, 1, args.size, args.size, generator=g).to(dev)
        labels = (torch.rand(b, 7, 2, generator=g) * (args.size - 32) + 16).to(dev)
        with torch.no_grad():
            heads = model(x)
        hw = (args.size, args.size)
        synthetic = tuple(hm.create_heatmap(labels + torch.tensor(sh, dtype=torch.float32, device=dev))
                          for sh in ((0, 0), (1, -2), (-3, 1)))
        runs = {
            "validate_step": lambda: validate_step(model, crit, hm, x, labels, threshold=args.threshold),
            "composed": lambda: composed(model, crit, hm, x, labels, args.threshold),
            "forward": lambda: model(x),
            "extract_stacked": lambda: ops.keypoints_extract(torch.stack(heads).view(-1, *hw), 3, args.threshold),
            "extract_per_head": lambda: [ops.keypoints_extract(o.reshape(-1, *hw), 3, args.threshold) for o in heads],
            "outputs_validate": lambda: validate_outputs(synthetic, crit, hm, labels, threshold=args.threshold),
            "outputs_composed": lambda: composed_outputs(synthetic, crit, hm, labels, args.threshold),
        }
        with torch.no_grad():
            for _ in range(args.warmup):
                for fn in runs.values():
                    fn()
            times = {k: [] for k in runs}
            for _ in range(args.reps):
                for k, fn in runs.items():
                    times[k].append(timed(fn))
        res = validate_step(model, crit, hm, x, labels, threshold=args.threshold)
        heat, land = composed(model, crit, hm, x, labels, args.threshold)
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {"ms_" + k: round(v, 4) for k, v in med.items()}
        row.update({"ms_%s_all" % k: [round(t, 4) for t in v] for k, v in times.items()})
        row["forward_share_validate_step"] = round(med["forward"] / med["validate_step"], 4)
        row["forward_share_composed"] = round(med["forward"] / med["composed"], 4)
        row["matched_count"] = res.matched_count.tolist()
        row["landmark_losses"] = res.landmark_losses.tolist()
        row["landmark_losses_composed"] = [float(v) for v in land]
        row["heatmap_losses_equal"] = bool(torch.equal(res.heatmap_losses, torch.stack(heat)))
        result["batches"][str(b)] = row
        row["matched_count_synthetic"] = validate_outputs(synthetic, crit, hm, labels).matched_count.tolist()
        print("batch %d: validate_step %.3f ms, composed %.3f ms, eval forward %.3f ms (%.0f%% / %.0f%%); extraction "
              "stacked %.3f ms, per head %.3f ms; after the forward on target-like heads: validate_outputs %.3f ms, "
              "composed %.3f ms" % (
                  b, med["validate_step"], med["composed"], med["forward"], 100 * row["forward_share_validate_step"],
                  100 * row["forward_share_composed"], med["extract_stacked"], med["extract_per_head"],
                  med["outputs_validate"], med["outputs_composed"]), flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
