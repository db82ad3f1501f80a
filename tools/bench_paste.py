"""Copy-paste of tiny objects on the GPU box: what ``SceneCrops(paste=ObjectPaste(...))`` adds to a batch, the three new
launches alone, and a torch composition of the same paste.

Workload: that of tools/bench_crops.py -- four 4096x4096 uint8 frames with 2000 labels each (uniform positions, 4
classes), batch 32, crop 256x256, default ``Augment``, radius 3 -- with ``ObjectPaste(max_pastes=4, p=1.0)`` (R = 4).
Contenders, warmed up, then alternating in one process round after round until each has at least ``--window`` seconds
(default 0.5) of device-event time; medians over the rounds; (a) opens and closes every round, and the distance between
its two medians is the run-to-run spread every other difference is read against:

  (a) ``crops.batch(32)`` without paste: draw, warp, targets -- three launches;
  (b) ``crops.batch(32)`` with paste: six launches;
  (c) ``unetpp_paste_draw`` alone;  (d) ``unetpp_paste_apply`` alone, in place on the batch's inputs;
  (e) ``work.copy_(target)`` then ``unetpp_paste_target`` on work: the merge always meets the frame's own target, as in
      a batch (on its own output it would find nothing left to store);
  (f) ``work.copy_(target)`` alone: one read plus one write of the target, the floor of (e) - (f);
  (g) the torch composition of (d) and (e) from rows read back beforehand: per paste a slice, ``rot90`` / ``flip``, a
      ``where`` over the weights; per window and class ``exp(-0.5 * cdist(pixels, pasted).min() / radius)`` and a
      ``maximum`` that leaves negatives alone.

``--plain-only`` times (a) alone, and ``--root DIR`` takes the package from another checkout (built there): the parent
commit's off path against this commit's, run alternately in one session, each run a process of its own.

    python tools/bench_paste.py [--out profiles/paste/bench_paste_mi355x.json] [--window 0.5] [--plain-only] [--root DIR]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S, SIDE, LABELS, CLASSES, BATCH, CROP, RADIUS = 4, 4096, 2000, 4, 32, 256, 3.0
SLOTS, PATCH = 4, 4


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "paste", "bench_paste_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    ap.add_argument("--plain-only", action="store_true", help="time crops.batch without paste alone")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured (default: this one)")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(1, os.path.join(HERE, "tools"))
    import torch
    from bench_crops import Variant, alternate
    sys.path.insert(0, root)   # (bench_crops puts its own checkout first)
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_paste.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    import unet_nested4tiny_objects_keypoints_amd as pkg
    from unet_nested4tiny_objects_keypoints_amd import SceneCrops, _lib, ops
    assert os.path.abspath(os.path.dirname(os.path.dirname(pkg.__file__))) == root, pkg.__file__
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (S, SIDE, SIDE, 1), dtype=torch.uint8, generator=g).to(dev)
    labels = (torch.rand(S, LABELS, 2, generator=g) * (SIDE - 1)).to(dev)
    classes = torch.randint(0, CLASSES, (S, LABELS), dtype=torch.int32, generator=g).to(dev)

    def make(paste=None):
        kw = {} if paste is None else {"paste": paste}
        return SceneCrops(frames, labels, classes, CLASSES, crop=(CROP, CROP), radius=RADIUS, seed=1, **kw)

    plain = make()
    result = {
        "device": torch.cuda.get_device_name(0), "root": os.path.relpath(root, HERE), "source_hash": _lib.source_hash(),
        "window_s": args.window,
        "timing": "HIP events on the launching stream around chunks of calls; all contenders alternate in one process; "
                  "median over the rounds; the first contender opens and closes every round",
        "workload": {"frames": [S, SIDE, SIDE, 1], "labels_per_frame": LABELS, "classes": CLASSES, "batch": BATCH,
                     "crop": [CROP, CROP], "radius": RADIUS, "max_pastes": SLOTS, "p": 1.0, "patch_radius": PATCH},
    }
    a_name, a_again = "(a) crops.batch(32)", "(a) again, closing the round"
    contenders = [Variant(a_name, lambda: plain.batch(BATCH))]

    if not args.plain_only:
        from unet_nested4tiny_objects_keypoints_amd import ObjectPaste
        crops = make(ObjectPaste(max_pastes=SLOTS, p=1.0, patch_radius=PATCH))
        ps = crops.paste
        inputs, target, _, _ = crops.batch(BATCH)
        params, index, _ = crops.last
        rows = crops.last_paste
        fresh = ops.points_target(labels, classes, index, params, CLASSES, (CROP, CROP), RADIUS)   # before the merge
        clean = ops.warp_batch(frames, index, params, (CROP, CROP), crops.mul, crops.add, 0.0)     # before the pixels
        work = torch.empty_like(fresh)
        h = {k: v.cpu() for k, v in rows._asdict().items()}
        took = (h["src"] >= 0)
        src_c = torch.floor(ps.src_xy.cpu().double() + 0.5).long()
        src_f, gain_bias, alpha = ps.src_frame.cpu(), params[:, 12:14].cpu(), ps.alpha
        ys, xs = torch.meshgrid(torch.arange(CROP, device=dev), torch.arange(CROP, device=dev), indexing="ij")
        pixels = torch.stack([xs.reshape(-1), ys.reshape(-1)], dim=1).float()
        jobs = [(n, k, int(h["src"][n, k]), int(h["dst"][n, k, 0]), int(h["dst"][n, k, 1]), int(h["code"][n, k]))
                for n, k in took.nonzero().tolist()]
        R = PATCH

        def composition(inp, tgt):
            for n, k, t, px, py, code in jobs:
                cx, cy = int(src_c[t, 0]), int(src_c[t, 1])
                patch = frames[int(src_f[t]), cy - R:cy + R + 1, cx - R:cx + R + 1, 0].float()
                patch = float(gain_bias[n, 0]) * (patch * crops.mul[0] + crops.add[0]) + float(gain_bias[n, 1])
                patch = torch.rot90(patch, -(code & 3), dims=(0, 1))
                if code & 4:
                    patch = torch.flip(patch, dims=(1,))
                d = inp[n, 0, py - R:py + R + 1, px - R:px + R + 1]
                d.copy_(torch.where(alpha == 1, patch, torch.where(alpha == 0, d, d + alpha * (patch - d))))
            for n in range(BATCH):
                for c in range(CLASSES):
                    if not bool((h["cls"][n] == c).any()):
                        continue
                    live = rows.cls[n] == c
                    v = torch.exp(-0.5 * torch.cdist(pixels, rows.xy[n][live]).min(dim=1).values / RADIUS).view(CROP, CROP)
                    tgt[n, c] = torch.where(tgt[n, c] < 0, tgt[n, c], torch.maximum(tgt[n, c], v))
            return inp, tgt

        c_in, c_t = composition(clean.clone(), fresh.clone())
        result["composition_agrees"] = {"inputs_equal": bool(torch.equal(c_in, inputs)),
                                        "targets_max_abs_difference": float((c_t - target).abs().max())}
        result["pastes"] = {"accepted": int(took.sum()), "slots": int(took.numel())}
        c_in, c_t = clean.clone(), fresh.clone()

        def merge():
            work.copy_(fresh)
            ops.paste_target(work, rows.xy, rows.cls, RADIUS)

        def compose():
            c_in.copy_(clean)
            c_t.copy_(fresh)
            composition(c_in, c_t)

        contenders += [
            Variant("(b) crops.batch(32) with paste", lambda: crops.batch(BATCH)),
            Variant("(c) paste_draw", lambda: ops.paste_draw(
                SLOTS, 7, ps.src_frame, ps.src_xy, ps.src_class, labels, classes, index, params, CLASSES, (SIDE, SIDE),
                (CROP, CROP), 1.0, PATCH, ps.clearance, True)),
            Variant("(d) paste_apply", lambda: ops.paste_apply(
                inputs, rows.src, rows.dst, rows.code, ps.src_frame, ps.src_xy, ps.src_class, frames, params, crops.mul,
                crops.add, ps.alpha, CLASSES)),
            Variant("(e) copy_ + paste_target", merge),
            Variant("(f) copy_", lambda: work.copy_(fresh)),
            Variant("(g) torch composition (with two copy_)", compose),
        ]
    contenders.append(Variant(a_again, lambda: plain.batch(BATCH)))
    times, rounds = alternate(contenders, args.window)
    med = {k: t[len(t) // 2] for k, t in times.items()}
    result["rounds"] = rounds
    result["contenders"] = [{"name": k, "ms_median": med[k], "ms_min": t[0], "ms_max": t[-1], "samples": len(t)}
                            for k, t in times.items()]
    result["spread_of_a"] = abs(med[a_again] - med[a_name]) / med[a_name]
    if not args.plain_only:
        e, f = med["(e) copy_ + paste_target"], med["(f) copy_"]
        result["target_bytes"] = work.numel() * 4
        result["paste_target_ms"] = e - f
        result["ratio_paste_target_over_copy"] = (e - f) / f
        result["ratio_b_over_a"] = med["(b) crops.batch(32) with paste"] / med[a_name]
        result["three_launches_ms"] = med["(c) paste_draw"] + med["(d) paste_apply"] + (e - f)
        result["ratio_composition_over_launches"] = ((med["(g) torch composition (with two copy_)"] - 2 * f)
                                                     / (med["(d) paste_apply"] + (e - f)))
    for r in result["contenders"]:
        print("  %-40s %9.4f ms  (min %.4f, max %.4f, %d samples)" % (r["name"], r["ms_median"], r["ms_min"], r["ms_max"],
                                                                     r["samples"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps({"wrote": args.out, **{k: v for k, v in result.items() if k.startswith(("ratio", "spread", "compo"))}}))


if __name__ == "__main__":
    main()
