"""Ignore regions on the GPU box: what the ``*_ignore`` loss calls cost beside their plain twins, and what the mark launch
adds to a training batch from scenes.

(a) Losses.  3 heads of [32, 4, 256, 256] (the head shape of the headline training step).  Per loss -- FocalLoss_BCE_2d,
    the top-k focal loss at fraction 0.01, the penalty-reduced focal loss -- four contenders, warmed up, then alternating
    in one process round after round until each has at least ``--window`` seconds (default 0.5) of device-event time;
    medians over the rounds:
      plain          the plain entry point on a target without a negative element;
      ignore / clean the ``_ignore`` entry point on the same target;
      ignore / 25 %  the ``_ignore`` entry point with a quarter of the target at -1 (64 x 64 blocks of a 128 x 128 grid);
      plain again    closing the round: the distance between the two plain medians is the spread of the measurement.
    The ``_ignore`` calls move the bytes of their twins, so a ratio beyond the spread is a finding.
(b) Batches.  ``crops.batch(32)`` of 256 x 256 windows from four 4096 x 4096 frames with 2000 labels each, without ignore
    and with 16 rectangles per frame plus ``ignore_outside``; then the mark launch alone against ``out.fill_(-1)`` on
    [32, 4, 256, 256], a plain write of every byte the mark launch could write.  Both are a few microseconds long, so
    the events around back-to-back Python calls may show the host's submission rate instead of the kernels: the two are
    therefore also captured 64 times each into a HIP graph and the replays timed, alternating, which leaves the device's
    own time per launch (the kernel and the dispatch of the next one, no host work).

``--plain-only`` times the three plain loss calls alone (each opening and closing a round) and works on a library built
from a commit without the new entry points (``UNETPP_LIB=...``): the record that the plain calls did not move.

    python tools/bench_ignore.py [--out profiles/ignore/bench_ignore_mi355x.json] [--window 0.5] [--plain-only]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.bench_crops import BATCH, CLASSES, CROP, LABELS, RADIUS, SIDE, S, Variant, alternate  # noqa: E402

HEADS, SHAPE, POSITIVES = 3, (32, 4, 256, 256), 0.001
GAMMA, FRACTION = 3.0, 0.01
ALPHA, BETA, EPS, POSITIVE = 2.0, 4.0, 1e-4, 1.0
RECTS = 16


def loss_calls(preds, target, ignore):
    """{name: callable} of the three heads calls on (preds, target)"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    kw = {"ignore": True} if ignore else {}
    rows, pixels = SHAPE[0] * SHAPE[1], SHAPE[2] * SHAPE[3]
    k = max(1, -(-int(FRACTION * pixels * 1000) // 1000))
    return {
        "focal": lambda: ops.focal_bce_heads(preds, target, rows, GAMMA, **kw),
        "topk": lambda: ops.topk_focal_heads(preds, target, k, rows, GAMMA, **kw),
        "prfocal": lambda: ops.pr_focal_heads(preds, target, ALPHA, BETA, EPS, POSITIVE, **kw),
    }


def summary(times):
    return [{"name": name, "ms_median": t[len(t) // 2], "ms_min": t[0], "ms_max": t[-1], "samples": len(t)}
            for name, t in times.items()]


def measure_losses(preds, clean, quarter, window, plain_only):
    out = {}
    plain, ign_clean, ign_quarter = loss_calls(preds, clean, False), None, None
    if not plain_only:
        ign_clean, ign_quarter = loss_calls(preds, clean, True), loss_calls(preds, quarter, True)
    for kind in ("focal", "topk", "prfocal"):
        contenders = [Variant("plain", plain[kind])]
        if not plain_only:
            contenders += [Variant("ignore / clean", ign_clean[kind]), Variant("ignore / 25 %", ign_quarter[kind])]
        contenders.append(Variant("plain again, closing the round", plain[kind]))
        times, rounds = alternate(contenders, window)
        med = {name: t[len(t) // 2] for name, t in times.items()}
        a, a2 = med["plain"], med["plain again, closing the round"]
        row = {"rounds": rounds, "contenders": summary(times), "spread_of_plain": abs(a - a2) / min(a, a2)}
        if not plain_only:
            row["ratio_ignore_clean_over_plain"] = med["ignore / clean"] / a
            row["ratio_ignore_quarter_over_plain"] = med["ignore / 25 %"] / a
        out[kind] = row
        print("  %-8s %s" % (kind, "  ".join("%s %.4f ms" % (r["name"], r["ms_median"]) for r in row["contenders"])))
    return out


GRAPH_LAUNCHES, GRAPH_SAMPLES = 64, 40


def graph_replays(fns):
    """{name: median ms per launch} of each callable captured GRAPH_LAUNCHES times in a row into a graph of its own; the
    graphs are replayed in turn, HIP events around every replay"""
    graphs = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(GRAPH_LAUNCHES):
                fn()
        graphs[name] = g
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    pairs = {name: [] for name in graphs}
    for _ in range(GRAPH_SAMPLES):
        for name, g in graphs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            g.replay()
            e.record()
            pairs[name].append((s, e))
    torch.cuda.synchronize()
    return {name: sorted(s.elapsed_time(e) / GRAPH_LAUNCHES for s, e in p)[len(p) // 2] for name, p in pairs.items()}


def measure_batches(dev, window):
    from unet_nested4tiny_objects_keypoints_amd import IgnoreRegions, SceneCrops, ops
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (S, SIDE, SIDE, 1), dtype=torch.uint8, generator=g).to(dev)
    labels = (torch.rand(S, LABELS, 2, generator=g) * (SIDE - 1)).to(dev)
    classes = torch.randint(0, CLASSES, (S, LABELS), dtype=torch.int32, generator=g).to(dev)
    corner = torch.rand(S, RECTS, 2, generator=g) * (SIDE - 400)
    extent = torch.rand(S, RECTS, 2, generator=g) * 380 + 20
    rects = torch.cat([corner, corner + extent], dim=2).to(dev)
    rect_class = torch.randint(-1, CLASSES, (S, RECTS), dtype=torch.int32, generator=g).to(dev)
    ign = IgnoreRegions(rects, rect_class)
    plain = SceneCrops(frames, labels, classes, CLASSES, crop=(CROP, CROP), radius=RADIUS, seed=1)
    marked = SceneCrops(frames, labels, classes, CLASSES, crop=(CROP, CROP), radius=RADIUS, seed=1, ignore=ign,
                        ignore_outside=True)
    _, target, _, _ = marked.batch(BATCH)
    rows, index, _ = marked.last
    share = float((target < 0).float().mean())
    out = torch.empty_like(target)
    contenders = [
        Variant("(a) crops.batch(32)", lambda: plain.batch(BATCH)),
        Variant("(b) crops.batch(32), 16 rectangles per frame and ignore_outside", lambda: marked.batch(BATCH)),
        Variant("(c) target_ignore alone", lambda: ops.target_ignore(out, ign.rects, ign.rect_class, index, rows,
                                                                     (SIDE, SIDE), True)),
        Variant("(d) out.fill_(-1)", lambda: out.fill_(-1.0)),
        Variant("(a) again, closing the round", lambda: plain.batch(BATCH)),
    ]
    times, rounds = alternate(contenders, window)
    med = {name: t[len(t) // 2] for name, t in times.items()}
    a, a2 = med["(a) crops.batch(32)"], med["(a) again, closing the round"]
    for r in summary(times):
        print("  %-66s %9.4f ms" % (r["name"], r["ms_median"]))
    replayed = graph_replays({
        "target_ignore": lambda: ops.target_ignore(out, ign.rects, ign.rect_class, index, rows, (SIDE, SIDE), True),
        "out.fill_(-1)": lambda: out.fill_(-1.0)})
    for name, ms in replayed.items():
        print("  %-66s %9.4f ms per launch, %d launches per graph replay" % (name, ms, GRAPH_LAUNCHES))
    return {"workload": {"frames": [S, SIDE, SIDE, 1], "labels_per_frame": LABELS, "classes": CLASSES, "batch": BATCH,
                         "crop": [CROP, CROP], "rectangles_per_frame": RECTS, "ignored_share_of_the_batch": share},
            "rounds": rounds, "contenders": summary(times), "spread_of_a": abs(a - a2) / min(a, a2),
            "ratio_b_over_a": med["(b) crops.batch(32), 16 rectangles per frame and ignore_outside"] / a,
            "ratio_c_over_d": med["(c) target_ignore alone"] / med["(d) out.fill_(-1)"],
            "graph_replay_ms_per_launch": replayed, "graph_launches_per_replay": GRAPH_LAUNCHES,
            "graph_replay_ratio_mark_over_fill": replayed["target_ignore"] / replayed["out.fill_(-1)"],
            "target_bytes": out.numel() * 4}


def library_hash(path):
    """the first 16 hex digits of the SHA-256 of the shared object that is timed (whichever build it is)"""
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "ignore", "bench_ignore_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    ap.add_argument("--plain-only", action="store_true", help="the plain loss calls alone (any library build)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ignore.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib
    if args.plain_only:   # a library built from an earlier commit lacks the new entry points: do not ask for them
        handle = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(handle, n)]:
            del _lib.SIGNATURES[name]
    g = torch.Generator().manual_seed(0)
    clean = torch.rand(SHAPE, generator=g) * 0.999
    clean[torch.rand(SHAPE, generator=g) < POSITIVES] = 1.0
    quarter = clean.clone()
    for y in range(0, SHAPE[2], 128):
        for x in range(0, SHAPE[3], 128):
            quarter[:, :, y:y + 64, x:x + 64] = -1.0
    clean, quarter = clean.to(dev), quarter.to(dev)
    preds = [(torch.rand(SHAPE, generator=g) * 0.98 + 0.01).to(dev) for _ in range(HEADS)]
    result = {
        "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
        "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
        "library": os.path.basename(_lib.LIB_PATH), "library_sha256": library_hash(_lib.LIB_PATH),
        "window_s": args.window, "plain_only": args.plain_only,
        "timing": "HIP events on the launching stream around chunks of calls; all contenders alternate in one process; "
                  "median over the rounds; the first contender opens and closes every round",
        "loss_workload": {"heads": HEADS, "shape": list(SHAPE), "positives": POSITIVES, "gamma": GAMMA,
                          "topk_fraction": FRACTION, "alpha": ALPHA, "beta": BETA, "eps": EPS, "positive": POSITIVE,
                          "ignored_share_of_quarter": float((quarter < 0).float().mean())},
        "losses": measure_losses(preds, clean, quarter, args.window, args.plain_only),
    }
    if not args.plain_only:
        result["batches"] = measure_batches(dev, args.window)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
