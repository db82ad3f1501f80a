"""Ignore masks on the GPU box: what the bit-plane mark costs per training batch beside the rectangle mark it replaces
for outlines, beside a torch composition and beside a plain write of the target; and the one-off cost of building a mask.

(a) The mark.  Batch 32 of 256 x 256 windows, C = 4, from four 4096 x 4096 frames (the geometry of tools/bench_crops.py;
    the windows are those ``SceneCrops`` draws from seed 1).  Contenders, all writing into the same [32, 4, 256, 256]:
      mask P = 1 / P = 4      unetpp_target_ignore_mask over one every-class plane / four planes (every class, 0, 1, 2)
      rectangles R = 16 / 300 unetpp_target_ignore, the existing path an outline would be approximated with
      torch                   per sample grid_sample(mode="nearest") of the float mask of the sample's frame at the same
                              source positions (the grid is built outside the timing), then torch.where into the target
      fill                    out.fill_(-1): a plain write of every byte a mark could write -- the floor
    The kernels are a few microseconds long, so events around Python calls may show the host's submission rate: every
    contender but torch is therefore also captured 64 times into a HIP graph and the replays timed, alternating
    (tools/bench_ignore.py: graph_replays) -- the device's own time per launch.  The call-by-call times are taken with HIP
    events around chunks of calls, contenders alternating, at least 20 rounds after a warm-up, medians.
(b) One-off.  ``IgnoreMask.from_raster`` of one 4096 x 4096 plane (uint8 and float32), ``from_polygons`` of 64 rings of 32
    vertices onto one such plane, and the torch packing ``from_raster`` uses on CPU tensors, run on the GPU.

    python tools/bench_mask.py [--out profiles/mask/bench_mask_mi355x.json] [--window 0.3]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import math
import os
import platform
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.bench_crops import BATCH, CLASSES, CROP, LABELS, RADIUS, SIDE, S, Variant  # noqa: E402
from tools.bench_ignore import graph_replays, library_hash, summary  # noqa: E402

MIN_ROUNDS = 20
RINGS, RING_VERTICES = 64, 32


def alternate(variants, window_s):
    """tools/bench_crops.py: alternate, with at least MIN_ROUNDS rounds"""
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
    while rounds < MIN_ROUNDS or min(sum(total[v.name]) * v.inner for v in variants) < window_s * 1e3:
        for v in variants:
            v.chunk()
        torch.cuda.synchronize()
        for v in variants:
            total[v.name] += v.drain()
        rounds += 1
        if rounds >= 400:
            break
    return {k: sorted(t) for k, t in total.items()}, rounds


def rings(g, count, vertices, side):
    """[1, count, vertices, 2] float32: wobbly rings of 60..400 pixels radius scattered over the frame"""
    centre = torch.rand(count, 1, 2, generator=g) * side
    radius = (torch.rand(count, 1, generator=g) * 340 + 60) * (0.75 + 0.5 * torch.rand(count, vertices, generator=g))
    angle = torch.arange(vertices).float().view(1, -1) * (2 * math.pi / vertices)
    return (centre + radius.unsqueeze(-1) * torch.stack([angle.cos(), angle.sin()], dim=-1)).unsqueeze(0).contiguous()


def measure_mark(dev, window):
    from unet_nested4tiny_objects_keypoints_amd import IgnoreMask, SceneCrops, ops
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (S, SIDE, SIDE, 1), dtype=torch.uint8, generator=g).to(dev)
    labels = (torch.rand(S, LABELS, 2, generator=g) * (SIDE - 1)).to(dev)
    classes = torch.randint(0, CLASSES, (S, LABELS), dtype=torch.int32, generator=g).to(dev)
    crops = SceneCrops(frames, labels, classes, CLASSES, crop=(CROP, CROP), radius=RADIUS, seed=1)
    _, target, _, _ = crops.batch(BATCH)
    rows, index, _ = crops.last
    del frames

    def rect_set(r):
        corner = torch.rand(S, r, 2, generator=g) * (SIDE - 400)
        extent = torch.rand(S, r, 2, generator=g) * 380 + 20
        return (torch.cat([corner, corner + extent], dim=2).to(dev),
                torch.randint(-1, CLASSES, (S, r), dtype=torch.int32, generator=g).to(dev))

    r16, r300 = rect_set(16), rect_set(300)
    # planes from rings: outlines a rectangle list would only approximate
    verts = torch.cat([rings(g, RINGS, RING_VERTICES, SIDE) for _ in range(S)]).to(dev)
    counts = torch.full((S, RINGS), RING_VERTICES, dtype=torch.int32, device=dev)
    plane4 = (torch.arange(RINGS) % 4).to(torch.int32)
    m1 = IgnoreMask.from_polygons(verts, counts, (SIDE, SIDE))
    m4 = IgnoreMask.from_polygons(verts, counts, (SIDE, SIDE), poly_plane=plane4, plane_class=[-1, 0, 1, 2])
    out = torch.empty_like(target)
    share = {}
    for name, m in (("mask P = 1", m1), ("mask P = 4", m4)):
        out.fill_(0.0)
        ops.target_ignore_mask(out, m.bits, m.plane_class, index, rows, (SIDE, SIDE), True)
        share[name] = float((out < 0).float().mean())
    for name, (rc, rk) in (("rectangles R = 16", r16), ("rectangles R = 300", r300)):
        out.fill_(0.0)
        ops.target_ignore(out, rc, rk, index, rows, (SIDE, SIDE), True)
        share[name] = float((out < 0).float().mean())

    # the torch composition: nearest sampling of the float mask at the same source positions
    mask_f = m1.to_raster().float()                                      # [S, 1, H, W]
    xo = torch.arange(CROP, device=dev, dtype=torch.float32).view(1, 1, CROP)
    yo = torch.arange(CROP, device=dev, dtype=torch.float32).view(1, CROP, 1)
    P = rows.view(BATCH, 16, 1, 1)
    xs, ys = (P[:, 0] * xo + P[:, 1] * yo) + P[:, 2], (P[:, 3] * xo + P[:, 4] * yo) + P[:, 5]
    grid = torch.stack([2.0 * xs / (SIDE - 1) - 1.0, 2.0 * ys / (SIDE - 1) - 1.0], dim=-1)       # [N, Ho, Wo, 2]
    frame_of = index.tolist()
    minus = torch.full((), -1.0, device=dev)

    def torch_mark():
        for n in range(BATCH):
            hit = torch.nn.functional.grid_sample(mask_f[frame_of[n]:frame_of[n] + 1], grid[n:n + 1], mode="nearest",
                                                  padding_mode="zeros", align_corners=True)
            out[n] = torch.where(hit[0] > 0, minus, out[n])

    fns = {
        "mask P = 1": lambda: ops.target_ignore_mask(out, m1.bits, m1.plane_class, index, rows, (SIDE, SIDE), True),
        "mask P = 4": lambda: ops.target_ignore_mask(out, m4.bits, m4.plane_class, index, rows, (SIDE, SIDE), True),
        "rectangles R = 16": lambda: ops.target_ignore(out, r16[0], r16[1], index, rows, (SIDE, SIDE), True),
        "rectangles R = 300": lambda: ops.target_ignore(out, r300[0], r300[1], index, rows, (SIDE, SIDE), True),
        "fill": lambda: out.fill_(-1.0),
    }
    contenders = [Variant(k, f) for k, f in fns.items()] + [Variant("torch", torch_mark),
                                                            Variant("fill again, closing the round", fns["fill"])]
    times, rounds = alternate(contenders, window)
    for r in summary(times):
        print("  %-34s %9.4f ms" % (r["name"], r["ms_median"]))
    replayed = graph_replays(fns)
    for name, ms in replayed.items():
        print("  %-34s %9.4f ms per launch in a graph replay" % (name, ms))
    med = {name: t[len(t) // 2] for name, t in times.items()}
    return {"workload": {"frames": [S, SIDE, SIDE], "batch": BATCH, "crop": [CROP, CROP], "classes": CLASSES,
                         "rings_per_frame": RINGS, "vertices_per_ring": RING_VERTICES, "outside": True,
                         "ignored_share_of_the_batch": share, "mask_coverage": m1.coverage().flatten().tolist()},
            "rounds": rounds, "contenders": summary(times),
            "spread_of_fill": abs(med["fill"] - med["fill again, closing the round"]) / min(med["fill"], med["fill again, closing the round"]),
            "graph_replay_ms_per_launch": replayed,
            "graph_replay_ratio_over_fill": {k: v / replayed["fill"] for k, v in replayed.items()},
            "graph_replay_ratio_mask1_over_rect16": replayed["mask P = 1"] / replayed["rectangles R = 16"],
            "graph_replay_ratio_mask1_over_rect300": replayed["mask P = 1"] / replayed["rectangles R = 300"],
            "ratio_torch_over_mask1_call_by_call": med["torch"] / med["mask P = 1"],
            "target_bytes": out.numel() * 4, "mask_bytes_per_plane": SIDE * ((SIDE + 31) // 32) * 4}


def measure_one_off(dev, window):
    from unet_nested4tiny_objects_keypoints_amd import IgnoreMask
    from unet_nested4tiny_objects_keypoints_amd.ignore import _pack_torch
    g = torch.Generator().manual_seed(3)
    u8 = (torch.rand(1, 1, SIDE, SIDE, generator=g) < 0.3).to(torch.uint8).to(dev)
    f32 = u8.float()
    on = u8.bool()
    verts = rings(g, RINGS, RING_VERTICES, SIDE).to(dev)
    counts = torch.full((1, RINGS), RING_VERTICES, dtype=torch.int32, device=dev)
    assert torch.equal(IgnoreMask.from_raster(u8).bits, _pack_torch(on))
    contenders = [Variant("from_raster uint8", lambda: IgnoreMask.from_raster(u8)),
                  Variant("from_raster float32", lambda: IgnoreMask.from_raster(f32)),
                  Variant("from_polygons 64 rings x 32 vertices", lambda: IgnoreMask.from_polygons(verts, counts, (SIDE, SIDE))),
                  Variant("torch packing of the bool raster", lambda: _pack_torch(on)),
                  Variant("from_raster uint8 again, closing the round", lambda: IgnoreMask.from_raster(u8))]
    times, rounds = alternate(contenders, window)
    for r in summary(times):
        print("  %-44s %9.4f ms" % (r["name"], r["ms_median"]))
    return {"plane": [SIDE, SIDE], "rounds": rounds, "contenders": summary(times),
            "polygon_coverage": float(IgnoreMask.from_polygons(verts, counts, (SIDE, SIDE)).coverage()[0, 0])}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(root, "profiles", "mask", "bench_mask_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.3, help="device-event seconds per contender (at least)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mask.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import _lib
    props = torch.cuda.get_device_properties(0)
    result = {
        "box": platform.node(), "device": torch.cuda.get_device_name(0), "arch": props.gcnArchName,
        "compute_units": props.multi_processor_count,
        "library": os.path.basename(_lib.LIB_PATH), "library_sha256": library_hash(_lib.LIB_PATH), "window_s": args.window,
        "timing": "HIP events on the launching stream around chunks of calls; all contenders alternate in one process; at "
                  "least %d rounds after a warm-up; medians; graph replays of %s launches for the device's own time"
                  % (MIN_ROUNDS, "64"),
        "mark": measure_mark(dev, args.window),
        "one_off": measure_one_off(dev, args.window),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
