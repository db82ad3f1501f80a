"""Scene inference on the GPU box: the tiled forward over one 4096x4096 frame against the forward alone on the same tiles,
the stitch launch against its torch composition, and the whole-frame forward at the sizes that are inside every limit.

Geometry: the headline network (fp32 storage, base 32, depth 4, 1 -> 4 channels), tile 512, heads 2 and 3, with and
without ``tta="dihedral"``, eager and graphed.  Without TTA a chunk is 8 tiles; with the eight variants a chunk is
``--tta-chunk`` tiles (default 2: 16 samples of 512x512).  A chunk of 8 tiles times 8 variants would be 64 samples whose
level-0 activation is exactly 2^31 bytes -- the size of a whole 4096x4096 frame's, which this tool is not here to try.

Contenders, method of tools/bench_infer.py: all of a group run in one process and alternate, round after round, until
each has at least ``--window`` seconds of device-event time; the first contender is timed at both ends of a round and
the difference is the run's own spread.
  (a) ``scene(frame)``: ms per frame and owned Mpx/s.
  (b) the forward alone over the same chunks of pre-gathered tiles: (a) - (b) is what gather plus stitch cost.
  (c) the stitch launch alone (one chunk of 8 tiles, K = 1 and K = 8) against the torch composition (per tile: slice,
      flip / transpose, sequential sum, divide, slice-assign): time and the number of torch operations issued.
  (d) whole-frame ``model.infer`` at 1024x1024 and 2048x2048 only.

    python tools/bench_scene.py [--out profiles/scene/bench_scene_mi355x.json] [--window 0.5] [--frame 4096]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

TILE, CHUNK = 512, 8


class Contender:
    def __init__(self, name, fn):
        self.name, self.fn, self.pairs, self.times = name, fn, [], []

    def run(self):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        self.fn()
        e.record()
        self.pairs.append((s, e))

    def drain(self):
        self.times += [s.elapsed_time(e) for s, e in self.pairs]
        self.pairs = []

    def median(self):
        t = sorted(self.times)
        return t[len(t) // 2]


def alternate(contenders, window_s, min_rounds=3, max_rounds=400):
    """contenders[0] and contenders[-1] are the same work: the two ends of a round.  -> (rounds, spread_ms)"""
    for c in contenders:
        for _ in range(2):
            c.fn()
    torch.cuda.synchronize()
    rounds = 0
    while rounds < min_rounds or min(sum(c.times) for c in contenders) < window_s * 1e3:
        for c in contenders:
            c.run()
        torch.cuda.synchronize()
        for c in contenders:
            c.drain()
        rounds += 1
        if rounds >= max_rounds:
            break
    a, b = contenders[0].median(), contenders[-1].median()
    pooled = sorted(contenders[0].times + contenders[-1].times)
    return rounds, max(abs(a - b), pooled[(9 * len(pooled)) // 10] - pooled[len(pooled) // 10])


def forward_only(scene, frame, graphed):
    """(b): the chunks of scene(frame), gathered once; each call runs the forward over all of them and nothing else"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    from unet_nested4tiny_objects_keypoints_amd.loader import _per_channel
    H, W = int(frame.shape[1]), int(frame.shape[2])
    th, tw = scene.tile_shape(H, W)
    dev = frame.device
    mul, add = _per_channel(scene.mul, 1, dev), _per_channel(scene.add, 1, dev)
    plan = scene._plan(1, H, W, dev)
    if graphed:   # the graph's own input holds one gathered chunk: the replay alone, no copy
        g = scene._graph(1, th, tw, dev)
        ops.warp_batch(frame, plan[0].index, plan[0].params, (th, tw), mul, add, 0.0, out=g.static_input)
        return lambda: [g(g.static_input) for _ in plan]
    xs = [ops.warp_batch(frame, c.index, c.params, (th, tw), mul, add, 0.0) for c in plan]
    return lambda: [scene.model.infer(x, scene.head, scene.ensemble) for x in xs]


def run_group(model, frame, head, tta, chunk, window_s):
    from unet_nested4tiny_objects_keypoints_amd import SceneInference
    H, W = int(frame.shape[1]), int(frame.shape[2])
    eager = SceneInference(model, head=head, tile=TILE, tta=tta, chunk=chunk)
    graphed = SceneInference(model, head=head, tile=TILE, tta=tta, chunk=chunk, graphed=True)
    same = bool(torch.equal(eager(frame), graphed(frame)))
    cs = [Contender("scene(frame) eager [start of round]", lambda: eager(frame)),
          Contender("infer alone on the gathered tiles, eager", forward_only(eager, frame, False)),
          Contender("scene(frame) graphed", lambda: graphed(frame)),
          Contender("GraphedForward alone on the gathered tiles", forward_only(graphed, frame, True)),
          Contender("scene(frame) eager [end of round]", lambda: eager(frame))]
    rounds, spread = alternate(cs, window_s)
    ms = {c.name: c.median() for c in cs}
    a_e = 0.5 * (cs[0].median() + cs[4].median())
    b_e, a_g, b_g = cs[1].median(), cs[2].median(), cs[3].median()
    n_chunks = len(eager._plan(1, H, W, frame.device))
    out = {"head": head, "tta": tta, "variants": len(eager.variants), "tile": TILE, "halo": eager.halo, "chunk_tiles": chunk,
           "samples_per_forward": chunk * len(eager.variants), "chunks_per_frame": n_chunks, "frame": [H, W],
           "efficiency_owned_over_computed": eager.efficiency(H, W), "graphed_equals_eager_bitwise": same,
           "rounds": rounds, "spread_ms": spread, "ms_median": ms,
           "eager": {"scene_ms_per_frame": a_e, "forward_alone_ms": b_e, "gather_plus_stitch_ms": a_e - b_e,
                     "gather_plus_stitch_share_of_forward": (a_e - b_e) / b_e, "owned_Mpx_per_s": H * W / a_e / 1e3,
                     "forward_ms_per_chunk": b_e / n_chunks},
           "graphed": {"scene_ms_per_frame": a_g, "forward_alone_ms": b_g, "gather_plus_stitch_ms": a_g - b_g,
                       "gather_plus_stitch_share_of_forward": (a_g - b_g) / b_g, "owned_Mpx_per_s": H * W / a_g / 1e3,
                       "forward_ms_per_chunk": b_g / n_chunks}}
    print("== head %d tta %s chunk %d: scene %.2f ms/frame eager (forward alone %.2f, +%.1f %%), %.2f graphed (forward "
          "alone %.2f, +%.1f %%); spread %.2f ms; %d rounds" % (
              head, tta, chunk, a_e, b_e, 100 * (a_e - b_e) / b_e, a_g, b_g, 100 * (a_g - b_g) / b_g, spread, rounds))
    sys.stdout.flush()
    del eager, graphed, cs
    torch.cuda.empty_cache()
    return out


def run_stitch(dev, K, window_s, n_classes=4, frame=2048):
    """(c): one chunk of 8 tiles of a 2048x2048 plan (halo 56), the launch against the torch composition"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    from unet_nested4tiny_objects_keypoints_amd.scene import plan_tiles
    rows, cols = plan_tiles(frame, frame, TILE, 56, 8)
    rects = [(0, oy, ox, y0, y1, x0, x1) for (oy, y0, y1) in rows for (ox, x0, x1) in cols][:CHUNK]
    codes = tuple(range(K))
    tiles = torch.randn(CHUNK, K, n_classes, TILE, TILE, device=dev)
    out = torch.zeros(1, n_classes, frame, frame, device=dev)
    table = ops.scene_rects(rects)
    table_dev = table.to(dev)
    issued = [0]

    def composition(count=False):
        n = 0
        for t, (_, oy, ox, y0, y1, x0, x1) in enumerate(rects):
            acc = None
            for k, code in enumerate(codes):
                v = tiles[t, k]
                if code & 2:
                    v, n = v.flip(-2), n + 1
                if code & 1:
                    v, n = v.flip(-1), n + 1
                if code & 4:
                    v = v.transpose(-1, -2)
                v = v[:, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
                if acc is not None:
                    acc, n = acc + v, n + 1
                else:
                    acc = v
            if K > 1:
                acc, n = acc / float(K), n + 1
            out[0, :, y0:y1, x0:x1] = acc
            n += 1
        if count:
            issued[0] = n

    composition(count=True)
    launch = lambda: ops.scene_stitch(tiles, table, table_dev, codes, out)  # noqa: E731
    cs = [Contender("scene_stitch [start of round]", lambda: [launch() for _ in range(20)]),
          Contender("torch composition", lambda: [composition() for _ in range(20)]),
          Contender("scene_stitch [end of round]", lambda: [launch() for _ in range(20)])]
    rounds, spread = alternate(cs, window_s)
    one = 0.5 * (cs[0].median() + cs[2].median()) / 20
    comp = cs[1].median() / 20
    owned = sum((y1 - y0) * (x1 - x0) for (_, _, _, y0, y1, x0, x1) in rects)
    alg = 4.0 * (K + 1) * n_classes * owned
    r = {"K": K, "tiles": CHUNK, "classes": n_classes, "owned_pixels": owned, "stitch_ms": one, "stitch_launches": 1,
         "composition_ms": comp, "composition_torch_ops_issued": issued[0], "speedup_over_composition": comp / one,
         "algorithmic_bytes": alg, "achieved_algorithmic_GB_per_s": alg / (one * 1e-3) / 1e9, "spread_ms": spread / 20,
         "rounds": rounds}
    print("== stitch alone K=%d: %.4f ms (%.0f GB/s algorithmic), torch composition %.4f ms in %d operations" % (
        K, one, r["achieved_algorithmic_GB_per_s"], comp, issued[0]))
    sys.stdout.flush()
    return r


def run_whole(model, size, head, window_s, dev):
    """(d): the whole-frame forward, only at sizes inside every limit of the launchers"""
    x = torch.rand(1, 1, size, size, device=dev)
    cs = [Contender("infer [start]", lambda: model.infer(x, head)), Contender("infer [end]", lambda: model.infer(x, head))]
    rounds, spread = alternate(cs, window_s)
    ms = 0.5 * (cs[0].median() + cs[1].median())
    print("== whole-frame infer(head=%d) %dx%d: %.2f ms, %.1f Mpx/s" % (head, size, size, ms, size * size / ms / 1e3))
    sys.stdout.flush()
    return {"size": size, "head": head, "ms": ms, "Mpx_per_s": size * size / ms / 1e3, "spread_ms": spread, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "scene", "bench_scene_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    ap.add_argument("--frame", type=int, default=4096)
    ap.add_argument("--tta-chunk", type=int, default=2, help="tiles per forward with the eight variants")
    ap.add_argument("--heads", default="2,3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_scene.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, _lib
    torch.manual_seed(0)
    model = UNet_Nested(in_channels=1, n_classes=4, feature_scale=1, depth=4).to(dev).eval()
    frame = torch.randint(0, 256, (1, args.frame, args.frame, 1), dtype=torch.uint8, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
              "timing": "HIP events on the launching stream around whole calls; all contenders of a group alternate in one "
                        "process; median over the rounds; spread = the two placements of the first contender",
              "network": "UNet_Nested fp32, base 32, depth 4, 1 -> 4 channels", "scene": [], "stitch": [], "whole_frame": []}
    for head in [int(h) for h in args.heads.split(",")]:
        result["scene"].append(run_group(model, frame, head, None, CHUNK, args.window))
        result["scene"].append(run_group(model, frame, head, "dihedral", args.tta_chunk, args.window))
    for K in (1, 8):
        result["stitch"].append(run_stitch(dev, K, args.window))
    for size in (1024, 2048):
        result["whole_frame"].append(run_whole(model, size, 3, args.window, dev))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
