"""Cascaded scene inference on the GPU box: what a frame costs when the deep head runs only where the shallow head fires.

Geometry: the headline network (fp32 storage, base 32, depth 4, 1 -> 4 channels), four 4096x4096x1 uint8 frames, deep
head 3 screened by head 1, tile 512, ``tta=None`` (8 tiles per forward) and ``tta="dihedral"`` (``--tta-chunk`` tiles per
forward, default 2: 16 samples of 512x512, as tools/bench_scene.py).  The weights are random: the time depends on how
many tiles are active, not on what the maps mean.  The active fraction is set through the threshold: a first call with
every tile active leaves ``last_scores``, and the threshold of fraction f is the ceil(f n)-th largest score (+inf for
0, -inf for 1); the fraction a call then achieves (ties share a score where screened rectangles overlap) is recorded.

Contenders, method of tools/bench_scene.py: all of a group run in one process and alternate, round after round, until
each has at least ``--window`` seconds of device-event time; the first contender is timed at both ends of a round and
the difference is the run's own spread.
  (a) plain ``SceneInference(head=3)(frames)``;
  (b) the screen stage alone, ``SceneInference(head=1)(frames)``;
  (c) the cascade at active fractions 0, 0.05, 0.25 and 1.0, next to the derived expectation
      t(screen stage) + fraction * t(plain) + t(screen launch);
  (d) the ``unetpp_scene_screen`` launch alone over the deep plan's rectangles, next to a plain read of M1 (``M1.max()``).

    python tools/bench_cascade.py [--out profiles/cascade/bench_cascade_mi355x.json] [--window 0.5] [--frame 4096]

Fails when no GPU is present: a timing taken anywhere else says nothing.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_scene import Contender, alternate  # noqa: E402

TILE, CHUNK, HEAD, SCREEN_HEAD = 512, 8, 3, 1
FRACTIONS = (0.0, 0.05, 0.25, 1.0)


def threshold_for(scores, fraction):
    """the threshold at which ceil(fraction * n) tiles (more where scores tie) are active"""
    if fraction <= 0.0:
        return float("inf")
    if fraction >= 1.0:
        return float("-inf")
    s = sorted(scores, reverse=True)
    return s[max(1, math.ceil(fraction * len(s))) - 1]


def run_launch(cascade, frames, window_s):
    """(d): the screen launch over the deep plan's rectangles against a plain read of M1"""
    from unet_nested4tiny_objects_keypoints_amd import ops
    M1 = cascade.screen(frames)
    p = cascade._plan(int(M1.shape[0]), int(M1.shape[2]), int(M1.shape[3]), M1.device)
    launch = lambda: ops.scene_screen(M1, p.screen, p.screen_dev, 0.5)  # noqa: E731
    cs = [Contender("scene_screen [start of round]", lambda: [launch() for _ in range(20)]),
          Contender("M1.max()", lambda: [M1.max() for _ in range(20)]),
          Contender("scene_screen [end of round]", lambda: [launch() for _ in range(20)])]
    rounds, spread = alternate(cs, window_s)
    one = 0.5 * (cs[0].median() + cs[2].median()) / 20
    read = cs[1].median() / 20
    live = p.screen[p.screen[:, 0] >= 0]
    area = float(((live[:, 4] - live[:, 3]) * (live[:, 6] - live[:, 5])).sum())
    alg = 4.0 * int(M1.shape[1]) * area
    r = {"rectangles": p.n, "margin": cascade.margin, "classes": int(M1.shape[1]), "screened_pixels": area,
         "frame_pixels": float(M1.shape[0] * M1.shape[2] * M1.shape[3]), "screen_launch_ms": one, "launches": 1,
         "algorithmic_bytes": alg, "achieved_algorithmic_GB_per_s": alg / (one * 1e-3) / 1e9, "plain_read_ms": read,
         "plain_read_bytes": 4.0 * M1.numel(), "plain_read_GB_per_s": 4.0 * M1.numel() / (read * 1e-3) / 1e9,
         "spread_ms": spread / 20, "rounds": rounds}
    print("== screen launch alone: %.4f ms over %d rectangles (%.0f GB/s algorithmic); M1.max() %.4f ms (%.0f GB/s)" % (
        one, p.n, r["achieved_algorithmic_GB_per_s"], read, r["plain_read_GB_per_s"]))
    sys.stdout.flush()
    return r


def run_group(model, frames, tta, chunk, window_s):
    from unet_nested4tiny_objects_keypoints_amd import CascadeSceneInference, SceneInference
    plain = SceneInference(model, head=HEAD, tile=TILE, tta=tta, chunk=chunk)
    kw = dict(head=HEAD, screen_head=SCREEN_HEAD, tile=TILE, tta=tta, chunk=chunk, screen_chunk=CHUNK)
    first = CascadeSceneInference(model, **kw)
    first.threshold = float("-inf")
    equal = bool(torch.equal(first(frames), plain(frames)))        # every tile active: the plain scene, bit for bit
    scores = first.last_scores.cpu().tolist()
    cascades = []
    for f in FRACTIONS:
        c = CascadeSceneInference(model, **kw)
        c.threshold = threshold_for(scores, f)
        cascades.append(c)
    launch = run_launch(first, frames, window_s)
    cs = [Contender("plain scene [start of round]", lambda: plain(frames)),
          Contender("screen stage alone", lambda: first.screen(frames))]
    cs += [Contender("cascade at fraction %g" % f, (lambda c: lambda: c(frames))(c)) for f, c in zip(FRACTIONS, cascades)]
    cs += [Contender("plain scene [end of round]", lambda: plain(frames))]
    rounds, spread = alternate(cs, window_s)
    t_plain = 0.5 * (cs[0].median() + cs[-1].median())
    t_screen = cs[1].median()
    rows = []
    for f, c, con in zip(FRACTIONS, cascades, cs[2:-1]):
        expect = t_screen + c.last_fraction * t_plain + launch["screen_launch_ms"]
        rows.append({"fraction_asked": f, "fraction_achieved": c.last_fraction, "threshold": c.threshold,
                     "deep_forwards": c.last_forwards, "ms": con.median(), "expected_ms": expect,
                     "measured_over_expected": con.median() / expect, "speedup_over_plain": t_plain / con.median()})
        print("   fraction %.2f (achieved %.3f, %d deep forwards): %.2f ms, expected %.2f, plain / cascade = %.2f" % (
            f, c.last_fraction, c.last_forwards, con.median(), expect, t_plain / con.median()))
    out = {"tta": tta, "variants": len(plain.variants), "head": HEAD, "screen_head": SCREEN_HEAD, "tile": TILE,
           "deep_halo": plain.halo, "screen_halo": first.screen.halo, "margin": first.margin, "chunk_tiles": chunk,
           "screen_chunk_tiles": CHUNK, "frames": list(frames.shape), "tiles": len(scores),
           "all_active_equals_plain_bitwise": equal, "rounds": rounds, "spread_ms": spread, "plain_scene_ms": t_plain,
           "screen_stage_ms": t_screen, "expectation": "screen_stage_ms + fraction_achieved * plain_scene_ms + screen_launch_ms",
           "cascade": rows, "screen_launch": launch, "ms_median": {c.name: c.median() for c in cs}}
    print("== tta %s: plain %.2f ms, screen stage %.2f ms, spread %.2f ms, %d rounds" % (tta, t_plain, t_screen, spread, rounds))
    sys.stdout.flush()
    del plain, first, cascades, cs
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "cascade", "bench_cascade_mi355x.json"))
    ap.add_argument("--window", type=float, default=0.5, help="device-event seconds per contender (at least)")
    ap.add_argument("--frame", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--tta-chunk", type=int, default=2, help="tiles per forward with the eight variants")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_cascade.py needs a GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    from unet_nested4tiny_objects_keypoints_amd import UNet_Nested, _lib
    torch.manual_seed(0)
    model = UNet_Nested(in_channels=1, n_classes=4, feature_scale=1, depth=4).to(dev).eval()
    frames = torch.randint(0, 256, (args.frames, args.frame, args.frame, 1), dtype=torch.uint8, device=dev)
    result = {"device": torch.cuda.get_device_name(0), "source_hash": _lib.source_hash(), "window_s": args.window,
              "timing": "HIP events on the launching stream around whole calls (the cascade's one read-back included); all "
                        "contenders of a group alternate in one process; median over the rounds; spread = the two "
                        "placements of the first contender",
              "network": "UNet_Nested fp32, base 32, depth 4, 1 -> 4 channels, random weights", "groups": []}
    for tta, chunk in ((None, CHUNK), ("dihedral", args.tta_chunk)):
        result["groups"].append(run_group(model, frames, tta, chunk, args.window))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
