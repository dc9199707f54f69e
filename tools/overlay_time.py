#!/usr/bin/env python3
"""Time of the overlay renderer ("Overlay").

One system of `streams` streams of width x height with uploaded maps (three seeded scenes cycled over the streams), a few frames
tracked so that every stream has found patches to draw.  Then, device output into one buffer of streams * height * width * 4 bytes:
    full        vslam_render_overlay(points | trails): every pixel written (gray base + discs)
    in_place    ... | VSLAM_DRAW_IN_PLACE: only drawn pixels written
    copy        a device-to-device copy of the same number of bytes, HIP events around it in this process: the yardstick
Each is warmed up, then repeated; the renders are timed by vslam_get_render_timing (HIP events around the launches), the copy by
events on torch's stream.  Median, minimum and maximum in ms, the ratio full / copy, one JSON line.

    python tools/overlay_time.py --streams 64 --out profiles/overlay_time.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dry", action="store_true", help="plan only (no device)")
    args = ap.parse_args()
    S, W, H = args.streams, args.width, args.height
    nbytes = S * H * W * 4
    if args.dry:
        print(json.dumps({"streams": S, "size": [W, H], "output_bytes": nbytes}))
        return
    import numpy as np
    import torch
    from helpers import make_scene
    from visualslam_android_amd import capi
    base = [make_scene(W, H, seed=700 + k, n_frames=args.frames) for k in range(3)]
    g = capi.System(capi.default_params(W, H, S, patch_size=8, overlay=1))
    for s in range(S):
        f, m, _fr = base[s % 3]
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
    for t in range(args.frames):
        g.track_frame(np.stack([base[s % 3][2][t] for s in range(S)]))
    discs = []
    out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    src = torch.ones(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"streams": S, "size": [W, H], "output_bytes": nbytes}
    flags = capi.DRAW_POINTS | capi.DRAW_TRAILS
    for name, fl in (("full", flags), ("in_place", flags | capi.DRAW_IN_PLACE)):
        ms = []
        for k in range(args.warmup + args.repeats):
            g.render_overlay_device(None, out.data_ptr(), 4 * W, 4 * W * H, fl)
            t = g.render_timing()
            if k >= args.warmup:
                ms.append(t)
        res[name] = summary(ms)
    discs = [g.overlay_info(s)["discs"] for s in range(S)]
    res["discs_per_stream"] = {"min": min(discs), "median": statistics.median(discs), "max": max(discs)}
    ms = []
    for k in range(args.warmup + args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out.copy_(src)
        e1.record()
        e1.synchronize()
        if k >= args.warmup:
            ms.append(e0.elapsed_time(e1))
    res["copy"] = summary(ms)
    res["full_over_copy"] = res["full"]["median_ms"] / res["copy"]["median_ms"]
    res["copy_GBps"] = nbytes / (res["copy"]["median_ms"] * 1e-3) / 1e9
    g.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
