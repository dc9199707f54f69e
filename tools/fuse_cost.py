#!/usr/bin/env python3
"""Cost of one vslam_fuse_points over a whole batch ("Point fusion").

A small system makes the stream once: the two halves of a seeded scene's map (4 + 4 keyframes of 640 x 480, 8 x 8 patches, as
tools/merge_cost.py and tests/test_gpu_merge.py cut them) in two streams, two frames, merge 0 <- 1, frames until the new queue is empty
(ReFindNewlyMade has looked for every appended point in the destination's keyframes).  Its snapshot, kept in device memory, is restored
into every one of `--streams` streams of a large system whose capacities the map fills.  Then one vslam_fuse_points over one stream
(in the small system: the first call of the process, which also loads the kernels; in the large one: the figure for one stream), that
stream restored again, and one call over all streams.  Each call is timed by HIP events around its four launches
(vslam_get_fuse_timing).  The bytes are what k_fuse_find must read at least: per tile of 256 candidate points, per keyframe, the row's
cells below the tile's end, 24 bytes each -- every row once per tile.  One JSON line per measurement.

    python tools/fuse_cost.py --streams 3072
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE = 256


def find_bytes(nk, n):
    """bytes of measurement rows one stream's find must read at least: tile [p0, pe) stages the cells [0, pe - 1) of every row"""
    return sum(nk * 24 * (min(p0 + TILE, n) - 1) for p0 in range(0, n, TILE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--min-views", type=int, default=2)
    args = ap.parse_args()
    S, W, H = args.streams, 640, 480
    import numpy as np
    from helpers import make_scene
    from test_gpu_merge import halves
    from visualslam_android_amd import capi
    opts = dict(patch_size=8, ba_sum_order=1, grow_map=3, idle_iterations=1)
    f, m, frames = make_scene(W, H, seed=1234, n_frames=16)
    first, second, _ = halves(m)
    small = capi.System(capi.default_params(W, H, 2, **opts))
    for s, part in enumerate((first, second)):
        small.load_map(s, part); small.set_pose(s, f.pose(-1))
    t = 0
    for t in range(2):
        small.track_frame(np.stack([frames[t]] * 2))
    counts = (small.state(0).n_keyframes, small.state(0).n_points, small.state(1).n_keyframes, small.state(1).n_points)
    small.merge_maps([0], [1])
    t = 2
    while small.idle_stats(0)["new_queue"] > 0 and t < len(frames):
        small.track_frame(np.stack([frames[t]] * 2)); t += 1
    assert small.idle_stats(0)["new_queue"] == 0 and small.state(0).quality == 2
    nk, n = small.state(0).n_keyframes, small.state(0).n_points
    hip = C.CDLL("libamdhip64.so")
    nbytes = small.snapshot_size(0)
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(nbytes)) == 0
    assert small.snapshot(0, out=(dev.value, nbytes)) == nbytes

    def report(g, streams, tag):
        g.fuse_points(streams, args.radius, args.min_views)
        ms = g.fuse_timing()
        cnt = g.S if streams is None else len(streams)
        total = cnt * find_bytes(nk, n)
        info = g.fuse_info(0)
        print(json.dumps({"fuse": tag, "streams": cnt, "keyframes": nk, "points": n, "merged_from": counts, "frames_to_drain": t - 2, "radius": args.radius,
                          "min_views": args.min_views, "dropped": info["dropped"], "taken": info["taken"], "not_taken": info["not_taken"], "chained": info["chained"],
                          "fuse_ms": round(ms, 4), "find_bytes_min": total, "TB_per_s": round(total / (ms * 1e-3) / 1e12, 3)}), flush=True)

    report(small, [0], "cold call, one stream")
    small.close()
    g = capi.System(capi.default_params(W, H, S, max_keyframes=nk, max_points=n, **opts))
    for s in range(S):
        g.restore(s, dev.value, nbytes)
    g.synchronize()
    report(g, [0], "one stream")
    g.restore(0, dev.value, nbytes)
    g.synchronize()
    report(g, None, "all streams")
    assert all(g.fuse_info(s)["dropped"] == g.fuse_info(0)["dropped"] for s in (1, S // 2, S - 1))
    g.close()
    hip.hipFree(dev)


if __name__ == "__main__":
    main()
