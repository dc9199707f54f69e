#!/usr/bin/env python3
"""Cost of one vslam_transform_maps over a whole batch ("Similarity transform"), beside vslam_retire_keyframes over the same
batch as a yardstick.

One system of `--streams` streams at 640 x 480 with patch size 8, three seeded scenes of 8 keyframes cycled over the streams as
bench.py's map size, max_keyframes = 8.  No frame is tracked: both operations walk the map's arrays whatever their contents.  The
transform is called `--repeat` times for every stream (streams == NULL; the first call also loads the kernel), then once for one stream,
then every stream retires one keyframe by policy; each is timed by HIP events on the system's stream (vslam_get_transform_timing,
vslam_get_retire_timing).  One JSON line per measurement.

    python tools/transform_cost.py --streams 3072
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    args = ap.parse_args()
    S, W, H = args.streams, args.width, args.height
    import numpy as np
    from helpers import make_scene
    from transform_ref import pose12, rotation
    from visualslam_android_amd import capi
    n_kf = 8
    base = [make_scene(W, H, seed=700 + k, n_frames=1, n_keyframes=n_kf) for k in range(3)]
    g = capi.System(capi.default_params(W, H, S, patch_size=8, max_keyframes=n_kf))
    for s in range(S):
        f, m, _fr = base[s % 3]
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
    g.synchronize()
    points = [len(b[1]["points"]) for b in base]
    rng = np.random.default_rng(1)
    poses = np.stack([pose12(rotation(rng.normal(size=3), rng.uniform(-3, 3)), rng.normal(size=3)) for _ in range(S)])
    scales = np.exp(rng.uniform(-0.5, 0.5, size=S))
    for k in range(args.repeat):
        g.transform_maps(None, poses, scales)
        print(json.dumps({"transform_streams": S, "call": k, "points_per_stream": points, "keyframes": n_kf, "transform_ms": round(g.transform_timing(), 4)}), flush=True)
    g.transform_maps([S // 2], poses[:1], scales[:1])
    print(json.dumps({"transform_streams": 1, "transform_ms": round(g.transform_timing(), 4)}), flush=True)
    g.retire_keyframes(np.arange(S, dtype=np.int32))
    print(json.dumps({"retire_streams": S, "retire_ms": round(g.retire_timing(), 4)}), flush=True)
    g.close()


if __name__ == "__main__":
    main()
