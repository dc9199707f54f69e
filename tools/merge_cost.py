#!/usr/bin/env python3
"""Cost of one vslam_merge_maps over a whole batch ("Map merge").

One system of `--streams` streams at 640 x 480 with patch size 8 and max_keyframes = 8; three seeded scenes of 4 keyframes are cycled
over the pairs, so every pair (2i <- 2i + 1) appends 4 keyframes to 4 and fills its destination.  No frame is tracked: the merge moves
the map's arrays whatever their contents.  A small system of 4 streams first merges one pair (that call also loads the kernels and is
reported as the cold call) and then its other pair: the figure for one pair.  Then the large system merges all its pairs in one call.
Each call is timed by HIP events on the system's stream (vslam_get_merge_timing).  The bytes moved are counted from the read-back counts:
everything copied is read and written, the zeroed cells of the measurement table's cross blocks, cur_meas and pt_level are written only.
One JSON line per measurement.

    python tools/merge_cost.py --streams 3072
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pair_bytes(w, h, nk_d, np_d, nk_s, np_s):
    """bytes one pair moves in a system without grow_map, relocalise and idle jobs"""
    img = sum(((((w >> l) + 63) // 64) * 64) * (h >> l) for l in range(4))        # a keyframe's pyramid: the pitch is a multiple of 64
    copied = nk_s * (img + 96 + 16) + np_s * (104 + 168 + 128 + 4) + nk_s * np_s * 24
    zeroed = (nk_d * np_s + nk_s * np_d) * 24 + np_s * (24 + 4) + nk_s * 4
    return 2 * copied + zeroed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    args = ap.parse_args()
    S, W, H = args.streams - args.streams % 2, args.width, args.height
    import numpy as np
    from helpers import make_scene
    from visualslam_android_amd import capi
    n_kf = 4
    base = [make_scene(W, H, seed=700 + k, n_frames=1, n_keyframes=n_kf) for k in range(3)]

    def system(n):
        g = capi.System(capi.default_params(W, H, n, patch_size=8, max_keyframes=2 * n_kf))
        for s in range(n):
            f, m, _fr = base[(s // 2) % 3]
            g.load_map(s, m); g.set_pose(s, f.pose(-1))
        g.synchronize()
        return g

    def report(g, dst, src, tag):
        counts = [(g.state(d).n_keyframes, g.state(d).n_points, g.state(s).n_keyframes, g.state(s).n_points) for d, s in zip(dst[:6], src[:6])]
        per = [pair_bytes(W, H, *c) for c in counts]                 # the scenes cycle with period 3 over the pairs
        total = sum(per[i % len(per)] for i in range(len(dst)))
        g.merge_maps(dst, src)
        ms = g.merge_timing()
        print(json.dumps({"merge": tag, "pairs": len(dst), "keyframes": "%d + %d" % (counts[0][0], counts[0][2]), "points_first_pairs": [(c[1], c[3]) for c in counts[:3]],
                          "merge_ms": round(ms, 4), "bytes_moved": total, "GB_per_s": round(total / (ms * 1e-3) / 1e9, 1)}), flush=True)

    small = system(4)
    report(small, [0], [1], "cold call, one pair")
    report(small, [2], [3], "one pair")
    small.close()
    g = system(S)
    report(g, np.arange(0, S, 2, dtype=np.int32), np.arange(1, S, 2, dtype=np.int32), "all pairs")
    assert g.merge_info(S - 2)["keyframes"] == n_kf and g.state(S - 2).n_keyframes == 2 * n_kf
    g.close()


if __name__ == "__main__":
    main()
