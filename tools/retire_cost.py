#!/usr/bin/env python3
"""Cost of keyframe retirement in a step ("Keyframe retirement").

One system shaped like bench.py's default line (640 x 480, patch 8, asynchronous map-maker with ba_delay_frames = 16, keyframe phases
staggered over 21 frames, frames resident in device memory), three seeded scenes cycled over the streams, the same frames twice:
    roomy      max_keyframes large enough never to fill, keyframe_retire = 0
    retiring   max_keyframes = the uploaded map's keyframes, keyframe_retire = 1: every keyframe request of a stream retires one first,
               about S / 21 streams per step
Per run: `warmup` untimed steps, then `steps` steps enqueued back to back between two host clocks that end in a device synchronise
(ms per step).  Afterwards, on the retiring system, the pending adjustments are drained and vslam_retire_keyframes is called for
S / 21 streams and for one stream (HIP events, vslam_get_retire_timing).  One JSON line per measurement.

    python tools/retire_cost.py --streams 3072 --steps 21
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STAGGER, DELAY = 21, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--steps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--dry", action="store_true", help="plan only (no device)")
    args = ap.parse_args()
    S, K, W, H = args.streams, args.steps, args.width, args.height
    n_frames = args.warmup + K
    n_kf = 8
    roomy = n_kf + (n_frames + STAGGER - 1) // STAGGER + 1
    if args.dry:
        print(json.dumps({"frames_per_stream": n_frames, "max_keyframes": {"roomy": roomy, "retiring": n_kf}, "retirements_per_step": S / STAGGER}))
        return
    import numpy as np
    import torch
    from helpers import make_scene
    from visualslam_android_amd import capi
    base = [make_scene(W, H, seed=700 + k, n_frames=n_frames, n_keyframes=n_kf) for k in range(3)]
    base_dev = torch.stack([torch.from_numpy(np.ascontiguousarray(b[2])) for b in base]).cuda()      # [3][n_frames][H][W]
    scene_of = torch.arange(S, device="cuda") % 3
    for name, kw in (("roomy", dict(max_keyframes=roomy, keyframe_retire=0)), ("retiring", dict(max_keyframes=n_kf, keyframe_retire=1))):
        g = capi.System(capi.default_params(W, H, S, patch_size=8, ba_delay_frames=DELAY, ba_batch_frames=10, **kw))
        for s in range(S):
            f, m, _fr = base[s % 3]
            g.load_map(s, m); g.set_pose(s, f.pose(-1))
            g.set_last_keyframe_dropped(s, -20 + (s * STAGGER) // S)
        bufs = [base_dev[scene_of, t].contiguous() for t in range(n_frames)]
        torch.cuda.synchronize()
        for t in range(args.warmup):
            g.track_frame_device(bufs[t].data_ptr(), W, H * W)
        g.synchronize()
        t0 = time.perf_counter()
        for t in range(args.warmup, n_frames):
            g.track_frame_device(bufs[t].data_ptr(), W, H * W)
        g.synchronize()
        wall = 1e3 * (time.perf_counter() - t0) / K
        st = g.states()
        added = sum(x.n_keyframes for x in st) - S * n_kf
        retired = sum(g.retire_info(s)["retired"] for s in range(0, S, max(1, S // 64))) if name == "retiring" else 0
        print(json.dumps({"run": name, "streams": S, "steps": K, "max_keyframes": kw["max_keyframes"], "wall_ms_per_step": round(wall, 4),
                          "net_keyframes_added": int(added), "good": int(sum(x.quality == 2 for x in st)),
                          "retirements_in_a_sample_of_streams": int(retired)}), flush=True)
        if name == "retiring":
            g.bundle_adjust_recent()                                   # drains every pending adjustment: no stream refuses the explicit call
            g.synchronize()
            for n in (max(1, S // STAGGER), 1):
                g.retire_keyframes(np.arange(n, dtype=np.int32) * (S // n if n > 1 else 1))
                print(json.dumps({"explicit_call_streams": n, "retire_ms": round(g.retire_timing(), 4)}), flush=True)
        del bufs
        g.close()


if __name__ == "__main__":
    main()
