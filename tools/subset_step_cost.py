#!/usr/bin/env python3
"""Cost of a subset step against a full step of the same system ("Subset steps").

One system shaped like bench.py's default line (640 x 480, patch 8, asynchronous map-maker with ba_delay_frames = 16, keyframe phases
staggered over 21 frames, frames resident in device memory) but with three seeded scenes cycled over the streams, steps through four
modes in turn:
    full      vslam_track_frame                       (every stream, the list-free path)
    all       vslam_track_frame_subset listing every stream
    half      ... listing S/2 streams (stream s in step j when s % 2 == j % 2)
    quarter   ... listing S/4 streams (s % 4 == j % 4)
Every stream consumes its own frames in order whatever the mode.  Per mode: one untimed step of the shape, K steps enqueued back to
back between two host clocks that end in a device synchronise (ms per step), then K steps under vslam_profile_begin / _end (HIP events
per stage, ms per step).  One JSON line per mode.

    python tools/subset_step_cost.py --streams 3072 --steps 8
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MODES = (("full", 1), ("all", 1), ("half", 2), ("quarter", 4))


def plan(S, K, warm_full):
    """-> per mode the list of steps, each (streams or None for the full call); and the own frames every stream needs"""
    import numpy as np
    own = np.zeros(S, np.int64) + warm_full
    steps = {}
    allv = np.arange(S)
    for name, mod in MODES:
        steps[name] = []
        for j in range(1 + 2 * K):
            idx = allv[allv % mod == j % mod]
            steps[name].append((None if name == "full" else idx.astype(np.int32), own[idx].copy(), idx))
            own[idx] += 1
    return steps, int(own.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=3072)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--dry", action="store_true", help="plan only (no device)")
    args = ap.parse_args()
    S, K, W, H = args.streams, args.steps, args.width, args.height
    steps, n_frames = plan(S, K, args.warmup)
    if args.dry:
        print(json.dumps({"frames_per_stream": n_frames, "steps": {k: [len(x[2]) for x in v] for k, v in steps.items()}}))
        return
    import numpy as np
    import torch
    from helpers import make_scene
    from visualslam_android_amd import capi
    base = [make_scene(W, H, seed=700 + k, n_frames=n_frames) for k in range(3)]
    base_dev = torch.stack([torch.from_numpy(np.ascontiguousarray(b[2])) for b in base]).cuda()      # [3][n_frames][H][W]
    scene_of = torch.arange(S, device="cuda") % 3
    stagger, delay = 21, 16
    g = capi.System(capi.default_params(W, H, S, patch_size=8, ba_delay_frames=delay, ba_batch_frames=10))
    for s in range(S):
        f, m, _fr = base[s % 3]
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
        g.set_last_keyframe_dropped(s, -20 + (s * stagger) // S)

    def gather(idx, own):
        i = torch.from_numpy(idx).cuda()
        return base_dev[scene_of[i], torch.from_numpy(own).cuda()].contiguous()

    def run(step, buf):
        if step[0] is None:
            g.track_frame_device(buf.data_ptr(), W, H * W)
        else:
            g.track_frame_subset_device(step[0], buf.data_ptr(), W, H * W)

    allv = np.arange(S)
    for t in range(args.warmup):
        buf = gather(allv, np.full(S, t, np.int64))
        g.track_frame_device(buf.data_ptr(), W, H * W)
        g.synchronize()
    for name, _mod in MODES:
        st = steps[name]
        bufs = [gather(x[2], x[1]) for x in st]
        torch.cuda.synchronize()
        run(st[0], bufs[0]); g.synchronize()                           # the shape's first step: untimed
        t0 = time.perf_counter()
        for j in range(1, 1 + K):
            run(st[j], bufs[j])
        g.synchronize()
        wall = 1e3 * (time.perf_counter() - t0) / K
        g.profile_begin(K)
        for j in range(1 + K, 1 + 2 * K):
            run(st[j], bufs[j])
        ms, n = g.profile_end()
        assert n == K
        stage = {k: round(v / K, 4) for k, v in ms.items()}
        fe = stage["pyr_fast0"] + stage["fast_lvl"] + stage["compact"]
        print(json.dumps({"mode": name, "streams_per_step": int(len(st[1][2])), "of": S, "steps": K, "wall_ms_per_step": round(wall, 4),
                          "front_end_ms": round(fe, 4), "tracker_and_mapmaker_ms": round(sum(stage.values()) - fe - stage["ba_compute"], 4),
                          "stage_ms_per_step": stage}), flush=True)
        del bufs
    kf = sum(st_.n_keyframes for st_ in g.states()) - sum(len(base[s % 3][1]["keyframes"]) for s in range(S))
    fr = [st_.frame for st_ in g.states()]
    print(json.dumps({"keyframes_added": int(kf), "own_frames_min": int(min(fr)), "own_frames_max": int(max(fr))}), flush=True)
    g.close()


if __name__ == "__main__":
    main()
