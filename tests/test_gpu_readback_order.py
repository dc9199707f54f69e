"""GPU: a read-back issued straight behind queued work returns what it returns after a synchronize.

A handle's streams are non-blocking, so nothing but the stream a copy is enqueued on orders it behind the kernels before it: that is
what the HostCopy primitives of csrc/vslam_internal.h are for ("Host copies").  Every read-back waits for its
stream, so only the FIRST one after queued work can be early; each family therefore gets queued work of its own in front of it.

Shown to have teeth on a scratch build whose vslam_get_states and bundle result read copy on the null stream and wait for nothing
(profiles/r07_host_waits.txt): both tests fail their first comparison, nothing faults."""
import ctypes as C

import numpy as np
import pytest
import torch

from ba_scene import ba_scene
from helpers import make_scene
from test_gpu_bundle import load
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

W, H, S = 640, 480, 8
FRAMES_PER_ROUND = 3


def blob(x):
    """bytes of whatever a read-back wrapper returns"""
    if isinstance(x, dict):
        return b"".join(blob(x[k]) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return b"".join(blob(v) for v in x)
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, (C.Structure, C.Array)):
        return bytes(x)
    return repr(x).encode()


SYSTEM_READS = [
    ("states", lambda g: g.states()),
    ("points", lambda g: g.points(1)),
    ("keyframe pose", lambda g: g.keyframe_pose(2, 5)),
    ("keyframe measurements", lambda g: g.keyframe_meas(3, 4)),
    ("templates", lambda g: g.templates(4)),
    ("bundle stats", lambda g: g.bundle_stats(5)),
    ("search plan", lambda g: g.search_plan(6)),
    ("corners", lambda g: [g.read_corners(7, l) for l in range(4)]),
    ("level image", lambda g: g.read_level_image(0, 1)),
    # entry points no other test calls: the keyframe-distance members and the launch totals
    ("need_new_keyframe", lambda g: (g.need_new_keyframe(1), g.distance_to_nearest_keyframe_excessive(1))),
    ("launch totals", lambda g: g.ba_launch_totals()),
    ("reset info", lambda g: g.reset_info(7)),      # last: its round resets stream 7
]


def test_system_readbacks_behind_queued_work():
    rounds = len(SYSTEM_READS)
    f, m, frames = make_scene(W, H, seed=31, n_frames=rounds * FRAMES_PER_ROUND, n_keyframes=8, per_level=(25, 9, 3, 1))
    assert len(m["keyframes"]) == 8 and 250 <= len(m["packed"]["pos"]) <= 350          # per_level is per keyframe
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()[:, None].repeat(1, S, 1, 1).contiguous()   # [frame][S][H][W]
    torch.cuda.synchronize()
    g = capi.System(capi.default_params(W, H, S))
    for s in range(S):
        g.load_map(s, m)
        g.set_pose(s, f.pose(-1))
    g.synchronize()
    t = 0
    for name, read in SYSTEM_READS:
        for _ in range(FRAMES_PER_ROUND):                           # back to back, from device memory, nothing waits
            g.track_frame_device(dev[t].data_ptr(), W, H * W)
            t += 1
        if name == "reset info":
            g.reset([7])
        capi._check(g.lib.vslam_bundle_adjust_all(g.h))             # host-driven, not waited for (System.bundle_adjust_all would)
        early = blob(read(g))
        g.synchronize()
        assert early == blob(read(g)), name
    st = g.states()
    assert all(x.frame == t for x in st[:7]) and st[7].frame == 0 and st[0].n_keyframes >= 8   # the queued work did run
    g.close()


BUNDLE_READS = [
    ("result", lambda b, n: b.result(n)),
    ("cameras", lambda b, n: b.cameras(n)),
    ("points", lambda b, n: b.points(n)),
    ("outlier_meas", lambda b, n: b.outlier_meas(n)),
    ("outlier_points", lambda b, n: b.outlier_points(n)),
    ("timing counters", lambda b, n: b.timing()[1]),                # (no other test calls vslam_bundle_get_timing)
]


def test_bundle_readbacks_behind_a_queued_compute():
    N = 4
    b = capi.Bundle(capi.default_params(W, H, 1, ba_max_iterations=10), N, 5, 300, 1500)
    for n in range(N):
        load(b, ba_scene(5, 300, seed=40 + n), problem=n)
    for name, read in BUNDLE_READS:
        b.compute(sync=False)                                       # every compute starts again from the caller's values
        early = [blob(read(b, n)) for n in (N - 1, 0)]
        b.synchronize()
        assert early == [blob(read(b, n)) for n in (N - 1, 0)], name
    assert all(b.result(n)["accepted"] > 0 and b.result(n)["trials"] > 0 for n in range(N))
    assert len(b.outlier_meas(0)) > 0
    b.close()
