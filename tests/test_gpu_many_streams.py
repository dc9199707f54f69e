"""GPU parity at stream counts where the launch plans change (many_stream_cases.py): the front end's strip heights 24..64, the
asynchronous map-maker's work list past its grid of 2 n_cu workgroups, the one-lane-per-stream kernels past their first workgroup of 64,
and byte offsets past 2^31 and 2^32.

The method throughout: K = 3 scenes (frames) go to the oracle; S streams replicate them by many_stream_cases.replica, which never puts
one scene in neighbouring streams.  The library's sums are deterministic (no floating-point atomics), so (a) every replica must equal,
bit for bit, its scene's stream in a K-stream control system run in the same test on the small-S plan the rest of the suite pins to the
oracle, (b) the control is held to the oracle at the bars the existing tests use for its mode, and (c) a fixed set of streams of the
large system (many_stream_cases.fixed_streams) is compared with the oracle directly."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import many_stream_cases as mc
import oracle.binding as orc
import overlay_ref as ov
from helpers import assert_map_close, assert_map_exact, assert_tracker_close, assert_tracker_exact, make_oracle, make_scene, pose_err
from test_gpu_frontend_shapes import check_all, reference, strip_eligible, synth_frames
from visualslam_android_amd import capi, feeder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = mc.K


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def replica_index(S):
    idx = [mc.replica(s) for s in range(S)]
    assert all(a != b for a, b in zip(idx, idx[1:]))
    return idx


# ---- 1. the front end at every strip height ------------------------------------------------------------------------------------------
FE_SEEDS = (9, 10, 11)
FE_SMALL = dict(max_points=64, max_keyframes=1)          # the tracker's arrays are not used here: keep them light


def fe_caps(refs_all, w, h):
    """corner capacity per level: twice the most the oracle finds in any frame that is fed (the default, half the pixels, is 36 B per
    entry and stream: 12 GB at 911 streams of 2080x250)"""
    return [max(256, 2 * max(len(r[l][1]) for r in refs_all)) for l in range(4)]


@pytest.mark.parametrize("case", range(len(mc.FE_SWEEP)), ids=["%dx%d-launch%d-R%d" % c for c in mc.FE_SWEEP])
def test_frontend_at_every_strip_height(oracle, case):
    """Every stream of S, S the smallest count at which the case's launch runs strips R high on this device: level images, corner lists,
    row LUTs, scores, maximal corners and Shi-Tomasi candidates == the oracle's for the stream's frame.  The frames are fed from device
    memory, 16-B aligned and tight (the strip form), after two other frames have gone through both front-end buffers."""
    import torch
    w, h, launch, R = mc.FE_SWEEP[case]
    assert strip_eligible(w, h)
    S = mc.smallest_streams(w, h, n_cu(), launch)[R]
    assert mc.pick(w, h, S, n_cu())[launch] == R and S > K
    frames = synth_frames(FE_SEEDS, w, h)
    other = synth_frames([s + 50 for s in FE_SEEDS], w, h)
    refs = [reference(oracle, ("synth", s, w, h), frames[i]) for i, s in enumerate(FE_SEEDS)]
    refs_other = [reference(oracle, ("synth", s + 50, w, h), other[i]) for i, s in enumerate(FE_SEEDS)]
    for ref in refs:                                                 # not vacuous: corners on every level that has a FAST row, candidates on one
        assert all(len(ref[l][1]) > 0 for l in range(4) if (h >> l) >= 7), [len(ref[l][1]) for l in range(4)]
        assert sum(len(ref[l][5]) for l in range(4)) > 0
    idx = replica_index(S)
    tidx = torch.tensor(idx, device="cuda")
    g = capi.System(capi.default_params(w, h, S, max_corners=fe_caps(refs + refs_other, w, h), **FE_SMALL))
    d_other = torch.from_numpy(other).cuda()
    for perm in (tidx, (tidx + 1) % K):                              # both buffers hold another frame's masks, counts and lists
        dev = d_other[perm].contiguous()
        torch.cuda.synchronize()                                     # the gather runs on torch's stream, the front end on the library's
        g.make_keyframe_lite_device(dev.data_ptr(), w, w * h)
        g.synchronize()
    dev = torch.from_numpy(frames).cuda()[tidx].contiguous()
    assert dev.data_ptr() % 16 == 0 and dev.shape == (S, h, w)
    torch.cuda.synchronize()
    g.make_keyframe_lite_device(dev.data_ptr(), w, w * h)
    g.synchronize()
    check_all(g, [refs[k] for k in idx], (w, h, S, R))
    g.close()


_FE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from visualslam_android_amd import capi
for arg in sys.argv[2:]:
    w, h, S = (int(x) for x in arg.split(","))
    g = capi.System(capi.default_params(w, h, S, max_corners=[256] * 4, max_points=64, max_keyframes=1))
    buf = torch.zeros(S * w * h, dtype=torch.uint8, device="cuda")   # a flat frame: no corner, nothing overflows
    g.make_keyframe_lite_device(buf.data_ptr(), w, w * h)
    g.synchronize()
    g.close()
    del buf
print("child done")
"""


def test_the_sweep_runs_the_heights_it_names():
    """fe_launch_slide's own account (VSLAM_FE_DEBUG, read once per process, hence the child) of the (w, h, S) of the sweep: the heights
    of both launches equal the restatement's, the sweep's cases cover 24..64 on level 0 and 24, 40, 48, 64 on levels 1..3 -- on a device
    with another compute-unit count the sweep asks for other S, and this test says whether they took."""
    plan = mc.sweep_plan(n_cu())
    env = dict(os.environ, VSLAM_FE_DEBUG="1")
    env.pop("VSLAM_FE_BANDS", None)
    out = subprocess.run([sys.executable, "-c", _FE_CHILD, ROOT] + ["%d,%d,%d" % p[:3] for p in plan], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0 and "child done" in out.stdout, out.stderr[-2000:]
    lines = [l for l in out.stderr.splitlines() if l.startswith("fe slide:")]
    print("\n".join(lines))
    assert len(lines) == len(plan), out.stderr[-2000:]
    seen0, seen1 = set(), set()
    for line, (w, h, S, R) in zip(lines, plan):
        m = re.match(r"fe slide: S (\d+) n_cu (\d+) R (\d+) (\d+) (\d+) (\d+) ", line)
        got = [int(x) for x in m.groups()]
        assert got[0] == S and got[1] == n_cu(), line
        assert got[2] == R[0] and got[3:] == [R[1]] * 3, (line, R)
        seen0.add(got[2]); seen1.add(got[3])
    assert seen0 >= set(mc.LEVEL0_HEIGHTS) and seen1 >= set(mc.LEVELS_HEIGHTS), (seen0, seen1)


# ---- 2. tracker and map-maker at S = 2 n_cu + 65 -------------------------------------------------------------------------------------
TW, TH = 320, 240
_scenes = {}


def scenes(n_frames, per_level=(120, 50, 20, 8)):
    """per_level (120, 50, 20, 8): the scenes of the asynchronous tests of test_gpu_tracking.py, about 1560 points"""
    if (n_frames, per_level) not in _scenes:
        _scenes[n_frames, per_level] = [make_scene(TW, TH, seed=900 + k, n_frames=n_frames, per_level=per_level) for k in range(K)]
    return _scenes[n_frames, per_level]


def build(S, sc, phases, **kw):
    """a system of S streams, stream s on scene replica(s) (S = K: the control, stream k on scene k)"""
    g = capi.System(capi.default_params(TW, TH, S, **kw))
    for s in range(S):
        f, m, _fr = sc[mc.replica(s) if S > K else s]
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
        if phases is not None:
            g.set_last_keyframe_dropped(s, phases[mc.replica(s) if S > K else s])
    return g


def device_frames(sc, n, idx):
    import torch
    base = torch.from_numpy(np.stack([x[2][:n] for x in sc])).cuda()             # [K, n, h, w]
    big = base[torch.tensor(idx, device="cuda")].transpose(0, 1).contiguous()     # [n, S, h, w]
    ctl = base.transpose(0, 1).contiguous()
    torch.cuda.synchronize()                                                      # before the library's streams read them
    return big, ctl


def assert_replicas_equal_control(g, c, idx, tag):
    big, ctl = g.states(), [bytes(x) for x in c.states()]
    bad = [s for s, x in enumerate(big) if bytes(x) != ctl[idx[s]]]
    assert not bad, (tag, bad[:10], len(bad))


def assert_snapshots_equal_control(g, c, idx, streams=None):
    ctl = [c.snapshot(k).tobytes() for k in range(K)]
    assert len(set(ctl)) == K
    for s in (range(g.S) if streams is None else streams):
        assert g.snapshot(s).tobytes() == ctl[idx[s]], s            # nothing in the blob depends on the slot (snapshot_format.h)


ASYNC = {                                # name: (ba_delay_frames, frames, last-keyframe phases per scene or None)
    "lockstep": (3, 18, None),           # every stream keyframes on frames 0 and 13: launches of S > 2 n_cu problems
    "staggered": (6, 24, (-12, -8, -4)),  # keyframe frames 0, 13 / 4, 17 / 8, 21: a launch holds about S / 3 problems, fewer than the grid
}


@pytest.mark.parametrize("mode", list(ASYNC))
def test_asynchronous_mapmaker_past_its_grid(mode):
    """ba_delay_frames > 0, batches of one frame, fast sums, S = 2 n_cu + 65: k_ba_compute's grid is 2 n_cu workgroups and the rest of
    the work list is drawn from the counter.  Bars of test_asynchronous_mapmaker_streams_keyframing_on_different_frames for the control
    and the fixed set; replicas == control in every frame and, at the end, in every stream's snapshot."""
    D, n, phases = ASYNC[mode]
    ncu = n_cu()
    S = mc.tracker_streams(ncu)
    idx = replica_index(S)
    fixed = mc.fixed_streams(S, ncu)
    sc = scenes(n)
    kw = dict(ba_delay_frames=D, ba_batch_frames=1, min_frames_between_kf=12, max_keyframes=12, max_points=2048)
    g, c = build(S, sc, phases, **kw), build(K, sc, phases, **kw)
    oracles = []
    for k, (f, m, _fr) in enumerate(sc):
        o = make_oracle(capi.default_params(TW, TH, 1, **kw), m, f.pose(-1))
        if phases is not None:
            o.set_last_keyframe_dropped(phases[k])
        oracles.append(o)
    big, ctl = device_frames(sc, n, idx)
    kf_frames = [[] for _ in range(K)]
    first_landed = [None] * K
    for t in range(n):
        g.track_frame_device(big[t].data_ptr(), TW, TW * TH)
        c.track_frame_device(ctl[t].data_ptr(), TW, TW * TH)
        g.synchronize(); c.synchronize()
        for k in range(K):
            oracles[k].track_frame(sc[k][2][t])
            if oracles[k].state().kf_added:
                kf_frames[k].append(t)
        assert_replicas_equal_control(g, c, idx, (mode, t))
        for sys_, streams in ((c, list(range(K))), (g, fixed)):
            for s in streams:
                k = s if sys_ is c else idx[s]
                o, tag = oracles[k], "%s stream %d frame %d" % (mode, s, t)
                so, sg = o.state(), sys_.state(s)
                assert so.kf_added == sg.kf_added and so.n_keyframes == sg.n_keyframes, tag
                if not kf_frames[k] or t < kf_frames[k][0] + D:
                    assert_tracker_exact(o, sys_, s, tag)            # nothing has touched the map yet
                else:
                    assert_tracker_close(o, sys_, s, tag)
        if mode == "lockstep" and t == 0:
            tot = g.ba_launch_totals()
            print("ba launch totals after frame 0:", tot, "S", S, "n_cu", ncu)
            assert all(kf == [0] for kf in kf_frames)
            assert tot["launches"] == 1 and tot["problems"] == S > 2 * ncu, (tot, S, ncu)
    assert all(len(kf) >= 2 for kf in kf_frames), kf_frames
    if mode == "staggered":
        assert len({kf[0] for kf in kf_frames}) == K, kf_frames      # different frames: no launch holds more than two scenes' streams
    g.synchronize(); c.synchronize()
    tot = g.ba_launch_totals()
    print("ba launch totals at the end:", tot)
    assert tot["problems"] == sum(len(kf_frames[idx[s]]) for s in range(S)), (tot, kf_frames)
    for sys_, streams in ((c, list(range(K))), (g, fixed)):
        for s in streams:
            o = oracles[s if sys_ is c else idx[s]]
            assert sys_.state(s).n_ba_trials == o.state().n_ba_trials > 0, s
            for kf in range(sys_.state(s).n_keyframes):
                assert pose_err(o.keyframe_pose(kf), sys_.keyframe_pose(s, kf)) < 1e-5, (s, kf)
    g.bundle_adjust_recent(); c.bundle_adjust_recent()               # collects what is still in flight, then one more adjustment: a stream
    assert_replicas_equal_control(g, c, idx, (mode, "end"))          # with an adjustment pending cannot be saved
    assert_snapshots_equal_control(g, c, idx)
    g.close(); c.close()


def stream_dump(g, s):
    """what a caller can read of a stream's result, as bytes (test_gpu_reset.dump)"""
    st = g.state(s)
    p = g.points(s)
    return (bytes(st), p["pos"].tobytes(), p["bad"].tobytes(), p["n_in"].tobytes(), p["n_out"].tobytes(),
            b"".join(g.keyframe_pose(s, k).tobytes() for k in range(st.n_keyframes)))


def new_stream_read(x, s):
    """read-backs of a stream that has no map (test_gpu_reset.test_read_backs_after_the_reset_equal_a_new_systems)"""
    out = [bytes(x.state(s)), x.points(s)["pos"].shape, x.idle_stats(s), x.bundle_stats(s), x.init_info(s), x.message(s),
           x.keyframe_pose(s, 0).tobytes(), x.keyframe_pose(s, 9).tobytes(), x.keyframe_corners(s, 3, 0).tobytes()]
    t = x.templates(s, 64)
    return out + [t[k].tobytes() for k in ("tmpl", "sum", "sumsq", "bad", "have")]


def test_synchronous_mapmaker_reference_order_sums():
    """ba_sum_order = 1, synchronous map-maker, grow_map = 3, created with a PVS shuffle seed that k_set_pvs_seed then sets to 0, the
    identity order, in every stream (a stream it missed would keep the shuffle, sum its pose update in another order and differ from the
    oracle, which has no shuffle, in the last bits), S = 2 n_cu + 65: the free_exact bars of test_gpu_tracking.run_streams --
    tracker == oracle in every frame, the whole map after each keyframe -- on the control and the fixed set, replicas == control; a
    further keyframe is asked for by the host (k_request_keyframe; the oracle has no such entry point: replicas == control).  Then
    render_overlay past the first workgroup of k_overlay_note / k_overlay_forget against overlay_ref.py, and reset_streams at the
    workgroup edges.  (The scenes are sparser than the asynchronous tests', which leave no room for the new keyframe to add points.)"""
    n = 4
    ncu = n_cu()
    S = mc.tracker_streams(ncu)
    idx = replica_index(S)
    fixed = mc.fixed_streams(S, ncu)
    sc = scenes(n, per_level=(40, 20, 10, 4))                        # about 590 points, 780 after the growth: sparse enough for the new keyframe to add points
    kw = dict(ba_sum_order=1, grow_map=3, pvs_shuffle_seed=77, max_keyframes=12, max_points=2048, overlay=1)
    g, c = build(S, sc, None, **kw), build(K, sc, None, **kw)
    g.set_pvs_seed(-1, 0); c.set_pvs_seed(-1, 0)
    oracles = [make_oracle(capi.default_params(TW, TH, 1, **kw), m, f.pose(-1)) for f, m, _fr in sc]
    big, ctl = device_frames(sc, n, idx)

    def check(t):
        assert_replicas_equal_control(g, c, idx, t)
        for sys_, streams in ((c, list(range(K))), (g, fixed)):
            for s in streams:
                o, tag = oracles[s if sys_ is c else idx[s]], "stream %d frame %s" % (s, t)
                assert_tracker_exact(o, sys_, s, tag)
                if o.state().kf_added:
                    assert_map_exact(o, sys_, s, tag)

    for t in range(n):
        g.track_frame_device(big[t].data_ptr(), TW, TW * TH)
        c.track_frame_device(ctl[t].data_ptr(), TW, TW * TH)
        g.synchronize(); c.synchronize()
        for k in range(K):
            oracles[k].track_frame(sc[k][2][t])
        check(t)
    base = [len(x[1]["keyframes"]) for x in sc]
    assert all(c.state(k).n_keyframes == base[k] + 1 and c.state(k).n_points > len(sc[k][1]["points"]) for k in range(K))   # frame 0's keyframe grew the map
    g.add_keyframe_now(-1); c.add_keyframe_now(-1)                   # the oracle binding has no host-driven AddKeyFrame: replicas == control only
    assert_replicas_equal_control(g, c, idx, "request")
    assert all(c.state(k).n_keyframes == base[k] + 2 for k in range(K))
    assert_snapshots_equal_control(g, c, idx)

    # the overlay of streams past lane 63: the reference image from the stream's read-backs, and the control's image of the same scene
    flags = capi.DRAW_POINTS | capi.DRAW_TRAILS | capi.DRAW_FAST
    drawn = [64, 65, S - 1]
    got = g.render_overlay(drawn, flags)
    for i, s in enumerate(drawn):
        want, counts = ov.render_stream(g, s, flags)
        assert counts[0] > 50 and np.array_equal(got[i], want), (s, counts, int((got[i] != want).any(-1).sum()))
        info = g.overlay_info(s)
        assert (info["discs"], info["lines"], info["marks"]) == counts and info["track_map_frame"] == n, (s, info)
        assert np.array_equal(got[i], c.render_overlay([idx[s]], flags)[0]), s
    assert not np.array_equal(got[0], got[1])

    # reset_streams at the edges of the 64-lane workgroups: the listed streams read as a new system's, their neighbours keep every bit
    listed = [0, 63, 64, 65, S - 1]
    keep = {s: stream_dump(g, s) for s in (62, 66, S - 2)}
    g.reset(listed)
    new = capi.System(capi.default_params(TW, TH, 1, **kw))
    want = new_stream_read(new, 0)
    for s in listed:
        assert new_stream_read(g, s) == want, s
        assert g.reset_info(s)["resets"] == 1
    for s, d in keep.items():
        assert stream_dump(g, s) == d and g.reset_info(s)["resets"] == 0, s
    new.close(); g.close(); c.close()


# ---- 3. offsets past 2^31 and 2^32 bytes ---------------------------------------------------------------------------------------------
def test_callers_buffer_with_a_stream_stride_past_4_gib(oracle):
    """Three streams in one device buffer whose stream_stride is 2^31 + 4096: stream 1 starts above 2^31 and stream 2 above 2^32 bytes.
    16-B aligned (the strip form) and the same frames one byte further on (the band form); only the frames are written."""
    import torch
    w, h = 224, 100
    assert strip_eligible(w, h)
    seeds = (20, 21, 22)
    frames = synth_frames(seeds, w, h)
    refs = [reference(oracle, ("synth", s, w, h), frames[i]) for i, s in enumerate(seeds)]
    sstride = (1 << 31) + 4096
    assert sstride % 16 == 0 and sstride > (1 << 31) and 2 * sstride > (1 << 32)
    buf = torch.empty(2 * sstride + w * h + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    g = capi.System(capi.default_params(w, h, 3, **FE_SMALL))
    for off in (0, 1):
        for s in range(3):
            buf[off + s * sstride: off + s * sstride + w * h].copy_(torch.from_numpy(frames[s].reshape(-1)))
        torch.cuda.synchronize()
        g.make_keyframe_lite_device(buf.data_ptr() + off, w, sstride)
        g.synchronize()
        check_all(g, refs, (w, h, "offset", off))
    g.close()
    del buf


def test_library_arrays_past_4_gib():
    """640x480 with 128 keyframe slots: a stream owns 39 MB of kf_img[0], so the streams of mc.offset_streams start beyond 2^31 and 2^32
    bytes in it.  The same scene in stream 0, the streams around both marks and the last; a keyframe on
    frame 0 (k_add_keyframe writes slot 8 of each), map growth, relocaliser on, reference-order sums: stream 0 == the oracle, the
    others == stream 0 bit for bit, snapshot included."""
    import torch
    w, h, KF, n = 640, 480, 128, 3
    S, streams = mc.offset_streams(w, h, KF)
    f, m, frames = make_scene(w, h, seed=1234, n_frames=n)
    kw = dict(ba_sum_order=1, grow_map=3, relocalise=1, max_keyframes=KF)
    o = make_oracle(capi.default_params(w, h, 1, **kw), m, f.pose(-1))
    g = capi.System(capi.default_params(w, h, S, **kw))
    for s in streams:
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
    dev = torch.from_numpy(frames[:n]).cuda()
    for t in range(n):
        one = dev[t].expand(S, h, w).contiguous()
        torch.cuda.synchronize()
        g.track_frame_device(one.data_ptr(), w, w * h)
        g.synchronize()
        o.track_frame(frames[t])
        assert_tracker_exact(o, g, 0, "frame %d" % t)
        if o.state().kf_added:
            assert_map_exact(o, g, 0, "frame %d" % t)
        st = g.states()
        for s in streams[1:]:
            assert bytes(st[s]) == bytes(st[0]), (s, t)
    assert g.state(0).n_keyframes == len(m["keyframes"]) + 1 and g.state(0).n_points > len(m["points"])
    kf_new = len(m["keyframes"])
    byte0 = [s * mc.keyframe_image_stride(w, h, 0, KF) + kf_new * mc.keyframe_image_stride(w, h, 0, 1) for s in streams]
    print("kf_img[0] byte offsets of the new keyframe:", dict(zip(streams, byte0)))
    assert byte0[-1] > (1 << 32)
    snap = g.snapshot(0).tobytes()
    for s in streams[1:]:
        assert g.snapshot(s).tobytes() == snap, s
    g.close()


def test_measurement_tables_past_4_gib():
    """kf_meas is [S][max_keyframes][max_points] of 24 B: with 128 keyframe slots and 4096 points a stream owns 12 MB, and the streams of
    mc.measurement_offset_streams start beyond 2^31 and 2^32 bytes in it -- the only other per-stream array that can pass 2^32 within
    about ten gigabytes.  A small frame keeps the images light; the system measures 13.8 GB, most of it the bundle-adjustment
    pool, and no smaller one puts a stream past 2^32 here (both capacities are at their maxima).  The same scene in stream 0, the streams around both marks and the
    last: the map upload writes their rows, frame 0's keyframe adds a row and grows the map, the adjustment reads and rewrites them.
    Fast sums (the reference-order workspace, 592 B per measurement slot, would add 13 GB here): stream 0 against the oracle at the bars
    of the fast mode -- the tracker exact in the keyframe's frame, the map within 1e-7 after it, assert_tracker_close from then on --
    and the others == stream 0 bit for bit: states, every measurement row, the snapshot."""
    import torch
    w, h, KF, P, n = 128, 96, 128, 4096, 3
    S, streams = mc.measurement_offset_streams(KF, P)
    f, m, frames = make_scene(w, h, seed=1234, n_frames=n, per_level=(40, 12, 4, 1))
    kw = dict(grow_map=3, max_keyframes=KF, max_points=P)
    o = make_oracle(capi.default_params(w, h, 1, **kw), m, f.pose(-1))
    free0 = torch.cuda.mem_get_info()[0]
    g = capi.System(capi.default_params(w, h, S, **kw))
    print("device memory of the system: %.2f GB" % ((free0 - torch.cuda.mem_get_info()[0]) / 1e9))
    for s in streams:
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
    dev = torch.from_numpy(frames[:n]).cuda()
    for t in range(n):
        one = dev[t].expand(S, h, w).contiguous()
        torch.cuda.synchronize()
        g.track_frame_device(one.data_ptr(), w, w * h)
        g.synchronize()
        o.track_frame(frames[t])
        if t == 0:
            assert o.state().kf_added
            assert_tracker_exact(o, g, 0, "frame 0")
            assert_map_close(o, g, 0, "frame 0", 1e-7)
        else:
            assert_tracker_close(o, g, 0, "frame %d" % t)
        st = g.states()
        for s in streams[1:]:
            assert bytes(st[s]) == bytes(st[0]), (s, t)
    kf_new = len(m["keyframes"])
    assert g.state(0).n_keyframes == kf_new + 1 and g.state(0).n_points > len(m["points"])
    rows = [g.keyframe_meas(0, k) for k in range(kf_new + 1)]
    mo = o.keyframe_meas(kf_new)
    assert len(rows[kf_new]["pt"]) > 50 and np.array_equal(mo["pt"], rows[kf_new]["pt"]) and np.array_equal(mo["root"], rows[kf_new]["root"])
    for s in streams[1:]:
        for k, want in enumerate(rows):
            got = g.keyframe_meas(s, k)
            assert all(np.array_equal(got[key], want[key]) for key in ("pt", "level", "root", "source")), (s, k)
    byte0 = [s * mc.measurement_table_stride(KF, P) + kf_new * P * mc.MEAS_BYTES for s in streams]
    print("kf_meas byte offsets of the new keyframe's row:", dict(zip(streams, byte0)))
    assert byte0[2] > (1 << 31) and byte0[-2] > (1 << 32) and byte0[-1] > (1 << 32)
    snap = g.snapshot(0).tobytes()
    for s in streams[1:]:
        assert g.snapshot(s).tobytes() == snap, s
    g.close()


# ---- the map bootstrap at S = 130: workgroups of 64, 64 and 2 lanes -----------------------------------------------------------------
def _mat(p):
    p = np.array(p[:])
    m = np.eye(4)
    m[:3, :3] = p[:9].reshape(3, 3); m[:3, 3] = p[9:]
    return m


def test_bootstrap_past_the_first_workgroup():
    """bootstrap = 1, S = 130, every stream pressed at frames 0 and 14 (k_boot_press and the boot_frame launches of one lane per stream):
    trails, InitFromStereo and the first tracked frames.  The K-stream control against the oracle at the bars of
    test_gpu_bootstrap.test_trails_and_init_from_stereo_match_the_oracle (integer results exactly, what follows the homography to its
    tolerances); every replica == the control: states, initialisation info and trails in every frame, the snapshot at the end."""
    import torch
    w, h, S, n, press = 640, 480, 130, 18, (0, 14)
    idx = replica_index(S)
    fr = [feeder.Feeder(w, h, seed=sd, noise=2).render(0, n) for sd in (1234, 77, 4321)]
    kw = dict(grow_map=3, bootstrap=1, max_keyframes=4)
    g, c = capi.System(capi.default_params(w, h, S, **kw)), capi.System(capi.default_params(w, h, K, **kw))
    os_ = [orc.OracleSystem(orc.params_from_vslam(capi.default_params(w, h, 1, grow_map=3))) for _ in range(K)]
    base = torch.from_numpy(np.stack(fr)).cuda()                                  # [K, n, h, w]
    big = base[torch.tensor(idx, device="cuda")].transpose(0, 1).contiguous()
    ctl = base.transpose(0, 1).contiguous()
    torch.cuda.synchronize()
    rel = {}
    for t in range(n):
        if t in press:
            g.press_spacebar(-1); c.press_spacebar(-1)
            for o in os_:
                o.press_spacebar()
        g.track_frame_device(big[t].data_ptr(), w, w * h)
        c.track_frame_device(ctl[t].data_ptr(), w, w * h)
        g.synchronize(); c.synchronize()
        assert_replicas_equal_control(g, c, idx, ("bootstrap", t))
        info_c = [c.init_info(k) for k in range(K)]
        trails_c = [c.trails(k) for k in range(K)] if t in (1, 7, 13) else None
        for s in range(S):
            assert g.init_info(s) == info_c[idx[s]], (s, t)
            if trails_c is not None:
                assert np.array_equal(g.trails(s), trails_c[idx[s]]), (s, t)
        for k, o in enumerate(os_):                                               # the control against the oracle
            o.track_frame(fr[k][t])
            io, ig, tag = o.init_info(), info_c[k], "stream %d frame %d" % (k, t)
            assert (io["stage"], io["trails"], io["init_ok"], io["map_good"]) == (ig["stage"], ig["trails"], ig["init_ok"], ig["map_good"]), (tag, io, ig)
            if io["stage"] == 1:
                assert np.array_equal(o.trails(), c.trails(k)), tag
            so, sg = o.state(), c.state(k)
            if t == press[1]:
                assert io["hom_inliers"] == ig["hom_inliers"] and io["stereo_points"] == ig["stereo_points"] > 100, (tag, io, ig)
                assert so.n_keyframes == sg.n_keyframes == 2
                mo, mg = o.keyframe_meas(1), c.keyframe_meas(k, 1)
                trail_o, trail_g = mo["source"] == 3, mg["source"] == 3
                assert np.array_equal(mo["pt"][trail_o], mg["pt"][trail_g]) and np.array_equal(mo["root"][trail_o], mg["root"][trail_g]), tag
                assert abs(so.n_points - sg.n_points) <= max(3, so.n_points // 50), (tag, so.n_points, sg.n_points)
                same_path = so.n_ba_trials == sg.n_ba_trials
                rel_o = _mat(o.keyframe_pose(1)) @ np.linalg.inv(_mat(o.keyframe_pose(0)))
                rel_g = _mat(c.keyframe_pose(k, 1)) @ np.linalg.inv(_mat(c.keyframe_pose(k, 0)))
                assert np.abs(rel_o - rel_g).max() < (1e-5 if same_path else 5e-3), (tag, np.abs(rel_o - rel_g).max())
                n0 = io["stereo_points"]
                bo, bg = (1.0, 1.0) if same_path else (np.linalg.norm(rel_o[:3, 3]), np.linalg.norm(rel_g[:3, 3]))
                po, pg = o.points(), c.points(k)
                assert np.array_equal(po["bad"][:n0], pg["bad"][:n0]) or not same_path, tag
                co = (_mat(o.keyframe_pose(0)) @ np.c_[po["pos"][:n0], np.ones(n0)].T).T
                cg = (_mat(c.keyframe_pose(k, 0)) @ np.c_[pg["pos"][:n0], np.ones(n0)].T).T
                assert np.abs(co[:, :3] / bo - cg[:, :3] / bg).max() < (1e-4 if same_path else 1.5), (tag, np.abs(co[:, :3] / bo - cg[:, :3] / bg).max())
                for side_pts, side_k0 in ((po, o.keyframe_pose(0)), (pg, c.keyframe_pose(k, 0))):   # the dominant plane is z = 0, the cameras above it
                    z = side_pts["pos"][side_pts["bad"] == 0][:, 2]
                    c0 = -np.array(side_k0[:9]).reshape(3, 3).T @ np.array(side_k0[9:])
                    assert abs(np.median(z)) < 0.01 and c0[2] > 1.0, tag
                rel[k] = (_mat(o.keyframe_pose(1)), _mat(c.keyframe_pose(k, 1)), np.linalg.norm(rel_o[:3, 3]), np.linalg.norm(rel_g[:3, 3]))
            if t > press[1]:
                assert so.quality == sg.quality == 2 and sum(sg.found) > 100, (tag, list(so.found), list(sg.found))
                assert abs(sum(so.found) - sum(sg.found)) <= max(5, sum(so.found) // 20), (tag, list(so.found), list(sg.found))
                ro, rg = _mat(so.pose) @ np.linalg.inv(rel[k][0]), _mat(sg.pose) @ np.linalg.inv(rel[k][1])
                assert np.abs(ro[:3, :3] - rg[:3, :3]).max() < 1e-3, tag
                assert np.abs(ro[:3, 3] / rel[k][2] - rg[:3, 3] / rel[k][3]).max() < 2e-2, tag
    assert all(c.state(k).n_keyframes >= 2 and os_[k].state().n_keyframes == c.state(k).n_keyframes for k in range(K))
    assert_snapshots_equal_control(g, c, idx)
    g.close(); c.close()
