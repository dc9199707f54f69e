"""GPU: MapMaker::InitFromStereo (jni/MapMaker.cc:204-376) past the homography, bit for bit.

tests/test_gpu_bootstrap.py sets the device against the oracle's OWN HomographyInit / CalcPlaneAligner mathematics, so everything behind the
homography is held to a tolerance there.  Here the oracle runs in shared-stage mode (oracle/binding.py set_shared_stages): it takes the
results of those two stages from the host build of csrc/bootstrap_math.h, which the device equals bit for bit stage by stage
(tests/test_gpu_bootstrap_stages.py).  Both sides then enter everything else from the same bits -- the point loop of k_boot_points, the five
BootAll adjustments, the scene depths, AddSomeMapPoints in level order 0, 3, 1, 2, the adjustments until convergence, k_boot_plane's
ApplyGlobalTransformationToMap, the boot_run gating -- and every comparison is ==, on the cases of tests/stereo_cases.py (the exits of the
point loop, both `return false` exits, fewer than ten points, a mixed batch; tests/test_stereo_cases.py asserts on the CPU that the oracle
reaches each).  vslam_params.ba_sum_order = 1, bootstrap = 1, grow_map = 3 throughout; floating-point values are compared as bit patterns.

same_boot() compares in pipeline order, so the first failing assertion names the stage."""
import numpy as np
import pytest

import retire_ref as rr
import stereo_cases as sc
from helpers import assert_map_exact, assert_tracker_exact
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    """== on bit patterns: no tolerance, a NaN equals the same NaN, -0.0 is not 0.0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def device_map(g, s):
    """the stream's map and tracker state as the snapshot holds them (csrc/snapshot_format.h, parsed by tests/retire_ref.py)"""
    h, sec = rr.sections(g.snapshot(s))
    n, nk = h.n_points, h.n_kf
    rest = sec[rr.POINT_REST].reshape(n, rr.REST_BYTES)
    vec = np.ascontiguousarray(rest[:, :48]).view(np.float64).reshape(n, 6)
    ints = np.ascontiguousarray(rest[:, 48:80]).view(np.int32).reshape(n, 8)
    meas = sec[rr.KF_MEAS].reshape(nk, n, rr.MEAS_BYTES)
    tables = []
    for k in range(nk):
        flags = np.ascontiguousarray(meas[k][:, 16:20]).view(np.int8).reshape(n, 4)      # valid, level, subpix, source
        v = np.flatnonzero(flags[:, 0])
        tables.append({"pt": v.astype(np.int32), "level": flags[v, 1].astype(np.int32), "subpix": flags[v, 2].astype(np.int32), "source": flags[v, 3].astype(np.int32),
                       "root": np.ascontiguousarray(meas[k][v, :16]).view(np.float64).reshape(len(v), 2)})
    return {"state": rr.TrackerState.from_buffer_copy(sec[rr.STATE].tobytes()), "n_points": n, "n_kf": nk,
            "pos": np.ascontiguousarray(sec[rr.POINT_POS]).view(np.float64).reshape(n, 3), "right": vec[:, :3], "down": vec[:, 3:],
            "src_kf": ints[:, 0], "src_level": ints[:, 1], "irx": ints[:, 2], "iry": ints[:, 3], "bad": ints[:, 4], "n_in": ints[:, 5], "n_out": ints[:, 6],
            "kf_pose": np.ascontiguousarray(sec[rr.KF_POSE]).view(np.float64).reshape(nk, 12), "kf_depth": np.ascontiguousarray(sec[rr.KF_DEPTH]).view(np.float64).reshape(nk, 2),
            "tables": tables}


def same_info(o, g, s, tag):
    io, ig = o.init_info(), g.init_info(s)
    assert io == ig, (tag, "init_info", io, ig)                       # all six: stage, trails, init_ok, hom_inliers, stereo_points, map_good
    return io


def same_boot(o, g, s, tag):
    """the state InitFromStereo left, device == oracle, in pipeline order (1-7 of the issue's list; 8, the frames that follow, is the caller's)"""
    io = same_info(o, g, s, tag)                                                                                                   # 1
    so, sg = o.state(), g.state(s)
    if not io["map_good"]:
        assert (so.n_points, so.quality, so.lost_frames, so.frame) == (sg.n_points, sg.quality, sg.lost_frames, sg.frame), (tag, "state of a failed call")
        return
    d = device_map(g, s)
    log = o.boot_log()
    made = log["code"] == sc.CODE_POINT
    t1 = d["tables"][1]
    trail = t1["source"] == 3
    # 2: the k-th match that made a point made point k; the adjustments have since erased the outlier measurements among them
    assert d["state"].n_init_points == int(made.sum()), (tag, "how many matches became points", d["state"].n_init_points, int(made.sum()))
    mo1 = o.keyframe_meas(1)
    assert np.array_equal(t1["pt"][trail], mo1["pt"][mo1["source"] == 3]), (tag, "which matches became points")
    assert same(t1["root"][trail], log["sub"][made][t1["pt"][trail]]), (tag, "sub-pixel positions of the stereo points")
    assert d["n_kf"] == so.n_keyframes == sg.n_keyframes == 2 and d["n_points"] == so.n_points == sg.n_points, (tag, "counts", d["n_kf"], so.n_keyframes, d["n_points"], so.n_points)
    for k in range(2):                                                                                                              # 3
        mo, sp = o.keyframe_meas(k), o.keyframe_meas_subpix(k)
        td = d["tables"][k]
        assert np.array_equal(mo["pt"], td["pt"]), (tag, "measured points of keyframe %d" % k)
        for f, want in (("level", mo["level"]), ("source", mo["source"]), ("subpix", sp)):
            assert np.array_equal(want, td[f]), (tag, "keyframe %d %s" % (k, f))
        assert same(mo["root"], td["root"]), (tag, "keyframe %d root positions" % k)
    st = d["state"]
    assert so.n_ba_trials == sg.n_ba_trials == st.n_ba_trials, (tag, "LM trials", so.n_ba_trials, sg.n_ba_trials)                  # 4
    assert o.converged() == (st.ba_converged_recent, st.ba_converged_full), (tag, "converged flags", o.converged(), (st.ba_converged_recent, st.ba_converged_full))
    for k in range(2):
        assert same(o.keyframe_depth(k), d["kf_depth"][k]), (tag, "scene depth of keyframe %d" % k, o.keyframe_depth(k), d["kf_depth"][k])
    for k in range(2):                                                                                                              # 5
        assert same(o.keyframe_pose(k), d["kf_pose"][k]), (tag, "pose of keyframe %d" % k, np.abs(o.keyframe_pose(k) - d["kf_pose"][k]).max())
        assert same(d["kf_pose"][k], g.keyframe_pose(s, k))
    po, ps = o.points(), o.point_sources()                                                                                          # 6
    assert same(po["pos"], d["pos"]), (tag, "point positions", np.abs(po["pos"] - d["pos"]).max())
    assert same(d["pos"], g.points(s)["pos"])
    for f in ("right", "down"):
        assert same(ps[f], d[f]), (tag, "pixel vector %s" % f, np.flatnonzero((bits(ps[f]) != bits(d[f])).any(axis=1))[:8], np.abs(ps[f] - d[f]).max())
    for f, want in (("bad", po["bad"]), ("src_kf", ps["src_kf"]), ("src_level", ps["src_level"]), ("irx", ps["irx"]), ("iry", ps["iry"]), ("n_in", po["n_in"]), ("n_out", po["n_out"])):
        assert np.array_equal(want, d[f]), (tag, f)
    assert same(so.pose[:], sg.pose[:]) and same(so.pose[:], st.pose_final[:]) and same(so.pose[:], st.start_pose[:]), (tag, "tracker pose")   # 7
    assert same(so.velocity[:], sg.velocity[:]) and (so.quality, so.lost_frames, so.frame) == (sg.quality, sg.lost_frames, sg.frame), (tag, "tracker state")
    assert same([o.boot_diag()["wiggle_depth_norm"]], [st.wiggle_depth_norm]), (tag, "wiggle_depth_norm", o.boot_diag()["wiggle_depth_norm"], st.wiggle_depth_norm)


def same_tables(o, g, s, tag):
    for k in range(o.state().n_keyframes):
        mo, mg = o.keyframe_meas(k), g.keyframe_meas(s, k)
        assert np.array_equal(mo["pt"], mg["pt"]) and np.array_equal(mo["source"], mg["source"]) and np.array_equal(mo["level"], mg["level"]), (tag, k)
        assert same(mo["root"], mg["root"]), (tag, k)


def follow(o, g, s, frame, tag, batch=None):
    """one further tracked frame on both sides (the caller has tracked the device's when it passes batch = True)"""
    if batch is None:
        g.track_frame(frame[None])
    o.track_frame(frame)
    same_info(o, g, s, tag)
    assert_tracker_exact(o, g, s, tag)                                 # its template comparison is the second witness of the pixel vectors
    if o.state().kf_added:
        assert_map_exact(o, g, s, tag)
        same_tables(o, g, s, tag)


CASE_NAMES = {p: [c.name for c in sc.one_stream_cases(p)] for p in sc.PATCHES}


@pytest.mark.parametrize("patch,name", [(p, n) for p in sc.PATCHES for n in CASE_NAMES[p]])
def test_init_from_stereo_bit_for_bit(patch, name):
    """cases A-F through vslam_init_from_stereo on a one-stream system: the return value, then same_boot, then three tracked frames"""
    c = {q.name: q for q in sc.one_stream_cases(patch)}[name]
    tag = "patch %d, %s" % (patch, name)
    g = capi.System(c.params(**sc.DEVICE_KW))
    g.set_boot_seed(0, c.seed)
    o = c.oracle(shared=True)
    ok_g, pose_g = g.init_from_stereo(c.first, c.second, c.matches)
    ok_o, pose_o = o.init_from_stereo(c.first, c.second, c.matches)
    assert ok_g == ok_o, (tag, "return value", ok_g, ok_o)
    same_boot(o, g, 0, tag)
    if ok_o:
        assert same(pose_g, pose_o), (tag, "the pose handed back")
    for t, f in enumerate(c.follow):
        follow(o, g, 0, f, "%s, frame %d after" % (tag, t + 1))
    g.close(); o.close()


@pytest.mark.parametrize("patch", sc.PATCHES)
def test_mixed_batch_through_the_spacebar_path(patch):
    """case G: five streams of one system -- one tracks a loaded map, two consume their second press in the same frame (one succeeds, one
    fails on a zero baseline), one consumes its first press in that frame, one is never pressed -- every stream == its own oracle after
    every frame; the oracles of the first and the last run no bootstrap at all."""
    streams = sc.mixed_batch(patch)
    S = len(streams)
    g = capi.System(sc.params(sc.SIZE[0], sc.SIZE[1], patch, n_streams=S, **sc.DEVICE_KW))
    os_ = []
    for s, st in enumerate(streams):
        role, frames, presses, scene, seed = st
        g.set_boot_seed(s, seed)
        if scene is not None:
            g.load_map(s, scene[1]); g.set_pose(s, scene[0].pose(-1))
        os_.append(sc.mixed_oracle(patch, st))
    t2 = sc.N_TRAIL_FRAMES - 1
    for t in range(sc.G_FRAMES):
        for s, st in enumerate(streams):
            if t in st[2]:
                g.press_spacebar(s); os_[s].press_spacebar()
        g.track_frame(np.stack([st[1][t] for st in streams]))
        for s, st in enumerate(streams):
            o, tag = os_[s], "patch %d, stream %d (%s), frame %d" % (patch, s, st[0], t)
            o.track_frame(st[1][t])
            io = same_info(o, g, s, tag)
            if io["stage"] == 1:
                assert np.array_equal(o.trails(), g.trails(s)), (tag, "trails")
            if t == t2 and t in st[2] and io["stage"] == 2:
                same_boot(o, g, s, tag)
            if io["map_good"]:
                assert_tracker_exact(o, g, s, tag)
                if o.state().kf_added:
                    assert_map_exact(o, g, s, tag)
                    same_tables(o, g, s, tag)
            else:                                                      # no map: everything but n_keyframes, which counts the first keyframe the
                so, sg = o.state(), g.state(s)                         # device keeps in slot 0 while the trails run (the oracle's map is empty)
                assert (so.frame, so.quality, so.lost_frames, so.n_points, so.kf_added) == (sg.frame, sg.quality, sg.lost_frames, sg.n_points, sg.kf_added), tag
                assert list(so.attempted) == list(sg.attempted) == [0] * 4 and list(so.found) == list(sg.found) == [0] * 4, tag
                if io["stage"] != 1:
                    assert so.n_keyframes == sg.n_keyframes == 0, (tag, so.n_keyframes, sg.n_keyframes)
    assert g.init_info(1)["map_good"] == 1 and g.init_info(2)["map_good"] == 0 and g.init_info(3)["stage"] == 1 and g.init_info(4)["stage"] == 0
    g.close()
    for o in os_:
        o.close()
