"""GPU: similarity transform of a live stream's map -- vslam_transform_maps, vslam_get_transform_info, vslam_get_transform_timing
(csrc/transform.hip, the rule in csrc/similarity_dev.h) and vslam_fit_similarity beside it.

The yardstick is the independent numpy model of tests/transform_ref.py, by the method of tests/test_gpu_retire.py: a stream's snapshot
inventories its whole state, so snapshot(after) == transform_blob(snapshot(before), T, s), byte for byte, says the device did what the
rule states and nothing else.  What a snapshot does not carry (keyframe corner lists, keyframe SmallBlurryImages) is compared with a
second system that restored the model's blob and remade them, and the continuation is compared with that system frame by frame.  Two
further tests do not go through the model: the direct meaning of each row in plain matrix arithmetic, and gauge invariance -- a run
transformed half way, mapped back, is the plain run."""
import ctypes as C

import numpy as np
import pytest

import retire_ref as rr
import transform_ref as tr
from helpers import POSE_TOL, pose_err
from test_gpu_reset import dump
from test_gpu_retire import scene, start
from test_gpu_snapshot import derived, random_map, readbacks
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

W, H = 640, 480
E_INVALID, E_STATE = -1, -4
KW = dict(grow_map=3, idle_iterations=1, relocalise=1, ba_sum_order=1)
BOUND = 1e-12                    # x (1 + extent): about 30 roundings of 1.1e-16 with a wide margin
IDENT = tr.pose12(np.eye(3), np.zeros(3))
T_GEN, S_GEN = tr.pose12(tr.rotation([1.0, 2.0, -0.5], 0.9), [0.3, -1.2, 2.0]), 1.7      # a rotation about an oblique axis


def transform_rc(g, streams, poses, scales=None, n=None):
    a = None if streams is None else np.array(streams, np.int32)
    q = None if poses is None else np.ascontiguousarray(poses, np.float64)
    sc = None if scales is None else np.ascontiguousarray(scales, np.float64)
    return g.lib.vslam_transform_maps(g.h, None if a is None else a.ctypes.data, (len(a) if a is not None else g.S) if n is None else n,
                                      None if q is None else q.ctypes.data, None if sc is None else sc.ctypes.data)


def mapped_back(pose, T, s):
    """a pose of the transformed run in the original gauge: C' T, then t /= s"""
    c = tr.mul(np.asarray(pose[:], np.float64), np.asarray(T, np.float64))
    c[9:] = c[9:] / s
    return c


def mapped_pose(pose, T, s):
    """plain matrix arithmetic, independent of the model: R' = R_c R^T, t' = s t_c - R' t"""
    c, T = np.asarray(pose[:], np.float64), np.asarray(T, np.float64)
    R = c[:9].reshape(3, 3) @ T[:9].reshape(3, 3).T
    return np.concatenate([R.reshape(-1), s * c[9:] - R @ T[9:]])


def extent(a):
    return float(np.abs(a).max()) if np.size(a) else 0.0


# ---- 1, 2, 3: the whole state against the model; the direct meaning; derived data and the continuation -------------------------------
N_MAX, N_MORE, N_BLANK = 40, 25, 6
_live = {}


def live():
    """System A, 3 streams (scenes 1234, 77, 4321).  Stream 1 is tracked until it has added a keyframe, then sees blank frames until it is
    lost and its relocaliser has made an attempt, then its own next frames again until it tracks GOOD with a velocity; then its map gets
    (T_GEN, S_GEN).
    Everything the three tests below compare is gathered here, once."""
    if _live:
        return _live
    scs = [scene(1234, N_MAX + N_MORE), scene(77, N_MAX + N_MORE), scene(4321, N_MAX + N_MORE)]
    A = capi.System(capi.default_params(W, H, 3, **KW))
    for s, sc in enumerate(scs):
        start(A, s, sc)
    blank = np.zeros((H, W), np.uint8)
    t = j = added = 0
    blanks = -1                                                      # -1: not yet; > 0: that many blank frames to go; 0: done
    while t < N_MAX:
        real = blanks <= 0
        A.track_frame(np.stack([scs[0][2][t], scs[1][2][j] if real else blank, scs[2][2][t]]))
        t += 1
        j += real
        st = A.state(1)
        added += st.kf_added
        if blanks < 0 and added >= 1 and t >= 2:
            blanks = N_BLANK
        elif blanks > 0:
            blanks -= 1
        elif blanks == 0 and A.reloc_info(1)["attempts"] >= 1 and st.quality == 2 and st.lost_frames == 0 and np.any(np.array(st.velocity[:])):
            break                                                    # (the frame that recovers has no motion model yet: one more)
    blob0 = A.snapshot(1).copy()
    others = [dump(A, 0), dump(A, 2), readbacks(A, 0), readbacks(A, 2)]
    _live.update(A=A, scs=scs, t=t, j=j, added=added, blob0=blob0, reloc=A.reloc_info(1), state=A.state(1), others=others)
    A.transform_maps([1], [T_GEN], [S_GEN])
    _live.update(blob1=A.snapshot(1).copy(), info=[A.transform_info(s) for s in range(3)], ms=A.transform_timing(),
                 others_after=[dump(A, 0), dump(A, 2), readbacks(A, 0), readbacks(A, 2)])
    return _live


def test_whole_state_against_the_model():
    """snapshot(1) after the transform == transform_blob(snapshot(1) before, T, s) byte for byte; streams 0 and 2 keep every bit of
    their dumps and read-backs; transform_info holds the one transform; the timing is positive."""
    L = live()
    assert L["added"] >= 1 and L["reloc"]["attempts"] >= 1 and np.any(L["reloc"]["best_pose"]), (L["t"], L["added"], L["reloc"])
    assert L["state"].quality == 2 and np.any(np.array(L["state"].velocity[:])), (L["t"], L["state"].quality)
    want, got = tr.transform_blob(L["blob0"], T_GEN, S_GEN), L["blob1"]
    assert len(got) == len(want) and np.array_equal(got, want), (len(got), len(want), int((got[:min(len(got), len(want))] != want[:min(len(got), len(want))]).sum()))
    assert not np.array_equal(L["blob0"], L["blob1"])
    assert L["others_after"] == L["others"]
    i0, i1, i2 = L["info"]
    assert (i1["transforms"], i1["frame"], i1["scale"]) == (1, L["state"].frame, S_GEN) and np.array_equal(i1["pose"], T_GEN), i1
    for i in (i0, i2):
        assert (i["transforms"], i["frame"], i["scale"]) == (0, 0, 1.0) and np.array_equal(i["pose"], IDENT), i
    assert L["ms"] > 0
    n = capi.snapshot_info(L["blob0"])
    print("transformed %d points, %d keyframes of one stream: %.3f ms" % (n.n_points, n.n_keyframes, L["ms"]))


def test_direct_meaning_of_each_row():
    """Independent of the model.  The stream of live() restored into a system of its own and tracked one frame; then s = 2 with a pure
    translation: the translational velocity and the depths are exactly twice what they were, the rotational velocity and msd_velocity are
    unchanged, vslam_need_new_keyframe answers the same, every point is R (2 x) + t, every keyframe pose, the tracker's pose and the
    relocaliser's mse3Best are mapped as a camera pose is, and the keyframe corner lists and SmallBlurryImages keep every bit."""
    L = live()
    D = capi.System(capi.default_params(W, H, 1, **KW))
    D.restore(0, L["blob0"])
    D.track_frame(L["scs"][1][2][L["j"]][None])
    T, s = tr.pose12(np.eye(3), [0.5, -2.0, 1.25]), 2.0
    st0, p0, r0, d0, need0 = D.state(0), D.points(0), D.reloc_info(0), derived(D, 0), D.need_new_keyframe(0)
    kf0 = [D.keyframe_pose(0, k) for k in range(st0.n_keyframes)]
    D.transform_maps([0], [T], [s])
    st1, p1, r1 = D.state(0), D.points(0), D.reloc_info(0)
    v0, v1 = np.array(st0.velocity[:]), np.array(st1.velocity[:])
    assert np.any(v0[:3]) and np.array_equal(v1[:3], 2.0 * v0[:3]) and np.array_equal(v1[3:], v0[3:])
    assert (st1.depth_mean, st1.depth_sigma, st1.msd_velocity) == (2.0 * st0.depth_mean, 2.0 * st0.depth_sigma, st0.msd_velocity)
    assert D.need_new_keyframe(0) == need0
    want = 2.0 * p0["pos"] + T[9:]
    worst = extent(p1["pos"] - want) / (1.0 + extent(want))
    assert len(want) > 100 and worst <= BOUND, worst
    for k in ("bad", "n_in", "n_out"):
        assert np.array_equal(p0[k], p1[k])
    worst_pose = 0.0
    for a, b in zip(kf0 + [st0.pose, r0["best_pose"]], [D.keyframe_pose(0, k) for k in range(st1.n_keyframes)] + [st1.pose, r1["best_pose"]]):
        m = mapped_pose(a, T, s)
        worst_pose = max(worst_pose, extent(np.asarray(b[:]) - m) / (1.0 + extent(m)))
    assert r0["attempts"] >= 1 and np.any(r0["best_pose"]) and worst_pose <= BOUND, worst_pose
    assert all(np.array_equal(r0[k], r1[k]) for k in r0 if k != "best_pose")
    assert derived(D, 0) == d0
    assert st1.n_keyframes == st0.n_keyframes and st1.n_points == st0.n_points and st1.frame == st0.frame and st1.quality == st0.quality
    print("direct meaning: points %.3e, poses %.3e of the bound %.0e" % (worst, worst_pose, BOUND))
    D.close()


def test_derived_data_and_the_continuation():
    """The model's blob restored into slot 0 of a system B with other capacities: right after, every read-back of A's stream 1 == B's
    slot 0, the keyframe corner lists, every keyframe's SmallBlurryImage and reloc_info among them; then 25 more frames on both with
    equal dumps after every frame, a keyframe and its bundle adjustment among them."""
    L = live()
    A, scs, t0, j0 = L["A"], L["scs"], L["t"], L["j"]
    B = capi.System(capi.default_params(W, H, 2, **KW, max_points=4000, max_keyframes=24))
    B.restore(0, tr.transform_blob(L["blob0"], T_GEN, S_GEN))
    assert readbacks(A, 1) == readbacks(B, 0)
    assert derived(A, 1) == derived(B, 0)
    ra, rb = A.reloc_info(1), B.reloc_info(0)
    assert all(np.array_equal(ra[k], rb[k]) for k in ra)
    added = trials = 0
    for d in range(N_MORE):
        A.track_frame(np.stack([scs[0][2][t0 + d], scs[1][2][j0 + d], scs[2][2][t0 + d]]))
        B.track_frame(np.stack([scs[1][2][j0 + d]] * 2))
        assert dump(A, 1) == dump(B, 0), d
        added += A.state(1).kf_added
    trials = A.state(1).n_ba_trials
    assert added >= 1 and trials > 0, (added, trials)
    assert readbacks(A, 1) == readbacks(B, 0) and derived(A, 1) == derived(B, 0)
    assert A.state(1).quality == 2
    assert A.transform_info(1)["transforms"] == 1 and B.transform_info(0)["transforms"] == 0       # a restore starts the record anew
    A.close(); B.close()
    _live.clear()


# ---- 4: gauge invariance ------------------------------------------------------------------------------------------------------------------
N_BEFORE, N_AFTER = 10, 25


@pytest.mark.parametrize("case", ["rigid", "rescaled"])
def test_gauge_invariance(case):
    """Scenes 1234 and 23 as two streams, run A plain and run A' transformed after frame 10, each stream by its own rotation and shift.
    "rigid": s = 1 with the map growing (grow_map = 3, idle jobs).  "rescaled": s = 2.5 with grow_map = 0 and no idle jobs, because the
    reference reads wiggle_scale as an absolute length where it grows the map -- and with ba_convergence_limit = 0 in BOTH runs, because
    Bundle::Compute ends on the squared length of its update (mdUpdateConvergenceLimit, an absolute length too): with the default 1e-6 the
    keyframe of frame 21 is adjusted in 20 trials in A and 24 in A', and the poses then differ by up to 1.03e-4 (scene 1234) and 4.6e-6
    (scene 23) where they differed by 2e-10 before; with the limit out of the way every adjustment runs its ba_max_iterations in both.
    For each of the next 25 frames A''s pose mapped back (C' T, then t /= s) is A's pose within POSE_TOL, and both track GOOD.  The
    largest pose difference and the largest difference of a map point are printed (DESIGN.md records them); the points have no bar."""
    kw = dict(KW) if case == "rigid" else dict(relocalise=1, ba_sum_order=1, ba_convergence_limit=0.0)
    scs = [scene(1234, N_MAX + N_MORE), scene(23, N_BEFORE + N_AFTER)]
    Ts = [T_GEN, tr.pose12(tr.rotation([-0.3, 0.2, 1.0], 2.2), [-1.5, 0.4, 0.7])]
    ss = [1.0, 1.0] if case == "rigid" else [2.5, 2.5]
    A, A2 = (capi.System(capi.default_params(W, H, 2, **kw)) for _ in range(2))
    for g in (A, A2):
        for s, sc in enumerate(scs):
            start(g, s, sc)
    worst = worst_pt = 0.0
    for t in range(N_BEFORE + N_AFTER):
        fr = np.stack([sc[2][t] for sc in scs])
        A.track_frame(fr); A2.track_frame(fr)
        if t == N_BEFORE - 1:
            assert [dump(A, s) for s in range(2)] == [dump(A2, s) for s in range(2)]
            A2.transform_maps([0, 1], Ts, ss)
        if t >= N_BEFORE:
            for s in range(2):
                a, b = A.state(s), A2.state(s)
                assert a.quality == 2 and b.quality == 2, (t, s, a.quality, b.quality)
                e = pose_err(mapped_back(b.pose, Ts[s], ss[s]), a.pose)
                worst = max(worst, e)
                assert e < POSE_TOL, (t, s, e)
    for s in range(2):
        Ti, si = tr.invert(Ts[s], ss[s])
        pa, pb = A.points(s)["pos"], A2.points(s)["pos"]
        if len(pa) == len(pb):
            worst_pt = max(worst_pt, extent(tr.sim_point(Ti, si, pb) - pa))
        else:
            print("stream %d: %d points plain, %d transformed" % (s, len(pa), len(pb)))
    print("gauge invariance, %s: largest pose difference %.3e (bar %.0e), largest point difference %.3e" % (case, worst, POSE_TOL, worst_pt))
    A.close(); A2.close()


# ---- 5: where the loops split ---------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
CAP = dict(max_points=513, max_keyframes=5)          # the largest counts fill the system
OPT = dict(grow_map=3, relocalise=1, idle_iterations=1)


def randomised(blob, rng):
    """The uploaded map's blob with every field the transform reads filled with random finite doubles, and the per-point tracker data
    around TrackData::cam with random bytes -> blob"""
    h, s = rr.sections(blob)
    n, nk = h.n_points, h.n_kf
    td = rng.integers(0, 256, (n, rr.TRACKDATA_BYTES), dtype=np.uint8)
    td[:, :24] = rng.normal(size=(n, 3)).view(np.uint8).reshape(n, 24)
    s[rr.TRACKDATA] = td.reshape(-1)
    s[rr.KF_DEPTH] = rng.uniform(0.5, 5, size=nk * 2).view(np.uint8)
    poses = np.stack([tr.pose12(tr.rotation(rng.normal(size=3), rng.uniform(0, 3)), rng.normal(size=3)) for _ in range(nk + 4)])
    s[rr.KF_POSE] = poses[:nk].reshape(-1).view(np.uint8)
    st = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes())
    st.pose_final[:], st.start_pose[:], st.pose_cur[:] = poses[nk].tolist(), poses[nk + 1].tolist(), poses[nk + 2].tolist()
    st.velocity[:] = rng.normal(size=6).tolist()
    st.msd_vel, st.depth_mean, st.depth_sigma, st.wiggle_depth_norm = rng.uniform(0.1, 2, size=4).tolist()
    s[rr.STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    ri = rr.RelocInfo.from_buffer_copy(s[rr.RELOC_INFO].tobytes())
    ri.attempts, ri.best = 2, int(rng.integers(nk))
    ri.best_pose[:], ri.ln_adj[:] = poses[nk + 3].tolist(), rng.normal(size=6).tolist()
    s[rr.RELOC_INFO] = np.frombuffer(bytes(ri), np.uint8).copy()
    return rr.assemble(h, s)


def test_where_the_loops_split():
    """No tracking.  96 x 64, max_points = 513, max_keyframes = 5.  Random maps of 1, 63, 64, 65, 255, 256, 257 and 513 points (the
    kernel's blocks are 256 points) with 2 and 5 keyframes are uploaded into streams 0 and 1, their snapshots filled with random values
    in every field the transform reads and restored; one call then moves both, each by its own transform, and each snapshot == the
    model's blob, while stream 2, a full map that is not listed, keeps every byte.  A stream of 1 point beside one of 513 is among the
    pairs.  A second system that restored the model's blob reads back the same, derived keyframe data included.  Last, a call with
    streams == NULL and scale == NULL moves all three."""
    w, h = 96, 64
    rng = np.random.default_rng(96064)
    g = capi.System(capi.default_params(w, h, 3, **CAP, **OPT))
    B = capi.System(capi.default_params(w, h, 1, max_points=600, max_keyframes=7, **OPT))
    g.load_map(2, random_map(rng, w, h, 5, 513))
    g.restore(2, randomised(g.snapshot(2), rng))
    other = g.snapshot(2).copy()
    for ci, n0 in enumerate(COUNTS):
        n1 = COUNTS[(ci + 7) % 8]                                    # (1, 513), (63, 1), (64, 63) ...
        nks = (2, 5) if ci % 2 == 0 else (5, 2)
        blobs = []
        g.reset([0, 1])
        for s, (n, nk) in enumerate(zip((n0, n1), nks)):
            g.load_map(s, random_map(rng, w, h, nk, n))
            blobs.append(randomised(g.snapshot(s), rng))
            g.restore(s, blobs[s])
            assert np.array_equal(g.snapshot(s), blobs[s]), (ci, s)
        Ts = [tr.pose12(tr.rotation(rng.normal(size=3), rng.uniform(-3, 3)), rng.normal(size=3) * 2) for _ in range(2)]
        ss = [float(np.exp(rng.uniform(-1, 1))), 1.0 if ci % 3 == 0 else float(np.exp(rng.uniform(-1, 1)))]
        order = [0, 1] if ci % 2 == 0 else [1, 0]                    # transform i belongs to streams[i], whatever the order
        g.transform_maps(order, [Ts[s] for s in order], [ss[s] for s in order])
        for s in range(2):
            want, got = tr.transform_blob(blobs[s], Ts[s], ss[s]), g.snapshot(s)
            assert len(got) == len(want) and np.array_equal(got, want), (ci, s, (n0, n1)[s], nks[s], int((got != want).sum()))
            assert g.transform_info(s)["transforms"] == 1
        assert np.array_equal(g.snapshot(2), other), ci
        B.restore(0, tr.transform_blob(blobs[0], Ts[0], ss[0]))
        assert readbacks(g, 0) == readbacks(B, 0) and derived(g, 0) == derived(B, 0), ci
    before = [g.snapshot(s).copy() for s in range(3)]
    Ts = [tr.pose12(tr.rotation(rng.normal(size=3), rng.uniform(-3, 3)), rng.normal(size=3)) for _ in range(3)]
    assert transform_rc(g, None, Ts, None) == 0
    for s in range(3):
        assert np.array_equal(g.snapshot(s), tr.transform_blob(before[s], Ts[s], 1.0)), s
    assert [g.transform_info(s)["transforms"] for s in range(3)] == [2, 2, 1]
    g.close(); B.close()


# ---- 6: gates ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """Three streams of a system with bootstrap = 1: stream 0 tracks an uploaded map, stream 1 has its trails running, stream 2 has no
    map.  VSLAM_E_INVALID: NULL system, n < 0, n > n_streams, an index outside the batch, a duplicate, NULL transforms, a non-finite
    entry or scale, s <= 0, a near-rotation with a 1e-6 shear, a reflection -- each also beside a valid entry.  VSLAM_E_STATE: a frame is
    open; a stream without a map beside a valid one; the trails running.  After each refusal the snapshots of streams 0 and 2 (a
    stream whose trails run cannot be snapshotted) and the dumps of all three are what they were, and no transform is on record.
    n == 0 succeeds and does nothing.  The timing is refused before the first call that transformed."""
    a = scene(1234, N_MAX + N_MORE)
    g = capi.System(capi.default_params(W, H, 3, grow_map=3, bootstrap=1, ba_sum_order=1))
    start(g, 0, a)
    g.press_spacebar(1)
    for t in range(2):
        g.track_frame(np.stack([a[2][t]] * 3))
    assert g.init_info(1)["stage"] == 1 and g.state(0).quality == 2 and g.state(2).n_keyframes == 0

    def everything():
        return [g.snapshot(0).tobytes(), g.snapshot(2).tobytes()] + [dump(g, s) for s in range(3)] + [g.transform_info(s)["transforms"] for s in range(3)]

    before = everything()
    ok = T_GEN
    shear = ok.copy(); shear[1] += 1e-6
    mirror = tr.pose12(np.diag([1.0, 1.0, -1.0]), [0, 0, 0])
    nan_t = ok.copy(); nan_t[10] = np.nan
    inf_r = ok.copy(); inf_r[4] = np.inf
    lib = g.lib
    one = np.array([0], np.int32)
    assert lib.vslam_transform_maps(None, one.ctypes.data, 1, ok.ctypes.data, None) == E_INVALID
    assert transform_rc(g, [0], [ok], n=-1) == E_INVALID and transform_rc(g, [0, 1, 2, 0], [ok] * 4, n=4) == E_INVALID
    assert transform_rc(g, [3], [ok]) == E_INVALID and transform_rc(g, [-1], [ok]) == E_INVALID and transform_rc(g, [0, 3], [ok, ok]) == E_INVALID
    assert transform_rc(g, [0, 0], [ok, ok]) == E_INVALID
    assert transform_rc(g, [0], None) == E_INVALID and transform_rc(g, None, None) == E_INVALID
    for bad in (shear, mirror, nan_t, inf_r):
        assert transform_rc(g, [0], [bad]) == E_INVALID and transform_rc(g, [2, 0], [ok, bad]) == E_INVALID
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert transform_rc(g, [0], [ok], [bad]) == E_INVALID
    assert b"transform_maps" in lib.vslam_last_error()
    assert everything() == before
    assert transform_rc(g, [2], [ok]) == E_STATE and transform_rc(g, [0, 2], [ok, ok]) == E_STATE          # no map
    assert transform_rc(g, [1], [ok]) == E_STATE and transform_rc(g, [1, 0], [ok, ok]) == E_STATE          # trails running
    assert transform_rc(g, None, [ok] * 3) == E_STATE
    assert everything() == before
    assert transform_rc(g, [0], [ok], n=0) == 0 and lib.vslam_transform_maps(g.h, None, 0, None, None) == 0
    ms = C.c_double(0.0)
    assert lib.vslam_get_transform_timing(g.h, C.byref(ms)) == E_STATE
    assert everything() == before
    g.make_keyframe_lite(np.stack([a[2][2]] * 3)); g.patch_search(0)
    assert transform_rc(g, [0], [ok]) == E_STATE                                                            # a frame is open
    g.pose_update(0); g.patch_search(1); g.pose_update(1); g.finish_frame()
    assert [g.transform_info(s)["transforms"] for s in range(3)] == [0, 0, 0]
    oi, od = np.zeros(2, np.int32), np.zeros(13)
    assert lib.vslam_get_transform_info(g.h, 3, oi.ctypes.data, od.ctypes.data) == E_INVALID and lib.vslam_get_transform_info(g.h, 0, None, od.ctypes.data) == E_INVALID
    # a rotation as a product of a few leaves far less than the limit, and the same call succeeds between frames
    prod = tr.rotation([1, 1, 0], 0.3) @ tr.rotation([0, 1, 2], 1.1) @ tr.rotation([3, -1, 0.5], 2.9) @ tr.rotation([0.1, 0.2, 0.3], 0.01)
    g.transform_maps([0], [tr.pose12(prod, [1, 2, 3])], [1.3])
    assert g.transform_info(0)["transforms"] == 1 and g.transform_timing() > 0
    g.track_frame(np.stack([a[2][3]] * 3))
    assert g.state(0).quality == 2
    g.reset([0])
    i = g.transform_info(0)
    assert (i["transforms"], i["frame"], i["scale"]) == (0, 0, 1.0) and np.array_equal(i["pose"], IDENT)
    g.close()


def test_a_pending_adjustment_is_refused_until_it_has_landed():
    """ba_delay_frames = 3: frame 0 is a keyframe frame; until its adjustment lands the call is refused with VSLAM_E_STATE and nothing
    changes (the result would land in the old gauge); the same call succeeds once it has landed, and the stream goes on GOOD."""
    D, n = 3, 6
    a = scene(1234, N_MAX + N_MORE)
    g = capi.System(capi.default_params(W, H, 2, ba_delay_frames=D, ba_sum_order=1))
    start(g, 0, a)
    ok_at = None
    for t in range(n):
        g.track_frame(np.stack([a[2][t]] * 2))
        if ok_at is not None:
            continue
        before = [dump(g, s) for s in range(2)]
        rc = transform_rc(g, [0], [T_GEN], [S_GEN])
        if rc == E_STATE:
            assert t < D and [dump(g, s) for s in range(2)] == before and g.transform_info(0)["transforms"] == 0
        else:
            assert rc == 0 and t == D
            ok_at = t
            assert g.transform_info(0)["frame"] == t + 1
    assert ok_at == D and g.state(0).quality == 2
    g.close()


# ---- 7: registering to a known frame, end to end ------------------------------------------------------------------------------------------
def centres(poses):
    p = np.asarray(poses, np.float64).reshape(-1, 12)
    return np.stack([-q[:9].reshape(3, 3).T @ q[9:] for q in p])


def test_registering_to_a_known_frame():
    """An uploaded map is moved into an arbitrary gauge G and tracked for 15 frames.  Its keyframe centres, read back, are fitted to the
    feeder's true centres with vslam_fit_similarity and the fit is applied: the tracker's pose is then the pose of a plain run within
    POSE_TOL, and transform_info's accumulated similarity is the composition of the two calls.  (min_frames_between_kf is out of reach,
    so the keyframes are the uploaded ones and their true centres are known; the map does not grow, because G rescales.)"""
    n = 15
    f, m, frames = scene(1234, N_MAX + N_MORE)
    kw = dict(ba_sum_order=1, min_frames_between_kf=1000)
    P, Q = (capi.System(capi.default_params(W, H, 1, **kw)) for _ in range(2))
    start(P, 0, (f, m, frames)); start(Q, 0, (f, m, frames))
    G, sG = tr.pose12(tr.rotation([0.4, -1.0, 0.3], 2.0), [5.0, -3.0, 1.0]), 1.6
    Q.transform_maps([0], [G], [sG])
    for t in range(n):
        P.track_frame(frames[t]); Q.track_frame(frames[t])
    assert P.state(0).quality == 2 and Q.state(0).quality == 2
    nk = Q.state(0).n_keyframes
    assert nk == len(m["keyframes"])
    true = centres([k["pose"] for k in m["keyframes"]])
    got = centres([Q.keyframe_pose(0, k) for k in range(nk)])
    assert extent(got - true) > 1.0                                  # Q really lives in another gauge
    F, sF, rms = capi.fit_similarity(got, true)
    Q.transform_maps([0], [F], [sF])
    e = pose_err(Q.state(0).pose, P.state(0).pose)
    print("registered: fit rms %.3e, pose against the plain run %.3e (bar %.0e)" % (rms, e, POSE_TOL))
    assert rms < 1e-9 and e < POSE_TOL, (rms, e)
    i = Q.transform_info(0)
    accT, accs = tr.compose(F, sF, G, sG)
    assert i["transforms"] == 2 and i["frame"] == n
    assert extent(i["pose"] - accT) <= BOUND * (1 + extent(accT)) and abs(i["scale"] - accs) <= BOUND
    assert extent(i["pose"] - IDENT) < 1e-9 and abs(i["scale"] - 1.0) < 1e-9      # back where the map was made
    P.track_frame(frames[n]); Q.track_frame(frames[n])              # and the stream goes on there
    assert Q.state(0).quality == 2 and pose_err(Q.state(0).pose, P.state(0).pose) < POSE_TOL
    P.close(); Q.close()
