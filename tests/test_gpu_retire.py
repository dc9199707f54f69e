"""GPU: keyframe retirement -- vslam_retire_keyframes and vslam_params.keyframe_retire (csrc/retire.hip).

The reference cannot retire (its map only grows), so the yardstick is the independent numpy model of tests/retire_ref.py: a stream's
snapshot inventories its whole state, so snapshot(after) == retire_blob(snapshot(before), r), byte for byte, says the device did what
the model states and nothing else.  What a snapshot does not carry (keyframe corner lists, keyframe SmallBlurryImages) is compared with a
second system that restored the model's blob and remade them, and the continuation is compared with that system frame by frame."""
import ctypes as C

import numpy as np
import pytest

import retire_ref as rr
from helpers import make_oracle, make_scene, pose_err
from test_gpu_reset import dump
from test_gpu_snapshot import derived, random_map, readbacks
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

W, H = 640, 480
E_INVALID, E_STATE = -1, -4
KW = dict(grow_map=3, idle_iterations=1, relocalise=1, ba_sum_order=1)
_scenes = {}


def scene(seed, n_frames, **kw):
    key = (seed, n_frames, tuple(sorted(kw.items())))
    if key not in _scenes:
        _scenes[key] = make_scene(W, H, seed=seed, n_frames=n_frames, **kw)
    return _scenes[key]


def start(g, s, sc):
    g.load_map(s, sc[1]); g.set_pose(s, sc[0].pose(-1))


def retire_rc(g, streams, keyframes):
    a, k = np.array(streams, np.int32), np.array(keyframes, np.int32)
    return g.lib.vslam_retire_keyframes(g.h, a.ctypes.data, k.ctypes.data, len(a))


# ---- 1 + 2: the whole state against the model; derived data and the continuation -----------------------------------------------------------
N_MAX, N_MORE = 40, 25
_live = {}


def live():
    """System A, 3 streams (scenes 1234, 77, 4321), tracked until stream 1 has a non-empty failure queue and a bad point; then one
    keyframe of stream 1 is retired.  Everything the two tests below compare is gathered here, once."""
    if _live:
        return _live
    scs = [scene(1234, N_MAX + N_MORE), scene(77, N_MAX + N_MORE), scene(4321, N_MAX + N_MORE)]
    A = capi.System(capi.default_params(W, H, 3, **KW))
    for s, sc in enumerate(scs):
        start(A, s, sc)
    t = 0
    while t < N_MAX:
        A.track_frame(np.stack([sc[2][t] for sc in scs]))
        t += 1
        if A.idle_stats(1)["failure_queue"] > 0 and A.points(1)["bad"].any():
            break
    blob0 = A.snapshot(1).copy()
    h, s = rr.sections(blob0)
    fq = s[rr.FAIL_QUEUE].view(np.int32).reshape(-1, 2)
    src = s[rr.POINT_REST].reshape(-1, rr.REST_BYTES)[:, rr.REST_SRC_KF:rr.REST_SRC_KF + 4].copy().view(np.int32).reshape(-1)
    bad = s[rr.POINT_REST].reshape(-1, rr.REST_BYTES)[:, rr.REST_BAD:rr.REST_BAD + 4].copy().view(np.int32).reshape(-1)
    # r: a keyframe that is in the failure queue but not in all of its entries, and sources some points but not all
    cands = [k for k in range(1, h.n_kf - 1) if 0 < (fq[:, 0] == k).sum() < len(fq) and 0 < (src == k).sum() < len(src)]
    others = [dump(A, 0), dump(A, 2), readbacks(A, 0), readbacks(A, 2)]
    _live.update(A=A, scs=scs, t=t, blob0=blob0, fq_n=len(fq), n_bad=int((bad != 0).sum()), cands=cands, others=others)
    if cands:
        r = cands[len(cands) // 2]
        A.retire_keyframes([1], [r])
        _live.update(r=r, blob1=A.snapshot(1).copy(), info=A.retire_info(1), ms=A.retire_timing(),
                     others_after=[dump(A, 0), dump(A, 2), readbacks(A, 0), readbacks(A, 2)], info_others=[A.retire_info(0), A.retire_info(2)])
    return _live


def test_whole_state_against_the_model():
    """snapshot(1) after the retirement == retire_blob(snapshot(1) before, r) byte for byte; get_retire_info == the model's counts;
    streams 0 and 2 keep every bit of their dumps and read-backs."""
    L = live()
    assert L["fq_n"] > 0 and L["n_bad"] > 0, (L["t"], L["fq_n"], L["n_bad"])
    assert L["cands"], "no keyframe that is in part of the failure queue and sources part of the points"
    want, counts = rr.retire(L["blob0"], L["r"])
    got = L["blob1"]
    assert len(got) == len(want) and np.array_equal(got, want), (len(got), len(want), int((got[:min(len(got), len(want))] != want[:min(len(got), len(want))]).sum()))
    st0 = rr.TrackerState.from_buffer_copy(rr.sections(L["blob0"])[1][rr.STATE].tobytes())
    assert L["info"] == {"retired": 1, "keyframe": L["r"], "points_sourced": counts["points_sourced"], "points_bad": counts["points_bad"],
                         "queue_dropped": counts["queue_dropped"], "frame": st0.frame}, (L["info"], counts)
    assert counts["points_sourced"] > 0 and counts["points_bad"] > 0 and 0 < counts["queue_dropped"] < L["fq_n"]
    assert L["others_after"] == L["others"]
    assert L["info_others"] == [dict.fromkeys(L["info"], 0)] * 2
    assert L["ms"] > 0
    print("retired keyframe %d of %d: %d points sourced, %d bad, %d of %d queue entries; %.3f ms" %
          (L["r"], capi.snapshot_info(L["blob0"]).n_keyframes, counts["points_sourced"], counts["points_bad"], counts["queue_dropped"], L["fq_n"], L["ms"]))


def test_derived_data_and_the_continuation():
    """The model's blob restored into slot 0 of a system B with other capacities: right after, every read-back of A's stream 1 == B's
    slot 0, the keyframe corner lists of all levels, every keyframe's SmallBlurryImage and reloc_info among them (B has remade them from
    the pyramids; A has shifted its own); then 25 more frames on both with equal dumps after every frame, a keyframe among them."""
    L = live()
    assert L["cands"]
    A, scs, t0 = L["A"], L["scs"], L["t"]
    B = capi.System(capi.default_params(W, H, 2, **KW, max_points=4000, max_keyframes=24))
    B.restore(0, rr.retire_blob(L["blob0"], L["r"]))
    assert readbacks(A, 1) == readbacks(B, 0)
    assert derived(A, 1) == derived(B, 0)
    ra, rb = A.reloc_info(1), B.reloc_info(0)
    assert all(np.array_equal(ra[k], rb[k]) for k in ra)
    added = 0
    for t in range(t0, t0 + N_MORE):
        A.track_frame(np.stack([sc[2][t] for sc in scs]))
        B.track_frame(np.stack([scs[1][2][t]] * 2))
        assert dump(A, 1) == dump(B, 0), t
        added += A.state(1).kf_added
    assert added >= 1
    assert readbacks(A, 1) == readbacks(B, 0) and derived(A, 1) == derived(B, 0)
    assert A.state(1).quality == 2
    A.close(); B.close()
    _live.clear()


# ---- 3: where the loops split -------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)
CAP = dict(max_points=513, max_keyframes=5)          # the largest counts fill the system: the last slot and the last column move
OPT = dict(grow_map=3, relocalise=1, idle_iterations=1)


def randomised(blob, rng, r, mode):
    """The uploaded map's blob with every array a retirement touches filled with random bytes, the sources assigned by `mode` ("none":
    r sources no point, "some", "all but one": r sources every point but one, "bad only": some points bad and none sourced in r) -> blob"""
    h, s = rr.sections(blob)
    n, nk = h.n_points, h.n_kf
    rest = s[rr.POINT_REST].reshape(n, rr.REST_BYTES).copy()
    other = [k for k in range(nk) if k != r]
    if mode == "all but one":
        src = np.full(n, r); src[rng.integers(n)] = other[0]
    elif mode == "some":
        src = rng.integers(0, nk, n); src[0] = other[-1]
        if n > 1:
            src[n - 1] = r
    else:
        src = np.array(other)[rng.integers(0, len(other), n)]
    bad = np.zeros(n, np.int32)
    if mode == "bad only":
        bad[rng.random(n) < 0.3] = 1; bad[n - 1] = 1
    elif mode == "some" and n > 2:
        bad[rng.random(n) < 0.1] = 1
    for off, v in ((rr.REST_SRC_KF, src), (rr.REST_BAD, bad), (rr.REST_N_MEAS_KFS, rng.integers(2, 9, n))):
        rest[:, off:off + 4] = v.astype(np.int32).view(np.uint8).reshape(n, 4)
    s[rr.POINT_REST] = rest.reshape(-1)
    for sec in (rr.TRACKDATA, rr.TMPL, rr.PT_FLAGS, rr.PT_LEVEL, rr.CUR_MEAS, rr.NEVER_RETRY, rr.RELOC_SCORES):
        s[sec] = rng.integers(0, 256, len(s[sec]), dtype=np.uint8)
    fq = sorted({(int(rng.integers(nk)), int(rng.integers(n))) for _ in range(min(2 * n, 300))})
    it = rng.permutation(n)[:max(1, (2 * n) // 3)].astype(np.int32)
    s[rr.FAIL_QUEUE] = np.array(fq, np.int32).reshape(-1, 2).view(np.uint8).reshape(-1)
    s[rr.ITER_LIST] = it.view(np.uint8)
    st = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes())
    st.fq_n, st.n_iter, st.n_coarse, st.n_l3, st.newq_head = len(fq), len(it), len(it) // 3, len(it) // 4, int(rng.integers(n + 1))
    s[rr.STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    ri = rr.RelocInfo.from_buffer_copy(s[rr.RELOC_INFO].tobytes())
    ri.attempts, ri.best = 2, int(rng.integers(nk))
    s[rr.RELOC_INFO] = np.frombuffer(bytes(ri), np.uint8).copy()
    h.fq_n, h.n_iter = len(fq), len(it)
    return rr.assemble(h, s)


@pytest.mark.parametrize("w,h", [(48, 48), (50, 49), (130, 57), (128, 56)])
def test_where_the_loops_split(w, h):
    """No tracking.  Random maps are uploaded (random_map of test_gpu_snapshot.py), their snapshot is filled with random bytes in every
    array a retirement moves and restored, then one keyframe is retired and the stream's snapshot == the model's blob; a second system
    that restored the model's blob reads back the same, derived keyframe data included; the neighbouring stream keeps every bit.
    Point counts 1, 63, 64, 65, 255, 256, 257, 513 (the tile of the compaction is 2048 words: 157 TrackData, 97 MapPointDev); 3 and 5
    keyframes (5 fills the system) with r first, middle and last; r sources no point, some, or every point but one; and cases in which
    every dropped point is bad and none is sourced in r."""
    rng = np.random.default_rng(w * 1000 + h)
    g = capi.System(capi.default_params(w, h, 2, **CAP, **OPT))
    B = capi.System(capi.default_params(w, h, 1, max_points=600, max_keyframes=7, **OPT))
    nb = random_map(rng, w, h, 5, 513)
    g.load_map(0, nb)
    neighbour = readbacks(g, 0) + derived(g, 0)
    modes = ("none", "some", "all but one", "bad only")
    case = [(48, 48), (50, 49), (130, 57), (128, 56)].index((w, h))
    seen = set()
    for ci, n in enumerate(COUNTS):
        for nk in (3, 5):
            pos = ("first", "middle", "last")[(ci + (nk == 5) + case) % 3]
            mode = modes[(ci + 2 * (nk == 5) + case) % 4]
            if n == 1 and mode in ("some", "all but one"):
                mode = "bad only"
            r = {"first": 0, "middle": nk // 2, "last": nk - 1}[pos]
            seen.add((nk, pos, mode))
            tag = (w, h, n, nk, r, mode)
            g.reset([1]); g.load_map(1, random_map(rng, w, h, nk, n))
            blob0 = randomised(g.snapshot(1), rng, r, mode)
            g.restore(1, blob0)
            assert np.array_equal(g.snapshot(1), blob0), tag
            g.retire_keyframes([1], [r])
            want, counts = rr.retire(blob0, r)
            got = g.snapshot(1)
            assert len(got) == len(want) and np.array_equal(got, want), (tag, len(got), len(want))
            info = g.retire_info(1)
            assert (info["retired"], info["keyframe"], info["points_sourced"], info["points_bad"], info["queue_dropped"]) == \
                (1, r, counts["points_sourced"], counts["points_bad"], counts["queue_dropped"]), (tag, info, counts)
            if mode == "bad only":
                assert counts["points_sourced"] == 0 and counts["points_bad"] > 0, tag
            B.restore(0, want)
            assert readbacks(g, 1) == readbacks(B, 0) and derived(g, 1) == derived(B, 0), tag
            ra, rb = g.reloc_info(1), B.reloc_info(0)
            assert all(np.array_equal(ra[k], rb[k]) for k in ra), tag
    assert len({(nk, pos) for nk, pos, _ in seen}) == 6 and len({m for _, _, m in seen}) == 4, seen
    assert readbacks(g, 0) + derived(g, 0) == neighbour
    g.close(); B.close()


# ---- 4: a full map keeps growing ------------------------------------------------------------------------------------------------------
GROW = dict(grow_map=3, ba_sum_order=1, min_frames_between_kf=4, max_kf_dist_wiggle_mult=0.05, max_keyframes=4)
N_GROW = 14


def centres(poses):
    p = np.asarray(poses, np.float64).reshape(-1, 12)
    return np.stack([-q[:9].reshape(3, 3).T @ q[9:] for q in p])


def test_a_full_map_keeps_growing():
    """A map of 3 keyframes in a system with max_keyframes = 4, and parameters with which the unbounded oracle adds a keyframe every
    fifth frame.  keyframe_retire = 1: never more than 4 keyframes, kf_added fires at least 3 times, at least 2 retirements, each
    reporting the keyframe whose camera centre was farthest from the pose of that frame (numpy, from the poses read back just before;
    the two largest distances differ by far more than a fused multiply-add could move them), quality GOOD and no lost frame throughout.
    keyframe_retire = 0 on the same frames: stops at 4 keyframes (today's behaviour).
    The pose errors against the feeder's ground truth are printed for both (DESIGN.md records them: 2.55e-4 retiring, 1.54e-4 stopped at
    capacity, 2.01e-4 the unbounded oracle, after 14 frames); no bar is set on them."""
    f, m, frames = scene(1234, N_GROW, n_keyframes=3)
    unbounded = dict(GROW); del unbounded["max_keyframes"]
    o = make_oracle(capi.default_params(W, H, 1, **unbounded), m, f.pose(-1))
    okf = []
    for t in range(N_GROW):
        o.track_frame(frames[t])
        okf.append(o.state().kf_added)
    assert sum(okf) >= 3, okf                                        # the unbounded reference adds at least 3 keyframes on these frames
    err_unbounded = pose_err(o.state().pose, f.pose(N_GROW - 1))
    g = capi.System(capi.default_params(W, H, 1, keyframe_retire=1, **GROW))
    g0 = capi.System(capi.default_params(W, H, 1, keyframe_retire=0, **GROW))
    for x in (g, g0):
        start(x, 0, (f, m, frames))
    added = retired = 0
    for t in range(N_GROW):
        before = centres([g.keyframe_pose(0, k) for k in range(g.state(0).n_keyframes)])
        g.track_frame(frames[t]); g0.track_frame(frames[t])
        st, info = g.state(0), g.retire_info(0)
        assert st.n_keyframes <= 4 and st.quality == 2 and st.lost_frames == 0, (t, st.n_keyframes, st.quality, st.lost_frames)
        assert g0.state(0).n_keyframes <= 4
        added += st.kf_added
        if info["retired"] > retired:
            assert info["retired"] == retired + 1 and st.kf_added == 1 and info["frame"] == st.frame and len(before) == 4, (t, info)
            d = np.linalg.norm(before - centres([st.pose[:]])[0], axis=1)
            top = np.sort(d)[::-1]
            assert (top[0] - top[1]) > 1e-9 * top[0], (t, d)
            assert info["keyframe"] == int(np.argmax(d)), (t, info, d)
            assert info["points_sourced"] > 0
            retired += 1
    assert added >= 3 and retired >= 2 and g.state(0).n_keyframes == 4, (added, retired)
    s0 = g0.state(0)
    assert s0.n_keyframes == 4 and g0.retire_info(0)["retired"] == 0 and sum(okf) > 1      # without the feature the map stopped at its capacity
    err = pose_err(g.state(0).pose, f.pose(N_GROW - 1)), pose_err(s0.pose, f.pose(N_GROW - 1))
    print("pose error to the ground truth after %d frames: retiring %.3e, stopped at capacity %.3e, unbounded oracle %.3e; %d keyframes added, %d retired, %d points"
          % (N_GROW, err[0], err[1], err_unbounded, added, retired, g.state(0).n_points))
    g.close(); g0.close()


# ---- 5: gates --------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """VSLAM_E_STATE: a frame is open; the stream has no map; the map has 2 keyframes.  VSLAM_E_INVALID: an index outside the batch, a
    duplicate stream, a keyframe >= n_keyframes.  A call that lists one good and one refused stream retires neither.  dump of every stream
    is unchanged each time.  reset zeroes get_retire_info."""
    a = scene(1234, 4)
    two = scene(77, 4, n_keyframes=2)
    kw = dict(ba_sum_order=1, min_frames_between_kf=1000)            # no keyframe of the tracker's own: stream 1 stays at 2
    g = capi.System(capi.default_params(W, H, 3, **kw))
    start(g, 0, a); start(g, 1, two)                                 # stream 2 has no map
    g.track_frame(np.stack([a[2][0], two[2][0], a[2][0]]))
    nk = g.state(0).n_keyframes
    assert nk >= 8 and g.state(1).n_keyframes == 2 and g.state(2).n_keyframes == 0
    before = [dump(g, s) for s in range(3)]

    def unchanged():
        assert [dump(g, s) for s in range(3)] == before and [g.retire_info(s)["retired"] for s in range(3)] == [0, 0, 0]

    assert retire_rc(g, [2], [-1]) == E_STATE and retire_rc(g, [1], [0]) == E_STATE and retire_rc(g, [1], [-1]) == E_STATE
    assert retire_rc(g, [0, 1], [1, 0]) == E_STATE and retire_rc(g, [0, 2], [-1, -1]) == E_STATE
    unchanged()
    assert retire_rc(g, [0, 0], [1, 2]) == E_INVALID and retire_rc(g, [3], [0]) == E_INVALID and retire_rc(g, [-1], [0]) == E_INVALID
    assert retire_rc(g, [0], [nk]) == E_INVALID and retire_rc(g, [0], [1000]) == E_INVALID
    assert g.lib.vslam_retire_keyframes(g.h, None, None, 1) == E_INVALID and g.lib.vslam_retire_keyframes(g.h, None, None, -1) == E_INVALID
    unchanged()
    assert g.lib.vslam_retire_keyframes(g.h, None, None, 0) == 0
    ms = C.c_double(0.0)
    assert g.lib.vslam_get_retire_timing(g.h, C.byref(ms)) == E_STATE           # nothing has been retired yet
    unchanged()
    g.make_keyframe_lite(np.stack([a[2][1], two[2][1], a[2][1]])); g.patch_search(0)
    assert retire_rc(g, [0], [1]) == E_STATE
    g.pose_update(0); g.patch_search(1); g.pose_update(1); g.finish_frame()
    ref = capi.System(capi.default_params(W, H, 3, **kw))            # the same frames without the refused calls: the frame ended the same
    start(ref, 0, a); start(ref, 1, two)
    for t in range(2):
        ref.track_frame(np.stack([a[2][t], two[2][t], a[2][t]]))
    assert [dump(g, s) for s in range(3)] == [dump(ref, s) for s in range(3)]
    ref.close()
    g.retire_keyframes([0], [1])                                     # and the same call succeeds between frames
    info = g.retire_info(0)
    assert (info["retired"], info["keyframe"], info["frame"]) == (1, 1, 2) and g.state(0).n_keyframes == nk - 1
    g.retire_keyframes([0])                                          # by policy
    assert g.retire_info(0)["retired"] == 2 and g.state(0).n_keyframes == nk - 2
    g.track_frame(np.stack([a[2][2], two[2][2], a[2][2]]))           # the stream goes on
    assert g.state(0).quality == 2
    g.reset([0])
    assert g.retire_info(0) == dict.fromkeys(info, 0)
    g.close()


def test_a_pending_adjustment_is_refused_until_it_has_landed():
    """ba_delay_frames = 3: frame 0 is a keyframe frame; until its adjustment lands the call is refused with VSLAM_E_STATE and nothing
    changes; the same call succeeds once it has landed."""
    D, n = 3, 6
    a = scene(1234, n)
    g = capi.System(capi.default_params(W, H, 2, ba_delay_frames=D, ba_sum_order=1))
    start(g, 0, a)
    ok_at = None
    for t in range(n):
        g.track_frame(np.stack([a[2][t]] * 2))
        if ok_at is not None:
            continue
        before = [dump(g, s) for s in range(2)]
        rc = retire_rc(g, [0], [2])
        if rc == E_STATE:
            assert t < D and [dump(g, s) for s in range(2)] == before and g.retire_info(0)["retired"] == 0
        else:
            assert rc == 0 and t == D
            ok_at = t
            assert g.retire_info(0)["keyframe"] == 2 and g.state(0).n_keyframes == len(a[1]["keyframes"])   # 8 + the one of frame 0 - 1
    assert ok_at == D and g.state(0).quality == 2
    g.close()


def test_a_held_stream_at_capacity_is_not_touched():
    """keyframe_retire = 1, two streams on the same frames, both full and both with the keyframe request of their last frame still set
    (frame 5 retired and added a keyframe in both).  A subset step for stream 0 alone: stream 1, held, is bit-identical before and after
    (snapshot, dump, retire_info), although its state says "full, keyframe pending"."""
    f, m, frames = scene(1234, N_GROW, n_keyframes=3)
    g = capi.System(capi.default_params(W, H, 2, keyframe_retire=1, **GROW))
    for s in range(2):
        start(g, s, (f, m, frames))
    t = 0
    while t < N_GROW - 1:
        g.track_frame(np.stack([frames[t]] * 2))
        t += 1
        if g.retire_info(1)["retired"] == 1:
            break
    assert g.retire_info(0)["retired"] == g.retire_info(1)["retired"] == 1 and g.state(1).n_keyframes == 4 and g.state(1).kf_added == 1
    assert dump(g, 0) == dump(g, 1)
    before = g.snapshot(1).copy(), dump(g, 1), g.retire_info(1)
    g.track_frame_subset([0], frames[t])
    assert g.state(0).frame == t + 1 and g.state(1).frame == t
    after = g.snapshot(1).copy(), dump(g, 1), g.retire_info(1)
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
    g.close()


def test_the_automatic_path_beside_the_asynchronous_map_maker():
    """ba_delay_frames = 2 and ba_min_keyframes = 3, so every keyframe of the 4-keyframe map starts an adjustment that lands two frames
    later, before the next keyframe is due: the map still never exceeds 4 keyframes, keyframes and retirements go on, the adjustments
    run (n_ba_trials grows) on maps whose first, fixed keyframe has been retired, and while one is pending an explicit call is refused
    with VSLAM_E_STATE and changes nothing."""
    f, m, frames = scene(1234, N_GROW, n_keyframes=3)
    g = capi.System(capi.default_params(W, H, 1, keyframe_retire=1, ba_delay_frames=2, ba_min_keyframes=3, **GROW))
    start(g, 0, (f, m, frames))
    added = refused = 0
    for t in range(N_GROW):
        g.track_frame(frames[t])
        st = g.state(0)
        assert st.n_keyframes <= 4 and st.lost_frames == 0, (t, st.n_keyframes, st.lost_frames)
        added += st.kf_added
        if st.kf_added:
            before = dump(g, 0), g.retire_info(0)
            assert retire_rc(g, [0], [-1]) == E_STATE
            assert (dump(g, 0), g.retire_info(0)) == before
            refused += 1
    g.synchronize()
    st = g.state(0)
    assert added >= 3 and refused == added and g.retire_info(0)["retired"] >= 2 and st.n_keyframes == 4, (added, g.retire_info(0))
    assert st.n_ba_trials > 0 and st.quality == 2, (st.n_ba_trials, st.quality)
    g.close()
