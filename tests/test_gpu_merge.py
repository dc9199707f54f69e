"""GPU: map merge -- vslam_merge_maps, vslam_get_merge_info, vslam_get_merge_timing (csrc/merge.hip, the index rules in csrc/merge_dev.h).

The reference cannot merge (its Map is one heap object), so the yardstick is the independent numpy model of tests/merge_ref.py, by the
method of tests/test_gpu_retire.py: a stream's snapshot inventories its whole state, so snapshot(d after) == merge(snapshot(d before),
snapshot(s before)), byte for byte, says the device did what the model states and nothing else.  What a snapshot does not carry (keyframe
corner lists, keyframe SmallBlurryImages) is compared with a second system that restored the model's blob and remade them, and the
continuation is compared with that system frame by frame.  One test does not go through the model: the merged stream against the same
union uploaded through the map upload."""
import ctypes as C

import numpy as np
import pytest

import merge_ref as mr
import retire_ref as rr
from test_gpu_reset import dump
from test_gpu_retire import scene, start
from test_gpu_snapshot import derived, random_map, readbacks
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

W, H = 640, 480
E_INVALID, E_CAPACITY, E_STATE = -1, -3, -4
OPT = dict(grow_map=3, relocalise=1, idle_iterations=1)
IDLE_STATS = 7                   # position of idle_stats in readbacks(): dump() has seven entries in front of it


def merge_rc(g, dst, src, n=None):
    a, b = np.array(dst, np.int32), np.array(src, np.int32)
    return g.lib.vslam_merge_maps(g.h, a.ctypes.data, b.ctypes.data, len(a) if n is None else n)


def same(a, b):
    return len(a) == len(b) and np.array_equal(a, b)


def union(a, b):
    """A (+) B on the host: keyframes A then B with B's fixed cleared, points A then B with src_kf + nk_A, measurements with both indices offset"""
    nk, n = len(a["keyframes"]), len(a["points"])
    kfs = list(a["keyframes"]) + [dict(k, fixed=False) for k in b["keyframes"]]
    pts = list(a["points"]) + [dict(p, src_kf=p["src_kf"] + nk) for p in b["points"]]
    meas = list(a["meas"]) + [(x[0] + nk, x[1] + n) + tuple(x[2:]) for x in b["meas"]]
    return {"keyframes": kfs, "points": pts, "meas": meas}


# ---- 1: against the map upload, no model involved --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(48, 48), (50, 49)])
def test_against_the_map_upload(w, h):
    """Random maps A and B uploaded into slots 0 and 1, merged 0 <- 1; slot 2 is given A (+) B built on the host.  Every snapshot section
    but the tracker state is equal byte for byte, and so are the read-backs (without the idle statistics: the new queue differs by
    design) and the derived keyframe data, which the merge copied and the upload remade.  The state is the model's.  Slot 1 keeps every bit."""
    rng = np.random.default_rng(w + h)
    g = capi.System(capi.default_params(w, h, 3, max_points=200, max_keyframes=6, **OPT))
    A, B = random_map(rng, w, h, 2, 70), random_map(rng, w, h, 3, 65)
    g.load_map(0, A); g.load_map(1, B); g.load_map(2, union(A, B))
    b0, b1 = g.snapshot(0).copy(), g.snapshot(1).copy()
    src_before = readbacks(g, 1) + derived(g, 1)
    g.merge_maps([0], [1])
    got, up = g.snapshot(0).copy(), g.snapshot(2).copy()
    hg, sg = rr.sections(got)
    hu, su = rr.sections(up)
    assert (hg.n_kf, hg.n_points, hg.parts) == (hu.n_kf, hu.n_points, hu.parts) == (5, 135, hu.parts)
    for sec in range(rr.N_SECTIONS):
        if sec != rr.STATE:
            assert same(sg[sec], su[sec]), sec
    ra, rb = readbacks(g, 0), readbacks(g, 2)
    del ra[IDLE_STATS], rb[IDLE_STATS]
    assert ra == rb and derived(g, 0) == derived(g, 2)
    assert same(got, mr.merge_blob(b0, b1))
    assert same(g.snapshot(1), b1) and readbacks(g, 1) + derived(g, 1) == src_before
    assert g.merge_info(0) == {"merged": 1, "source": 1, "keyframes": 3, "points": 65, "queue": 0, "frame": 0}
    assert g.merge_info(1) == g.merge_info(2) == dict.fromkeys(g.merge_info(0), 0)
    g.close()


# ---- 2: where the loops split ----------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
SIZES = [(48, 48), (50, 49), (130, 57), (128, 56)]


def point_cases():
    """(np_d, np_s): every count as the destination's against a source of less and of more than a block, every count as the source's
    behind an empty destination and behind one that ends on a block boundary, and the pair that fills max_points: 29 pairs"""
    out = [(a, b) for a in COUNTS for b in (1, 65)] + [(a, b) for a in (0, 64) for b in COUNTS] + [(257, 257)]
    return sorted(set(out))


def randomised(blob, rng):
    """The uploaded map's blob with every array the merge reads filled with random bytes (as randomised() of test_gpu_retire.py does for
    the retirement): sources, bad flags, TrackData, templates, flags with all six bits, levels, cur_meas, never-retry sets limited to the
    map's keyframes, a sorted random failure queue, newq_head, RelocInfo, scores -> blob"""
    h, s = rr.sections(blob)
    n, nk = h.n_points, h.n_kf
    rest = s[rr.POINT_REST].reshape(n, rr.REST_BYTES).copy()
    for off, v in ((rr.REST_SRC_KF, rng.integers(0, nk, n)), (rr.REST_BAD, rng.random(n) < 0.1), (rr.REST_N_MEAS_KFS, rng.integers(2, 9, n))):
        rest[:, off:off + 4] = np.asarray(v).astype(np.int32).view(np.uint8).reshape(n, 4)
    s[rr.POINT_REST] = rest.reshape(-1)
    for sec in (rr.TRACKDATA, rr.TMPL, rr.PT_LEVEL, rr.CUR_MEAS, rr.NEVER_RETRY, rr.RELOC_SCORES):
        s[sec] = rng.integers(0, 256, len(s[sec]), dtype=np.uint8)
    s[rr.PT_FLAGS] = rng.integers(0, 64, n).astype(np.int32).view(np.uint8)
    nr = s[rr.NEVER_RETRY].view(np.uint64).reshape(n, 2)
    nr[:, 0] &= np.uint64((1 << min(nk, 64)) - 1)
    nr[:, 1] &= np.uint64((1 << max(nk - 64, 0)) - 1)
    fq = sorted({(int(rng.integers(nk)), int(rng.integers(n))) for _ in range(min(2 * n, 300))}) if n else []
    it = rng.permutation(n)[:(2 * n) // 3].astype(np.int32)
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


@pytest.mark.parametrize("w,h", SIZES)
def test_where_the_loops_split(w, h):
    """No tracking.  Random maps are uploaded into slots 0 and 1, their snapshots are filled with random bytes in every array the merge
    reads and restored; then 0 <- 1 and snapshot(0) == the model's blob, merge_info == the model's counts, a second system that restored
    the model's blob reads back the same, derived keyframe data included; the source and a neighbour filled to capacity keep every bit.
    Point counts 0, 1, 63, 64, 65, 255, 256, 257 on either side (a block of the point mover is 256 points; 257 + 257 fills max_points);
    keyframes 1 and 2 + 1 and 3 (2 + 3 fills max_keyframes), and at 48 x 48 also 63, 64 and 65 + 1 and 3 in a system of 68, across the
    word boundary of the never-retry sets.  The last case runs behind a capacity-filling map that was reset."""
    rng = np.random.default_rng(w * 1000 + h)
    small = (w, h) == (48, 48)
    K, P = (68 if small else 5), 514
    kf_cases = [(a, b) for a in ((1, 2, 63, 64, 65) if small else (1, 2)) for b in (1, 3)]
    g = capi.System(capi.default_params(w, h, 3, max_points=P, max_keyframes=K, **OPT))
    B = capi.System(capi.default_params(w, h, 1, max_points=600, max_keyframes=K + 2, **OPT))
    full = random_map(rng, w, h, K, P)
    g.load_map(2, full)
    neighbour = readbacks(g, 2) + derived(g, 2)
    cases = point_cases()
    filled = False
    for ci, (np_d, np_s) in enumerate(cases + [cases[len(cases) // 2]]):
        nk_d, nk_s = kf_cases[(ci + SIZES.index((w, h))) % len(kf_cases)]
        if (np_d, np_s) == (257, 257):
            nk_d, nk_s = kf_cases[-1]                                # both capacities at equality in one case
            filled = True
        tag = (w, h, nk_d, np_d, nk_s, np_s)
        if ci == len(cases):                                         # behind a reset: what the full map left above the new counts must not show
            g.reset([0]); g.load_map(0, full); g.reset([0])
        blobs = []
        for slot, (nk, n) in enumerate(((nk_d, np_d), (nk_s, np_s))):
            g.reset([slot]); g.load_map(slot, random_map(rng, w, h, nk, n))
            blobs.append(randomised(g.snapshot(slot), rng))
            g.restore(slot, blobs[slot])
            assert same(g.snapshot(slot), blobs[slot]), (tag, slot)
        src_before = readbacks(g, 1) + derived(g, 1)
        g.merge_maps([0], [1])
        want, counts = mr.merge(blobs[0], blobs[1])
        got = g.snapshot(0)
        assert same(got, want), (tag, len(got), len(want))
        info = g.merge_info(0)
        assert info == {"merged": 1, "source": 1, "keyframes": counts["keyframes"], "points": counts["points"], "queue": counts["queue"], "frame": 0}, (tag, info, counts)
        B.restore(0, want)
        assert readbacks(g, 0) == readbacks(B, 0) and derived(g, 0) == derived(B, 0), tag
        ra, rb = g.reloc_info(0), B.reloc_info(0)
        assert all(np.array_equal(ra[k], rb[k]) for k in ra), tag
        assert same(g.snapshot(1), blobs[1]) and readbacks(g, 1) + derived(g, 1) == src_before, tag
    assert filled and readbacks(g, 2) + derived(g, 2) == neighbour
    g.close(); B.close()


# ---- 3 + 4: a live pair, the continuation, the new queue ---------------------------------------------------------------------------------
LIVE = dict(ba_sum_order=1, grow_map=3, relocalise=1)
N_PRE, N_MORE = 3, 25


def halves(m):
    """One map of 8 keyframes split on the host: keyframes 0-3 and 4-7, each with the points it sources and the measurements inside the
    half; the second half's first keyframe is fixed -> (first, second, measurements dropped because they crossed the halves)"""
    out, dropped = [], 0
    for lo, hi in ((0, 4), (4, 8)):
        kfs = [dict(k) for k in m["keyframes"][lo:hi]]
        kfs[0]["fixed"] = True
        idx = [i for i, p in enumerate(m["points"]) if lo <= p["src_kf"] < hi]
        new = {p: i for i, p in enumerate(idx)}
        pts = [dict(m["points"][i], src_kf=m["points"][i]["src_kf"] - lo) for i in idx]
        meas = [(x[0] - lo, new[x[1]]) + tuple(x[2:]) for x in m["meas"] if lo <= x[0] < hi and x[1] in new]
        dropped += sum(1 for x in m["meas"] if x[1] in new and not lo <= x[0] < hi)
        out.append({"keyframes": kfs, "points": pts, "meas": meas})
    return out[0], out[1], dropped


def test_a_live_pair_and_the_continuation():
    """Streams 0 and 1 hold the halves of one map and have tracked three frames, so TrackData, flags and templates are live; stream 2
    holds only the first half, stream 3 the whole map.  0 <- 1: snapshot(0) == the model's blob; streams 2 and 3 keep every bit, and so
    does 1.  A system B restores the model's blob; 25 more frames on both with equal dumps after every frame, a keyframe among them,
    quality GOOD and no frame lost.  The found counts of the merged stream are printed beside those of stream 2 (no bar)."""
    f, m, frames = scene(1234, 65)                                # the scene tests/test_gpu_retire.py and test_gpu_transform.py render: one cache entry
    first, second, dropped = halves(m)
    assert dropped > 0 and len(first["points"]) > 50 and len(second["points"]) > 50, (dropped, len(first["points"]), len(second["points"]))
    A = capi.System(capi.default_params(W, H, 4, **LIVE))
    for s, part in enumerate((first, second, first, m)):
        A.load_map(s, part); A.set_pose(s, f.pose(-1))
    for t in range(N_PRE):
        A.track_frame(np.stack([frames[t]] * 4))
    assert all(A.state(s).quality == 2 for s in range(4))
    b0, b1 = A.snapshot(0).copy(), A.snapshot(1).copy()
    others = [dump(A, s) for s in (1, 2, 3)] + [readbacks(A, s) for s in (1, 2, 3)]
    A.merge_maps([0], [1])
    want, counts = mr.merge(b0, b1)
    assert same(A.snapshot(0), want)
    assert counts["keyframes"] >= 4 and counts["points"] == A.state(1).n_points
    assert A.merge_info(0) == {"merged": 1, "source": 1, "keyframes": counts["keyframes"], "points": counts["points"], "queue": 0, "frame": N_PRE}
    assert others == [dump(A, s) for s in (1, 2, 3)] + [readbacks(A, s) for s in (1, 2, 3)] and same(A.snapshot(1), b1)
    ms = A.merge_timing()
    assert ms > 0
    B = capi.System(capi.default_params(W, H, 1, max_points=4000, max_keyframes=24, **LIVE))
    B.restore(0, want)
    assert readbacks(A, 0) == readbacks(B, 0) and derived(A, 0) == derived(B, 0)
    added, found = 0, []
    for t in range(N_PRE, N_PRE + N_MORE):
        A.track_frame(np.stack([frames[t]] * 4)); B.track_frame(frames[t][None])
        assert dump(A, 0) == dump(B, 0), t
        st = A.state(0)
        assert st.quality == 2 and st.lost_frames == 0, (t, st.quality, st.lost_frames)
        added += st.kf_added
        found.append((sum(st.found[:]), sum(A.state(2).found[:])))
    assert added >= 1
    assert readbacks(A, 0) == readbacks(B, 0) and derived(A, 0) == derived(B, 0)
    print("merge of %d + %d keyframes, %d + %d points: %.3f ms; found per frame, merged / first half only: %s" %
          (4, counts["keyframes"], rr.sections(b0)[0].n_points, counts["points"], ms, found))
    A.close(); B.close()


def test_the_new_queue_holds_the_appended_points():
    """idle_iterations = 1: right after a merge the new queue is d's pending points and every point of s; after a few frames the stream
    is GOOD.  n_refound_new is printed (no bar): it is the number that shows the parts being tied together."""
    f, m, frames = scene(1234, 65)                                # the scene tests/test_gpu_retire.py and test_gpu_transform.py render: one cache entry
    first, second, _ = halves(m)
    g = capi.System(capi.default_params(W, H, 2, idle_iterations=1, **LIVE))
    for s, part in enumerate((first, second)):
        g.load_map(s, part); g.set_pose(s, f.pose(-1))
    for t in range(2):
        g.track_frame(np.stack([frames[t]] * 2))
    pending, refound0 = g.idle_stats(0)["new_queue"], g.idle_stats(0)["refound_new"]
    np_s = g.state(1).n_points
    g.merge_maps([0], [1])
    assert g.idle_stats(0)["new_queue"] == pending + np_s
    for t in range(2, 8):
        g.track_frame(np.stack([frames[t]] * 2))
    assert g.state(0).quality == 2
    print("n_refound_new %d -> %d after 6 frames, new queue %d -> %d" % (refound0, g.idle_stats(0)["refound_new"], pending + np_s, g.idle_stats(0)["new_queue"]))
    g.close()


# ---- 5 + 6: associativity on the device; several pairs in one call -----------------------------------------------------------------------
def test_associativity_on_the_device():
    """Three maps in two systems: (0 <- 1) then (0 <- 2) against (1 <- 2) then (0 <- 1): the snapshots of slot 0 are equal"""
    rng = np.random.default_rng(9)
    maps = [random_map(rng, 48, 48, nk, n) for nk, n in ((2, 40), (3, 65), (1, 70))]
    x, y = (capi.System(capi.default_params(48, 48, 3, max_points=200, max_keyframes=6, **OPT)) for _ in range(2))
    for g in (x, y):
        for s in range(3):
            g.load_map(s, maps[s])
    x.merge_maps([0], [1]); x.merge_maps([0], [2])
    y.merge_maps([1], [2]); y.merge_maps([0], [1])
    assert same(x.snapshot(0), y.snapshot(0))
    assert x.merge_info(0)["merged"] == 2 and y.merge_info(0) == {"merged": 1, "source": 1, "keyframes": 4, "points": 135, "queue": 0, "frame": 0}
    x.close(); y.close()


def test_several_pairs_in_one_call():
    """merge_maps([0, 2], [1, 3]) gives the snapshots two separate calls give"""
    rng = np.random.default_rng(10)
    maps = [random_map(rng, 50, 49, nk, n) for nk, n in ((2, 40), (3, 65), (1, 257), (2, 1))]
    x, y = (capi.System(capi.default_params(50, 49, 4, max_points=300, max_keyframes=6, **OPT)) for _ in range(2))
    for g in (x, y):
        for s in range(4):
            g.load_map(s, maps[s])
    x.merge_maps([0, 2], [1, 3])
    y.merge_maps([0], [1]); y.merge_maps([2], [3])
    for s in range(4):
        assert same(x.snapshot(s), y.snapshot(s)), s
        assert x.merge_info(s) == y.merge_info(s)
    assert x.merge_info(2) == {"merged": 1, "source": 3, "keyframes": 2, "points": 1, "queue": 0, "frame": 0}
    x.close(); y.close()


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    """Every VSLAM_E_INVALID and VSLAM_E_STATE case and VSLAM_E_CAPACITY at one keyframe and at one point over: dump and merge_info of
    every stream are unchanged each time.  The exact fit succeeds; a call with one good and one refused pair merges neither; after
    retire_keyframes has made room the merge refused for keyframes succeeds; reset zeroes merge_info; the timing is refused before the
    first merge and positive after."""
    rng = np.random.default_rng(11)
    w, h, S = 48, 48, 6
    g = capi.System(capi.default_params(w, h, S, max_points=100, max_keyframes=6, **OPT))
    maps = {0: (3, 40), 1: (3, 60), 2: (4, 10), 3: (1, 61), 4: (2, 5)}   # stream 5 has no map
    for s, (nk, n) in maps.items():
        g.load_map(s, random_map(rng, w, h, nk, n))
    before = [dump(g, s) for s in range(S)]
    zero = dict.fromkeys(("merged", "source", "keyframes", "points", "queue", "frame"), 0)

    def unchanged():
        assert [dump(g, s) for s in range(S)] == before and all(g.merge_info(s) == zero for s in range(S))

    ms = C.c_double(0.0)
    assert g.lib.vslam_get_merge_timing(g.h, C.byref(ms)) == E_STATE
    for dst, src in (([6], [0]), ([0], [-1]), ([0], [0]), ([0, 0], [1, 4]), ([0, 4], [1, 0]), ([0, 4], [1, 1]), ([4, 1], [0, 4])):
        assert merge_rc(g, dst, src) == E_INVALID, (dst, src)
        assert b"merge" in g.lib.vslam_last_error()
    assert g.lib.vslam_merge_maps(g.h, None, None, 1) == E_INVALID and g.lib.vslam_merge_maps(g.h, None, None, -1) == E_INVALID
    unchanged()
    assert g.lib.vslam_merge_maps(g.h, None, None, 0) == 0
    unchanged()
    assert merge_rc(g, [5], [0]) == E_STATE and merge_rc(g, [0], [5]) == E_STATE and merge_rc(g, [4, 0], [3, 5]) == E_STATE
    unchanged()
    assert merge_rc(g, [0], [2]) == E_CAPACITY                       # 3 + 4 keyframes of 6
    assert b"3 + 4" in g.lib.vslam_last_error() and b"6" in g.lib.vslam_last_error()
    assert merge_rc(g, [0], [3]) == E_CAPACITY                       # 40 + 61 points of 100
    assert b"40 + 61" in g.lib.vslam_last_error() and b"100" in g.lib.vslam_last_error()
    assert merge_rc(g, [4, 0], [3, 2]) == E_CAPACITY                 # one good pair beside a refused one: neither
    unchanged()
    g.make_keyframe_lite(rng.integers(0, 256, (S, h, w), dtype=np.uint8)); g.patch_search(0)
    assert merge_rc(g, [0], [1]) == E_STATE
    g.pose_update(0); g.patch_search(1); g.pose_update(1); g.finish_frame()
    before = [dump(g, s) for s in range(S)]
    g.merge_maps([0], [1])                                           # the exact fit: 3 + 3 keyframes of 6, 40 + 60 points of 100
    assert g.merge_info(0) == dict(zero, merged=1, source=1, keyframes=3, points=60, frame=1) and g.state(0).n_keyframes == 6 and g.state(0).n_points == 100
    assert [dump(g, s) for s in range(1, S)] == before[1:]
    assert g.merge_timing() > 0
    assert merge_rc(g, [2], [1]) == E_CAPACITY                       # 4 + 3 keyframes
    g.retire_keyframes([2], [1])
    n2 = g.state(2).n_points
    g.merge_maps([2], [1])
    assert g.state(2).n_keyframes == 6 and g.merge_info(2) == dict(zero, merged=1, source=1, keyframes=3, points=60, frame=1) and g.state(2).n_points == n2 + 60
    g.reset([0])
    assert g.merge_info(0) == zero and g.merge_info(2)["merged"] == 1
    g.close()


def test_a_pending_adjustment_is_refused_until_it_has_landed():
    """ba_delay_frames = 3: frame 0 is a keyframe frame of stream 0; until its adjustment lands the merge is refused with VSLAM_E_STATE,
    with the stream as destination and as source, and nothing changes; the same call succeeds once it has landed."""
    D, n = 3, 6
    a = scene(1234, n)
    first, second, _ = halves(a[1])
    g = capi.System(capi.default_params(W, H, 3, ba_delay_frames=D, ba_sum_order=1, max_keyframes=40))
    start(g, 0, a)
    for s, part in ((1, first), (2, second)):
        g.load_map(s, part); g.set_pose(s, a[0].pose(-1))
    ok_at = None
    for t in range(n):
        g.track_frame(np.stack([a[2][t]] * 3))
        if ok_at is not None:
            continue
        pending = [s for s in range(3) if g.state(s).kf_added]
        before = [dump(g, s) for s in range(3)]
        rc = merge_rc(g, [0], [1])
        if rc == E_STATE:
            assert t < D and merge_rc(g, [1], [0]) == E_STATE and [dump(g, s) for s in range(3)] == before and g.merge_info(0)["merged"] == 0, (t, pending)
        else:
            assert rc == 0 and t == D, (rc, t)
            ok_at = t
            assert g.merge_info(0)["source"] == 1 and g.merge_info(0)["frame"] == t + 1
    assert ok_at == D
    g.close()
