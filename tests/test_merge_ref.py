"""CPU: the numpy model of the map merge (tests/merge_ref.py) held to three things that do not depend on it: a case written out by hand,
associativity on random blobs, and the model of keyframe retirement (tests/retire_ref.py) applied to what it makes."""
import ctypes as C

import numpy as np
import pytest

import merge_ref as mr
import retire_ref as rr


def make_blob(rng, w, h, nk, n, parts=rr.PART_IDLE | rr.PART_RELOC, fq=None, head=None, n_iter=None):
    """A well-formed snapshot blob with these counts: random bytes in every section, then the fields whose meaning the models read
    (src_kf in range, no bad point, a sorted failure queue, an iteration set of distinct points, a sane TrackerState)."""
    hd = rr.Header()
    hd.magic, hd.version, hd.header_bytes = b"VSLMSNAP", 1, C.sizeof(rr.Header)
    hd.width, hd.height, hd.patch_size, hd.quirks = w, h, 8, 0
    for i, v in enumerate((1.1, 1.2, 0.5, 0.5, 0.9)):
        hd.cam[i] = v
    if fq is None:
        fq = sorted({(int(rng.integers(nk)), int(rng.integers(n))) for _ in range(min(n, 20))}) if nk and n else []
    if not parts & rr.PART_IDLE:
        fq = []
    n_iter = min(n, 5) if n_iter is None else n_iter
    hd.n_kf, hd.n_points, hd.frame, hd.map_good, hd.n_iter, hd.fq_n, hd.parts = nk, n, 7, 1, n_iter, len(fq), parts
    secs = []
    for i in range(rr.N_SECTIONS):
        rows, rb = rr.section_rows(hd, i)
        secs.append(rng.integers(0, 256, rows * rb, dtype=np.uint8))
    rest = secs[rr.POINT_REST].reshape(n, rr.REST_BYTES)
    for off, v in ((rr.REST_SRC_KF, rng.integers(0, max(nk, 1), n)), (rr.REST_BAD, np.zeros(n)), (rr.REST_N_MEAS_KFS, rng.integers(2, 9, n))):
        rest[:, off:off + 4] = v.astype(np.int32).view(np.uint8).reshape(n, 4)
    if parts & rr.PART_IDLE:                                         # a set names keyframes of its own map only (the state's invariant)
        nr = secs[rr.NEVER_RETRY].view(np.uint64).reshape(n, 2)
        nr[:, 0] &= np.uint64((1 << min(nk, 64)) - 1)
        nr[:, 1] &= np.uint64((1 << max(nk - 64, 0)) - 1)
    secs[rr.FAIL_QUEUE] = np.array(fq, np.int32).reshape(-1, 2).view(np.uint8).reshape(-1)
    secs[rr.ITER_LIST] = rng.permutation(max(n, 1))[:n_iter].astype(np.int32).view(np.uint8)
    secs[rr.KF_FIXED] = (np.arange(nk) == 0).astype(np.int32).view(np.uint8)
    st = rr.TrackerState()
    for k in range(12):
        st.pose_final[k] = rng.normal()
    st.frame, st.map_good, st.quality, st.n_points, st.n_kf = 7, 1, 2, n, nk
    st.n_iter, st.n_coarse, st.n_l3 = n_iter, n_iter // 3, n_iter // 4
    st.ba_converged_recent, st.ba_converged_full, st.ba_countdown = 1, 1, -1
    st.newq_head, st.fq_n = (int(rng.integers(n + 1)) if head is None else head), len(fq)
    st.n_refound_new, st.pvs_seed = int(rng.integers(100)), int(rng.integers(1, 1000))
    secs[rr.STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    if parts & rr.PART_RELOC:
        ri = rr.RelocInfo.from_buffer_copy(secs[rr.RELOC_INFO].tobytes())
        ri.attempts, ri.best = 2, int(rng.integers(max(nk, 1)))
        secs[rr.RELOC_INFO] = np.frombuffer(bytes(ri), np.uint8).copy()
    return rr.assemble(hd, secs)


def test_a_case_written_out_by_hand():
    """d: 2 keyframes, 3 points; s: 1 keyframe, 2 points; one never-retry bit and one queue entry each.  Every section of the result is
    stated here from the two inputs by slicing, without the model's code."""
    rng = np.random.default_rng(1)
    bd = make_blob(rng, 48, 48, 2, 3, fq=[(1, 2)], head=1)
    bs = make_blob(rng, 48, 48, 1, 2, fq=[(0, 1)], head=2)
    hd, d = rr.sections(bd)
    hs, s = rr.sections(bs)
    d[rr.NEVER_RETRY] = np.array([0, 0, 2, 0, 0, 0], np.uint64).view(np.uint8)          # point 1 of d never retries keyframe 1
    s[rr.NEVER_RETRY] = np.array([0, 0, 0xff01, 0xff], np.uint64).view(np.uint8)        # point 1 of s: keyframe 0, and rubbish above its one keyframe
    s[rr.PT_FLAGS] = np.array([63, 16 | 2], np.int32).view(np.uint8)
    s[rr.POINT_REST].reshape(2, 80)[:, 48:52] = np.zeros(2, np.int32).view(np.uint8).reshape(2, 4)
    bd, bs = rr.assemble(hd, d), rr.assemble(hs, s)
    got, counts = mr.merge(bd, bs)
    assert counts == {"keyframes": 1, "points": 2, "queue": 1}
    h, g = rr.sections(got)
    assert (h.n_kf, h.n_points, h.fq_n, h.n_iter, h.parts) == (3, 5, 2, hd.n_iter, hd.parts)
    for sec in (rr.POINT_POS, rr.TRACKDATA, rr.TMPL, rr.KF_POSE, rr.KF_DEPTH, rr.KF_IMG0, rr.KF_IMG1, rr.KF_IMG2, rr.KF_IMG3):
        assert np.array_equal(g[sec], np.r_[d[sec], s[sec]]), sec
    rest = g[rr.POINT_REST].reshape(5, 80)
    assert np.array_equal(rest[:3], d[rr.POINT_REST].reshape(3, 80))
    assert list(rest[3:, 48:52].copy().view(np.int32).reshape(-1)) == [2, 2]             # src_kf 0 of s is keyframe 2 of d
    assert np.array_equal(np.delete(rest[3:], np.s_[48:52], axis=1), np.delete(s[rr.POINT_REST].reshape(2, 80), np.s_[48:52], axis=1))
    assert list(g[rr.PT_FLAGS].view(np.int32)[3:]) == [48, 16] and np.array_equal(g[rr.PT_FLAGS][:12], d[rr.PT_FLAGS])
    assert list(g[rr.PT_LEVEL].view(np.int32)[3:]) == [-1, -1] and np.array_equal(g[rr.PT_LEVEL][:12], d[rr.PT_LEVEL])
    assert np.array_equal(g[rr.CUR_MEAS], np.r_[d[rr.CUR_MEAS], np.zeros(48, np.uint8)])
    assert list(g[rr.KF_FIXED].view(np.int32)) == [1, 0, 0]
    m = g[rr.KF_MEAS].reshape(3, 5, 24)
    assert np.array_equal(m[:2, :3], d[rr.KF_MEAS].reshape(2, 3, 24)) and np.array_equal(m[2:, 3:], s[rr.KF_MEAS].reshape(1, 2, 24))
    assert not m[:2, 3:].any() and not m[2:, :3].any()
    assert list(g[rr.NEVER_RETRY].view(np.uint64)) == [0, 0, 2, 0, 0, 0, 0, 0, 4, 0]     # bit 0 of s -> bit 2; nothing above s's one keyframe
    assert [tuple(e) for e in g[rr.FAIL_QUEUE].view(np.int32).reshape(-1, 2)] == [(1, 2), (2, 4)]
    assert np.array_equal(g[rr.RELOC_SCORES], np.r_[d[rr.RELOC_SCORES], np.zeros(8, np.uint8)])
    for sec in (rr.ITER_LIST, rr.RELOC_INFO, rr.RELOC_CUR_TMPL, rr.SBI_SMALL, rr.SBI_TMPL, rr.SBI_JACS, rr.SBI_ROT):
        assert np.array_equal(g[sec], d[sec]), sec
    st0, st1 = rr.TrackerState.from_buffer_copy(d[rr.STATE].tobytes()), rr.TrackerState.from_buffer_copy(g[rr.STATE].tobytes())
    assert (st1.n_kf, st1.n_points, st1.fq_n, st1.newq_head, st1.ba_converged_recent, st1.ba_converged_full) == (3, 5, 2, 1, 0, 0)
    st1.n_kf, st1.n_points, st1.fq_n, st1.ba_converged_recent, st1.ba_converged_full = 2, 3, 1, 1, 1
    assert bytes(st1) == bytes(st0)                                                      # every other byte of the state is d's


@pytest.mark.parametrize("seed", range(6))
def test_associativity_on_random_blobs(seed):
    """merge(merge(a, b), c) == merge(a, merge(b, c)) byte for byte, STATE included: the head stays a's, the flags are 0 either way, the
    shifts of the never-retry sets and of the queue compose; counts around the word boundary of the sets among them."""
    rng = np.random.default_rng(seed)
    w, h = ((48, 48), (50, 49))[seed % 2]
    nks = ((1, 1, 1), (3, 2, 4), (63, 1, 2), (60, 4, 3), (2, 62, 3), (1, 64, 63))[seed]
    nps = ((0, 1, 2), (5, 0, 3), (7, 9, 1), (1, 1, 1), (4, 6, 0), (3, 2, 5))[seed]
    parts = rr.PART_IDLE | rr.PART_RELOC if seed != 4 else 0
    a, b, c = (make_blob(rng, w, h, nks[i], nps[i], parts=parts | (rr.PART_SBI if i == 0 else 0)) for i in range(3))
    left, right = mr.merge_blob(mr.merge_blob(a, b), c), mr.merge_blob(a, mr.merge_blob(b, c))
    assert len(left) == len(right) and np.array_equal(left, right)
    hd, s = rr.sections(left)
    assert (hd.n_kf, hd.n_points) == (sum(nks), sum(nps))
    st, sta = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes()), rr.TrackerState.from_buffer_copy(rr.sections(a)[1][rr.STATE].tobytes())
    assert st.newq_head == sta.newq_head and bytes(st.pose_final) == bytes(sta.pose_final)
    src = s[rr.POINT_REST].reshape(-1, 80)[:, 48:52].copy().view(np.int32).reshape(-1)
    lo = np.repeat(np.cumsum((0,) + nks[:2]), nps)
    assert ((src >= lo) & (src < lo + np.repeat(nks, nps))).all()    # every point is sourced in a keyframe of its own part


def test_retiring_an_appended_keyframe_drops_exactly_its_points():
    """retire_ref.retire on the merged blob, for a keyframe that came from the source: the points it drops are the source's points
    sourced there, under their new indices -- the renumbered src_kf is what decides it."""
    rng = np.random.default_rng(5)
    bd, bs = make_blob(rng, 48, 48, 3, 11), make_blob(rng, 48, 48, 3, 9)
    merged = mr.merge_blob(bd, bs)
    _, s = rr.sections(bs)
    src_s = s[rr.POINT_REST].reshape(9, 80)[:, 48:52].copy().view(np.int32).reshape(-1)
    for k in range(3):
        out, counts = rr.retire(merged, 3 + k)
        assert counts["points_sourced"] == int((src_s == k).sum()) and counts["points_bad"] == 0
        ho, so = rr.sections(out)
        _, sm = rr.sections(merged)
        keep = np.r_[np.ones(11, bool), src_s != k]
        assert ho.n_points == keep.sum() and ho.n_kf == 5
        assert np.array_equal(so[rr.POINT_POS].reshape(-1, 24), sm[rr.POINT_POS].reshape(-1, 24)[keep])
        assert np.array_equal(so[rr.TMPL].reshape(-1, 128), sm[rr.TMPL].reshape(-1, 128)[keep])
