"""CPU test: the numpy model of keyframe retirement (tests/retire_ref.py) against values written out here, on hand-built snapshot blobs."""
import ctypes as C

import numpy as np

import retire_ref as rr
from visualslam_android_amd import capi

W, H = 48, 48


def tagged(n, eb, tag):
    """n elements of eb bytes; every byte of element i is tag + i, so a moved element is recognised wherever it lands"""
    return np.repeat(((tag + np.arange(n)) % 256).astype(np.uint8), eb)


def build(nk, pts, valid, fq=(), iter_list=(), n_coarse=0, n_l3=0, newq_head=0, never_retry=None, fixed=None, best=0, parts=rr.PART_IDLE | rr.PART_RELOC):
    """A well-formed blob: pts = [(src_kf, bad, n_meas_kfs)], valid[k][i] = keyframe k measures point i"""
    n = len(pts)
    h = rr.Header()
    h.magic, h.version, h.header_bytes = b"VSLMSNAP", 1, C.sizeof(rr.Header)
    h.width, h.height, h.patch_size, h.quirks = W, H, 11, 0
    h.n_kf, h.n_points, h.frame, h.map_good, h.n_iter, h.fq_n, h.parts = nk, n, 7, 1, len(iter_list), len(fq), parts
    st = rr.TrackerState()
    st.n_kf, st.n_points, st.frame, st.map_good, st.quality = nk, n, 7, 1, 2
    st.n_iter, st.n_coarse, st.n_l3, st.newq_head, st.fq_n, st.ba_countdown, st.n_search = len(iter_list), n_coarse, n_l3, newq_head, len(fq), -1, 99
    s = [np.zeros(0, np.uint8)] * rr.N_SECTIONS
    s[rr.STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    s[rr.POINT_POS] = tagged(n, 24, 10)
    rest = tagged(n, rr.REST_BYTES, 20).reshape(n, rr.REST_BYTES)
    for i, (src, bad, nmk) in enumerate(pts):
        for off, v in ((rr.REST_SRC_KF, src), (rr.REST_BAD, bad), (rr.REST_N_MEAS_KFS, nmk)):
            rest[i, off:off + 4] = np.frombuffer(np.int32(v).tobytes(), np.uint8)
    s[rr.POINT_REST] = rest.reshape(-1)
    s[rr.TRACKDATA], s[rr.TMPL] = tagged(n, rr.TRACKDATA_BYTES, 30), tagged(n, rr.TMPL_BYTES, 40)
    s[rr.PT_FLAGS], s[rr.PT_LEVEL], s[rr.CUR_MEAS] = tagged(n, 4, 50), tagged(n, 4, 60), tagged(n, rr.MEAS_BYTES, 70)
    meas = np.zeros((nk, n, rr.MEAS_BYTES), np.uint8)
    for k in range(nk):
        for i in range(n):
            meas[k, i, :] = (100 + 10 * k + i) % 256
            meas[k, i, rr.MEAS_VALID] = 1 if valid[k][i] else 0
    s[rr.KF_MEAS] = meas.reshape(-1)
    s[rr.KF_POSE], s[rr.KF_DEPTH] = tagged(nk, rr.POSE_BYTES, 80), tagged(nk, 16, 90)
    s[rr.KF_FIXED] = np.array(fixed if fixed is not None else [1] + [0] * (nk - 1), np.int32).view(np.uint8)
    for l in range(4):
        s[rr.KF_IMG0 + l] = tagged(nk, (W >> l) * (H >> l), 150 + 10 * l)
    s[rr.ITER_LIST] = np.array(iter_list, np.int32).view(np.uint8)
    if parts & rr.PART_IDLE:
        nr = np.zeros((n, 2), np.uint64) if never_retry is None else np.array(never_retry, np.uint64).reshape(n, 2)
        s[rr.NEVER_RETRY] = nr.reshape(-1).view(np.uint8)
        s[rr.FAIL_QUEUE] = np.array(sorted(fq), np.int32).reshape(-1, 2).view(np.uint8).reshape(-1)
    if parts & rr.PART_RELOC:
        N = ((W >> 3) // 2) * ((H >> 3) // 2)
        ri = rr.RelocInfo()
        ri.attempts, ri.successes, ri.best, ri.frame, ri.score = 3, 1, best, 5, 0.25
        s[rr.RELOC_INFO] = np.frombuffer(bytes(ri), np.uint8).copy()
        s[rr.RELOC_CUR_TMPL] = tagged(1, N * 4, 200)
        s[rr.RELOC_SCORES] = tagged(nk, 8, 210)
    return rr.assemble(h, s)


# 3 keyframes, 5 points: point 2 is bad, points 1 and 3 are sourced in keyframe 1; two failure-queue entries
PTS = [(0, 0, 3), (1, 0, 2), (0, 1, 0), (1, 0, 3), (2, 0, 2)]
VALID = [[1, 1, 0, 1, 0], [1, 1, 0, 1, 0], [1, 0, 0, 1, 1]]
NEVER = [[0b111, 0], [0, 0], [0, 0], [0b010, 0], [0b100, 1]]


def base_blob(**kw):
    args = dict(fq=[(1, 0), (2, 4)], iter_list=[4, 1, 0, 2, 3], n_coarse=2, n_l3=1, newq_head=4, never_retry=NEVER, fixed=[0, 1, 0], best=2)
    args.update(kw)
    return build(3, PTS, VALID, **args)


def elem(sec, eb, h):
    return sec.reshape(-1, eb)[:, 0].tolist()


def test_retire_the_middle_keyframe_field_by_field():
    blob = base_blob()
    out, counts = rr.retire(blob, 1)
    assert counts == {"points_sourced": 2, "points_bad": 1, "queue_dropped": 1}
    i = capi.snapshot_info(out)                                      # pure host code: the result is a well-formed snapshot
    assert (i.n_keyframes, i.n_points, i.frame, i.map_good, i.total_bytes) == (2, 2, 7, 1, len(out))
    h, s = rr.sections(out)
    assert (h.n_kf, h.n_points, h.n_iter, h.fq_n) == (2, 2, 2, 1)
    # the survivors are points 0 and 4, in that order, moved whole
    for sec, eb, tag in ((rr.POINT_POS, 24, 10), (rr.TRACKDATA, 168, 30), (rr.TMPL, 128, 40), (rr.PT_FLAGS, 4, 50), (rr.PT_LEVEL, 4, 60), (rr.CUR_MEAS, 24, 70)):
        assert s[sec].tolist() == [tag] * eb + [tag + 4] * eb, sec
    rest = s[rr.POINT_REST].reshape(2, 80)
    got = [[int(rest[j, o:o + 4].copy().view(np.int32)[0]) for o in (rr.REST_SRC_KF, rr.REST_BAD, rr.REST_N_MEAS_KFS)] for j in range(2)]
    assert got == [[0, 0, 2], [1, 0, 2]]                             # point 0 lost keyframe 1's measurement; point 4's source 2 became 1
    other = np.ones(80, bool)
    other[[o + b for o in (rr.REST_SRC_KF, rr.REST_BAD, rr.REST_N_MEAS_KFS) for b in range(4)]] = False
    assert set(rest[0][other]) == {20} and set(rest[1][other]) == {24}
    # measurement rows 0 and 2, columns 0 and 4
    m = s[rr.KF_MEAS].reshape(2, 2, 24)
    assert [[int(m[k, j, 0]) for j in range(2)] for k in range(2)] == [[100, 104], [120, 124]]
    assert [[int(m[k, j, rr.MEAS_VALID]) for j in range(2)] for k in range(2)] == [[1, 0], [1, 1]]
    # keyframes 0 and 2
    assert elem(s[rr.KF_POSE], 96, h) == [80, 82] and elem(s[rr.KF_DEPTH], 16, h) == [90, 92] and elem(s[rr.RELOC_SCORES], 8, h) == [210, 212]
    for l in range(4):
        n = (W >> l) * (H >> l)
        assert s[rr.KF_IMG0 + l].tolist() == [150 + 10 * l] * n + [152 + 10 * l] * n
    assert s[rr.KF_FIXED].view(np.int32).tolist() == [1, 0]          # the only fixed keyframe left: survivor 0 holds the gauge
    assert s[rr.NEVER_RETRY].view(np.uint64).reshape(2, 2).tolist() == [[0b11, 0], [0b10 | (1 << 63), 0]]
    assert s[rr.FAIL_QUEUE].view(np.int32).tolist() == [1, 1]        # (2, 4) renumbered; (1, 0) went with its keyframe
    assert s[rr.ITER_LIST].view(np.int32).tolist() == [1, 0]
    st = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes())
    assert (st.n_kf, st.n_points, st.newq_head, st.fq_n, st.n_iter, st.n_coarse, st.n_l3) == (2, 2, 1, 1, 2, 1, 1)
    # every other byte of the state stays
    before = rr.TrackerState.from_buffer_copy(rr.sections(blob)[1][rr.STATE].tobytes())
    for f in ("n_kf", "n_points", "newq_head", "fq_n", "n_iter", "n_coarse", "n_l3"):
        setattr(before, f, getattr(st, f))
    assert bytes(before) == bytes(st)
    assert rr.RelocInfo.from_buffer_copy(s[rr.RELOC_INFO].tobytes()).best == 1
    hb, sb = rr.sections(blob)
    for sec in (rr.RELOC_CUR_TMPL, rr.SBI_SMALL, rr.SBI_TMPL, rr.SBI_JACS, rr.SBI_ROT):
        assert np.array_equal(s[sec], sb[sec])
    assert (h.width, h.height, h.patch_size, h.quirks, h.frame, h.map_good, h.parts) == (hb.width, hb.height, hb.patch_size, hb.quirks, hb.frame, hb.map_good, hb.parts)


def test_retire_the_last_and_the_first_keyframe():
    blob = base_blob()
    out, counts = rr.retire(blob, 2)                                 # the last: point 4 is sourced there, point 2 is bad
    assert counts == {"points_sourced": 1, "points_bad": 1, "queue_dropped": 1}
    assert capi.snapshot_info(out).n_keyframes == 2
    h, s = rr.sections(out)
    assert s[rr.POINT_POS].reshape(-1, 24)[:, 0].tolist() == [10, 11, 13]
    assert s[rr.POINT_REST].reshape(-1, 80)[:, rr.REST_SRC_KF:rr.REST_SRC_KF + 4].copy().view(np.int32).reshape(-1).tolist() == [0, 1, 1]
    assert s[rr.POINT_REST].reshape(-1, 80)[:, rr.REST_N_MEAS_KFS:rr.REST_N_MEAS_KFS + 4].copy().view(np.int32).reshape(-1).tolist() == [2, 2, 2]
    assert elem(s[rr.KF_POSE], 96, h) == [80, 81] and s[rr.KF_FIXED].view(np.int32).tolist() == [0, 1]
    assert s[rr.FAIL_QUEUE].view(np.int32).tolist() == [1, 0] and s[rr.ITER_LIST].view(np.int32).tolist() == [1, 0, 2]
    assert s[rr.NEVER_RETRY].view(np.uint64).reshape(3, 2).tolist() == [[0b11, 0], [0, 0], [0b10, 0]]
    st = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes())
    assert (st.n_kf, st.n_points, st.newq_head, st.fq_n, st.n_iter, st.n_coarse, st.n_l3) == (2, 3, 3, 1, 3, 1, 1)
    assert rr.RelocInfo.from_buffer_copy(s[rr.RELOC_INFO].tobytes()).best == -1
    out, counts = rr.retire(blob, 0)                                 # the first: points 0 and 2 are sourced there (2 is bad as well)
    assert counts == {"points_sourced": 2, "points_bad": 0, "queue_dropped": 1}
    assert capi.snapshot_info(out).n_points == 3
    h, s = rr.sections(out)
    assert s[rr.POINT_POS].reshape(-1, 24)[:, 0].tolist() == [11, 13, 14]
    assert s[rr.POINT_REST].reshape(-1, 80)[:, rr.REST_SRC_KF:rr.REST_SRC_KF + 4].copy().view(np.int32).reshape(-1).tolist() == [0, 0, 1]
    assert s[rr.POINT_REST].reshape(-1, 80)[:, rr.REST_N_MEAS_KFS:rr.REST_N_MEAS_KFS + 4].copy().view(np.int32).reshape(-1).tolist() == [1, 2, 2]
    assert elem(s[rr.KF_POSE], 96, h) == [81, 82] and s[rr.KF_FIXED].view(np.int32).tolist() == [1, 0]
    assert s[rr.FAIL_QUEUE].view(np.int32).tolist() == [1, 2]        # (2, 4) -> (1, 2); (1, 0) went with point 0
    assert s[rr.ITER_LIST].view(np.int32).tolist() == [2, 0, 1]
    assert s[rr.NEVER_RETRY].view(np.uint64).reshape(3, 2).tolist() == [[0, 0], [0b01, 0], [0b10 | (1 << 63), 0]]
    st = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes())
    assert (st.n_kf, st.n_points, st.newq_head, st.fq_n, st.n_iter, st.n_coarse, st.n_l3) == (2, 3, 2, 1, 3, 2, 0)
    assert rr.RelocInfo.from_buffer_copy(s[rr.RELOC_INFO].tobytes()).best == 1


def test_a_fixed_survivor_keeps_the_gauge_and_a_blob_without_the_optional_parts():
    out = rr.retire_blob(base_blob(fixed=[1, 1, 0]), 1)
    assert rr.sections(out)[1][rr.KF_FIXED].view(np.int32).tolist() == [1, 0]
    out = rr.retire_blob(base_blob(fixed=[0, 0, 0]), 1)              # nothing was fixed: nothing becomes fixed
    assert rr.sections(out)[1][rr.KF_FIXED].view(np.int32).tolist() == [0, 0]
    out = rr.retire_blob(base_blob(fq=[], parts=0), 1)
    h, s = rr.sections(out)
    assert capi.snapshot_info(out).has_idle_state == 0 and len(s[rr.NEVER_RETRY]) == len(s[rr.FAIL_QUEUE]) == len(s[rr.RELOC_INFO]) == 0 and h.n_points == 2


def test_never_retry_bit_deletion_across_the_word_boundary():
    top = (1 << 64) - 1
    assert rr.delete_bit(1 << 63, 0b1, 63) == (1 << 63, 0)           # bit 63 leaves, bit 64 takes its place
    assert rr.delete_bit(1 << 63, 0b1, 64) == (1 << 63, 0)           # bit 64 leaves, bit 63 stays
    assert rr.delete_bit(top, 0b10, 63) == ((top >> 1), 0b1)         # 65 -> 64, and bit 63 is what was bit 64: clear
    assert rr.delete_bit(1 << 62, 0b110, 64) == (1 << 62, 0b11)
    assert rr.delete_bit(0b101, 1 << 63, 0) == (0b10, 1 << 62)
    assert rr.delete_bit(0, 1 << 63, 127) == (0, 0)
    # through a blob: 66 keyframes, one point, its set = {62, 63, 64, 65}
    nk = 66
    for r, want in ((63, [(1 << 62) | (1 << 63), 0b1]), (64, [(1 << 62) | (1 << 63), 0b1]), (62, [(1 << 62) | (1 << 63), 0b1]), (0, [(1 << 61) | (1 << 62) | (1 << 63), 0b1])):
        blob = build(nk, [(1, 0, 2)], [[1]] * nk, never_retry=[[(1 << 62) | (1 << 63), 0b11]], parts=rr.PART_IDLE)
        out = rr.retire_blob(blob, r)
        assert rr.sections(out)[1][rr.NEVER_RETRY].view(np.uint64).tolist() == want, r
        assert capi.snapshot_info(out).n_keyframes == nk - 1
