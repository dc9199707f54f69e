"""An independent numpy model of keyframe retirement (csrc/retire.hip): retire_blob(blob, r) applies the semantics to a stream snapshot
(csrc/snapshot_format.h), section by section, and rebuilds the header and the section table.  The snapshot inventories a stream's whole
state, so "snapshot after the device retired r" == retire_blob(snapshot before, r) says the device did exactly this and nothing else.

Retired keyframe r of nk, np points.  A point is dropped when bad || src_kf == r; remap[i] is the new index of a survivor.
  per keyframe   row r of kf_pose, kf_fixed, kf_depth, the four pyramid levels, kf_meas and the relocaliser's scores leaves, later rows move down
  per point      pos, the rest of MapPointDev, TrackData, templates, pt_flags, pt_level, cur_meas, never_retry and the columns of every
                 kf_meas row are compacted; a survivor's src_kf > r is decremented, its n_meas_kfs is decremented where row r measured it,
                 its never-retry set loses bit r and the bits above move down one across both words
  failure queue  entries of keyframe r or of a dropped point go, the rest are renumbered; fq_n = the number kept among the stored entries
  iter_list      dropped points go, order kept; n_coarse, n_l3, n_iter shrink by what left their segments
  TrackerState   n_kf, n_points, newq_head (= survivors below the old head), fq_n, n_iter, n_coarse, n_l3; every other byte stays
  RelocInfo      best: -1 if it was r, one less if it was above r
  fixedness      if r was fixed and no survivor is, survivor 0 becomes fixed
"""
import ctypes as C

import numpy as np

_P = C.c_double * 12


class TrackerState(C.Structure):
    """csrc/vslam_internal.h TrackerState"""
    _fields_ = [("pose_final", _P), ("start_pose", _P), ("pose_cur", _P), ("velocity", C.c_double * 6),
                ("msd_vel", C.c_double), ("depth_mean", C.c_double), ("depth_sigma", C.c_double), ("wiggle_depth_norm", C.c_double),
                ("frame", C.c_int), ("last_kf_dropped", C.c_int), ("lost_frames", C.c_int), ("quality", C.c_int),
                ("attempted", C.c_int * 4), ("found", C.c_int * 4),
                ("did_coarse", C.c_int), ("just_recovered", C.c_int), ("map_good", C.c_int), ("kf_pending", C.c_int),
                ("n_points", C.c_int), ("n_kf", C.c_int), ("pvs_count", C.c_int * 4), ("pvs_head", C.c_int * 4),
                ("n_coarse", C.c_int), ("n_search", C.c_int), ("n_iter", C.c_int), ("n_l3", C.c_int),
                ("coarse_range", C.c_int), ("fine_range", C.c_int), ("coarse_found", C.c_int),
                ("ba_accepted", C.c_int), ("kf_added", C.c_int), ("ba_converged_recent", C.c_int), ("ba_converged_full", C.c_int),
                ("ba_countdown", C.c_int), ("n_zmssd", C.c_ulonglong), ("n_ba_trials", C.c_ulonglong),
                ("newq_head", C.c_int), ("fq_n", C.c_int), ("idle_count", C.c_int), ("idle_do_fail", C.c_int),
                ("n_refound_new", C.c_int), ("n_refound_failed", C.c_int), ("n_ba_all", C.c_int), ("n_ba_recent_idle", C.c_int),
                ("init_stage", C.c_int), ("spacebar", C.c_int), ("n_trails", C.c_int), ("trail_buf", C.c_int),
                ("boot_action", C.c_int), ("boot_run", C.c_int), ("boot_ok", C.c_int), ("n_hom_inliers", C.c_int), ("n_init_points", C.c_int),
                ("boot_seed", C.c_uint), ("boot_host_matches", C.c_int), ("recovered_now", C.c_int), ("pvs_seed", C.c_uint)]


class MapPointDev(C.Structure):
    """csrc/vslam_internal.h MapPointDev; the blob carries pos (24 bytes) and the rest (80) as two sections"""
    _fields_ = [("pos", C.c_double * 3), ("right", C.c_double * 3), ("down", C.c_double * 3),
                ("src_kf", C.c_int), ("src_level", C.c_int), ("irx", C.c_int), ("iry", C.c_int),
                ("bad", C.c_int), ("n_in", C.c_int), ("n_out", C.c_int), ("n_meas_kfs", C.c_int)]


class RelocInfo(C.Structure):
    """csrc/vslam_internal.h RelocInfo"""
    _fields_ = [("attempts", C.c_int), ("successes", C.c_int), ("best", C.c_int), ("frame", C.c_int),
                ("best_zmssd", C.c_double), ("score", C.c_double), ("ln_adj", C.c_double * 6), ("best_pose", _P)]


assert C.sizeof(TrackerState) == 624 and C.sizeof(MapPointDev) == 104 and C.sizeof(RelocInfo) == 176

# ---- csrc/snapshot_format.h ------------------------------------------------------------------------------------------------------
(STATE, POINT_POS, POINT_REST, TRACKDATA, TMPL, PT_FLAGS, PT_LEVEL, CUR_MEAS, KF_MEAS, KF_POSE, KF_FIXED, KF_DEPTH, KF_IMG0, KF_IMG1, KF_IMG2, KF_IMG3,
 ITER_LIST, NEVER_RETRY, FAIL_QUEUE, SBI_SMALL, SBI_TMPL, SBI_JACS, SBI_ROT, RELOC_INFO, RELOC_CUR_TMPL, RELOC_SCORES, N_SECTIONS) = range(27)
PART_IDLE, PART_SBI, PART_RELOC = 1, 2, 4
REST_BYTES, TRACKDATA_BYTES, TMPL_BYTES, MEAS_BYTES, POSE_BYTES = 80, 168, 128, 24, 96
MEAS_VALID = 16                  # byte of MeasDev::valid behind root[2]
REST_SRC_KF, REST_BAD, REST_N_MEAS_KFS = 48, 64, 76          # byte offsets inside the rest of MapPointDev


class Header(C.Structure):
    _fields_ = [("magic", C.c_char * 8), ("version", C.c_uint), ("header_bytes", C.c_uint), ("total_bytes", C.c_ulonglong),
                ("width", C.c_int), ("height", C.c_int), ("patch_size", C.c_int), ("quirks", C.c_int), ("cam", C.c_double * 5),
                ("n_kf", C.c_int), ("n_points", C.c_int), ("frame", C.c_int), ("map_good", C.c_int), ("n_iter", C.c_int), ("fq_n", C.c_int),
                ("parts", C.c_uint), ("reserved", C.c_uint), ("sec", C.c_ulonglong * (2 * N_SECTIONS))]


assert C.sizeof(Header) == 112 + 16 * N_SECTIONS and MapPointDev.src_kf.offset - 24 == REST_SRC_KF and MapPointDev.bad.offset - 24 == REST_BAD \
    and MapPointDev.n_meas_kfs.offset - 24 == REST_N_MEAS_KFS


def section_rows(h, sec):
    """(rows, row_bytes) of a section for the header's counts: snap_section_rows"""
    n, k, N = h.n_points, h.n_kf, ((h.width >> 3) // 2) * ((h.height >> 3) // 2)
    idle, sbi, reloc = h.parts & PART_IDLE, h.parts & PART_SBI, h.parts & PART_RELOC
    r = {STATE: (1, 624), POINT_POS: (n, 24), POINT_REST: (n, REST_BYTES), TRACKDATA: (n, TRACKDATA_BYTES), TMPL: (n, TMPL_BYTES), PT_FLAGS: (n, 4),
         PT_LEVEL: (n, 4), CUR_MEAS: (n, MEAS_BYTES), KF_MEAS: (k, n * MEAS_BYTES), KF_POSE: (k, POSE_BYTES), KF_FIXED: (k, 4), KF_DEPTH: (k, 16),
         ITER_LIST: (h.n_iter, 4), NEVER_RETRY: (n, 16) if idle else (0, 0), FAIL_QUEUE: (h.fq_n, 8) if idle else (0, 0),
         SBI_SMALL: (1, N) if sbi else (0, 0), SBI_TMPL: (1, N * 4) if sbi else (0, 0), SBI_JACS: (1, N * 8) if sbi else (0, 0),
         SBI_ROT: (1, 64) if sbi else (0, 0), RELOC_INFO: (1, 176) if reloc else (0, 0), RELOC_CUR_TMPL: (1, N * 4) if reloc else (0, 0),
         RELOC_SCORES: (k, 8) if reloc else (0, 0)}
    for l in range(4):
        r[KF_IMG0 + l] = (k * (h.height >> l), h.width >> l)
    rows, rb = r[sec]
    return (rows, rb) if rows and rb else (0, 0)


def sections(blob):
    """-> (Header, [uint8 array of each section])"""
    blob = np.frombuffer(bytes(blob), np.uint8)
    h = Header.from_buffer_copy(blob[:C.sizeof(Header)].tobytes())
    assert h.magic == b"VSLMSNAP" and h.total_bytes == len(blob)
    out = []
    for i in range(N_SECTIONS):
        off, nb = h.sec[2 * i], h.sec[2 * i + 1]
        rows, rb = section_rows(h, i)
        assert nb == rows * rb, (i, nb, rows, rb)
        out.append(blob[off:off + nb].copy())
    return h, out


def assemble(h, secs):
    """the blob of these sections: the table of snap_table (every section at a multiple of 16, zeros between), the header around it"""
    off = C.sizeof(Header)
    for i in range(N_SECTIONS):
        rows, rb = section_rows(h, i)
        assert len(secs[i]) == rows * rb, (i, len(secs[i]), rows, rb)
        h.sec[2 * i], h.sec[2 * i + 1] = off, rows * rb
        off = (off + rows * rb + 15) & ~15
    h.total_bytes = off
    out = np.zeros(off, np.uint8)
    out[:C.sizeof(Header)] = np.frombuffer(bytes(h), np.uint8)
    for i in range(N_SECTIONS):
        out[h.sec[2 * i]:h.sec[2 * i] + h.sec[2 * i + 1]] = secs[i]
    return out


def delete_bit(w0, w1, r):
    """bit r of the 128-bit set (w0 low, w1 high) leaves, the bits above it move down one"""
    v = (int(w1) << 64) | int(w0)
    low = v & ((1 << r) - 1)
    v = low | ((v >> (r + 1)) << r)
    return v & ((1 << 64) - 1), v >> 64


def retire(blob, r):
    """-> (the blob after keyframe r has been retired, {"points_sourced", "points_bad", "queue_dropped"})"""
    h, s = sections(blob)
    nk, n = h.n_kf, h.n_points
    assert 0 <= r < nk and nk >= 3
    st = TrackerState.from_buffer_copy(s[STATE].tobytes())
    assert (st.n_kf, st.n_points) == (nk, n)
    rest = s[POINT_REST].reshape(n, REST_BYTES)

    def ints(a, off):
        return a[:, off:off + 4].copy().view(np.int32).reshape(-1)

    src, bad = ints(rest, REST_SRC_KF), ints(rest, REST_BAD)
    drop = (bad != 0) | (src == r)
    keep = ~drop
    remap = np.where(keep, np.cumsum(keep) - 1, -1)
    n_new = int(keep.sum())
    counts = {"points_sourced": int((src == r).sum()), "points_bad": int(((bad != 0) & (src != r)).sum())}
    meas = s[KF_MEAS].reshape(nk, n, MEAS_BYTES)
    valid_r = meas[r, :, MEAS_VALID].view(np.int8) != 0
    # survivors: the two fields that follow the retirement
    nmk = ints(rest, REST_N_MEAS_KFS)
    src2 = np.where(src > r, src - 1, src).astype(np.int32)
    nmk2 = (nmk - valid_r.astype(np.int32)).astype(np.int32)
    rest = rest.copy()
    rest[:, REST_SRC_KF:REST_SRC_KF + 4] = src2.view(np.uint8).reshape(n, 4)
    rest[:, REST_N_MEAS_KFS:REST_N_MEAS_KFS + 4] = nmk2.view(np.uint8).reshape(n, 4)
    s[POINT_REST] = rest[keep].reshape(-1)
    for sec, eb in ((POINT_POS, 24), (TRACKDATA, TRACKDATA_BYTES), (TMPL, TMPL_BYTES), (PT_FLAGS, 4), (PT_LEVEL, 4), (CUR_MEAS, MEAS_BYTES)):
        s[sec] = s[sec].reshape(n, eb)[keep].reshape(-1)
    rows = [k for k in range(nk) if k != r]
    s[KF_MEAS] = meas[rows][:, keep].reshape(-1)
    for sec, eb in ((KF_POSE, POSE_BYTES), (KF_DEPTH, 16)) + ((RELOC_SCORES, 8),) * bool(h.parts & PART_RELOC):
        s[sec] = s[sec].reshape(nk, eb)[rows].reshape(-1)
    for l in range(4):
        s[KF_IMG0 + l] = s[KF_IMG0 + l].reshape(nk, -1)[rows].reshape(-1)
    fixed = s[KF_FIXED].view(np.int32).copy()
    was_fixed = fixed[r] != 0
    fixed = fixed[rows]
    if was_fixed and not fixed.any():
        fixed[0] = 1
    s[KF_FIXED] = fixed.view(np.uint8)
    counts["queue_dropped"] = 0
    if h.parts & PART_IDLE:
        nr = s[NEVER_RETRY].view(np.uint64).reshape(n, 2)[keep].copy()
        for i in range(len(nr)):
            nr[i] = delete_bit(nr[i, 0], nr[i, 1], r)
        s[NEVER_RETRY] = nr.reshape(-1).view(np.uint8)
        fq = s[FAIL_QUEUE].view(np.int32).reshape(-1, 2)
        kept = sorted((int(k) - (k > r), int(remap[p])) for k, p in fq if k != r and 0 <= p < n and remap[p] >= 0)
        counts["queue_dropped"] = len(fq) - len(kept)
        s[FAIL_QUEUE] = np.array(kept, np.int32).reshape(-1, 2).view(np.uint8).reshape(-1)
        st.fq_n = len(kept)
        h.fq_n = len(kept)
    # the last frame's iteration set: [0, n_coarse) coarse, then n_l3 of level 3, then the rest
    it = s[ITER_LIST].view(np.int32)
    n_it = len(it)
    seg_c = min(max(st.n_coarse, 0), n_it)
    seg_l = seg_c + min(max(st.n_l3, 0), n_it - seg_c)
    ok = np.array([0 <= p < n and remap[p] >= 0 for p in it], bool)
    s[ITER_LIST] = remap[it[ok]].astype(np.int32).view(np.uint8)
    st.n_coarse -= int((~ok[:seg_c]).sum())
    st.n_l3 -= int((~ok[seg_c:seg_l]).sum())
    st.n_iter -= int((~ok).sum())
    st.newq_head = int(keep[:max(st.newq_head, 0)].sum())
    st.n_kf, st.n_points = nk - 1, n_new
    s[STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    if h.parts & PART_RELOC:
        ri = RelocInfo.from_buffer_copy(s[RELOC_INFO].tobytes())
        ri.best = -1 if ri.best == r else ri.best - (ri.best > r)
        s[RELOC_INFO] = np.frombuffer(bytes(ri), np.uint8).copy()
    h.n_kf, h.n_points, h.n_iter = nk - 1, n_new, max(st.n_iter, 0)
    return assemble(h, s), counts


def retire_blob(blob, r):
    return retire(blob, r)[0]
