"""An independent numpy model of the map merge (csrc/merge.hip): merge(blob_d, blob_s) appends the map in the snapshot of a source
stream to the map in the snapshot of a destination stream, section by section (csrc/snapshot_format.h), and rebuilds the header and
the section table.  The snapshot inventories a stream's whole state, so "snapshot of d after the device merged" == merge(snapshot of d
before, snapshot of s before) says the device did exactly this and nothing else.  Built on the blob tools of tests/retire_ref.py; it
restates the rules and does not read csrc/merge_dev.h.

Destination d (nk_d keyframes, np_d points), source s (nk_s, np_s):
  per point      pos, the rest of MapPointDev, TrackData and templates of s follow d's; a source point's src_kf grows by nk_d
                 pt_flags of s & (TMPL_BAD | HAVE_LAST) = & 48; pt_level -1; cur_meas zero
                 never_retry: s's 128-bit set & (2^nk_s - 1), shifted up by nk_d (mod 2^128)
  per keyframe   kf_pose, kf_depth, the four pyramid levels of s follow d's; kf_fixed 0; the relocaliser's scores 0
  kf_meas        [[d, 0], [0, s]]: the cross blocks are zero
  failure queue  d's entries, then s's as (k + nk_d, p + np_d); the blob holds the queue sorted by (keyframe, point), and every
                 renumbered entry sorts behind every entry of d, so the concatenation is sorted if both parts were
  TrackerState   n_kf, n_points the sums; fq_n = stored_d + stored_s (the stored entries of each: the blob's count); ba_converged_recent =
                 ba_converged_full = 0; every other byte d's (newq_head among them)
  everything else (iter_list, the last frame's SmallBlurryImage, RelocInfo, the last attempt's frame template)   d's
"""
import numpy as np

import retire_ref as rr

KEEP_FLAGS = 16 | 32
MASK128 = (1 << 128) - 1
FQ_CAP = 8192                    # capacity of a stream's failure queue (csrc/track.hip, trk_fill_params)


def shift_set(w0, w1, nk_s, nk_d):
    """the never-retry set (w0 low, w1 high) of a source point as the destination holds it -> (low, high)"""
    v = ((int(w1) << 64) | int(w0)) & ((1 << nk_s) - 1)
    v = (v << nk_d) & MASK128
    return v & ((1 << 64) - 1), v >> 64


def queue_entry(k, p, nk_d, np_d):
    return k + nk_d, p + np_d


def merge(blob_d, blob_s, fq_cap=FQ_CAP):
    """-> (the destination's blob after the source has been appended, {"keyframes", "points", "queue"})"""
    hd, d = rr.sections(blob_d)
    hs, s = rr.sections(blob_s)
    assert (hd.width, hd.height, hd.patch_size, hd.quirks) == (hs.width, hs.height, hs.patch_size, hs.quirks) and bytes(hd.cam) == bytes(hs.cam)
    for part in (rr.PART_IDLE, rr.PART_RELOC):                       # what d keeps per point or per keyframe, s must bring
        assert (hd.parts & part) == (hs.parts & part), (hd.parts, hs.parts)
    nk_d, np_d, nk_s, np_s = hd.n_kf, hd.n_points, hs.n_kf, hs.n_points
    st = rr.TrackerState.from_buffer_copy(d[rr.STATE].tobytes())
    assert (st.n_kf, st.n_points) == (nk_d, np_d) and nk_d + nk_s <= 128
    rest = s[rr.POINT_REST].reshape(np_s, rr.REST_BYTES).copy()
    src = rest[:, rr.REST_SRC_KF:rr.REST_SRC_KF + 4].copy().view(np.int32).reshape(-1)
    rest[:, rr.REST_SRC_KF:rr.REST_SRC_KF + 4] = (src + nk_d).astype(np.int32).view(np.uint8).reshape(np_s, 4)
    out = list(d)
    out[rr.POINT_REST] = np.concatenate([d[rr.POINT_REST], rest.reshape(-1)])
    for sec in (rr.POINT_POS, rr.TRACKDATA, rr.TMPL, rr.KF_POSE, rr.KF_DEPTH, rr.KF_IMG0, rr.KF_IMG1, rr.KF_IMG2, rr.KF_IMG3):
        out[sec] = np.concatenate([d[sec], s[sec]])
    out[rr.PT_FLAGS] = np.concatenate([d[rr.PT_FLAGS], (s[rr.PT_FLAGS].view(np.int32) & KEEP_FLAGS).astype(np.int32).view(np.uint8)])
    out[rr.PT_LEVEL] = np.concatenate([d[rr.PT_LEVEL], np.full(np_s, -1, np.int32).view(np.uint8)])
    out[rr.CUR_MEAS] = np.concatenate([d[rr.CUR_MEAS], np.zeros(np_s * rr.MEAS_BYTES, np.uint8)])
    out[rr.KF_FIXED] = np.concatenate([d[rr.KF_FIXED], np.zeros(nk_s * 4, np.uint8)])
    meas = np.zeros((nk_d + nk_s, np_d + np_s, rr.MEAS_BYTES), np.uint8)
    meas[:nk_d, :np_d] = d[rr.KF_MEAS].reshape(nk_d, np_d, rr.MEAS_BYTES)
    meas[nk_d:, np_d:] = s[rr.KF_MEAS].reshape(nk_s, np_s, rr.MEAS_BYTES)
    out[rr.KF_MEAS] = meas.reshape(-1)
    counts = {"keyframes": nk_s, "points": np_s, "queue": 0}
    if hd.parts & rr.PART_IDLE:
        nr = s[rr.NEVER_RETRY].view(np.uint64).reshape(np_s, 2).copy()
        for i in range(np_s):
            nr[i] = shift_set(nr[i, 0], nr[i, 1], nk_s, nk_d)
        out[rr.NEVER_RETRY] = np.concatenate([d[rr.NEVER_RETRY], nr.reshape(-1).view(np.uint8)])
        fd = [tuple(int(x) for x in e) for e in d[rr.FAIL_QUEUE].view(np.int32).reshape(-1, 2)]
        fs = [queue_entry(int(k), int(p), nk_d, np_d) for k, p in s[rr.FAIL_QUEUE].view(np.int32).reshape(-1, 2)]
        fs = fs[:max(0, fq_cap - len(fd))]                           # positions stored_d + j below the capacity
        counts["queue"] = len(fs)
        st.fq_n = hd.fq_n + hs.fq_n                                  # it counts past the capacity
        hd.fq_n = len(fd) + len(fs)
        out[rr.FAIL_QUEUE] = np.array(sorted(fd + fs), np.int32).reshape(-1, 2).view(np.uint8).reshape(-1)
    if hd.parts & rr.PART_RELOC:
        out[rr.RELOC_SCORES] = np.concatenate([d[rr.RELOC_SCORES], np.zeros(nk_s * 8, np.uint8)])
    st.n_kf, st.n_points = nk_d + nk_s, np_d + np_s
    st.ba_converged_recent = st.ba_converged_full = 0
    out[rr.STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    hd.n_kf, hd.n_points = nk_d + nk_s, np_d + np_s
    return rr.assemble(hd, out), counts


def merge_blob(blob_d, blob_s):
    return merge(blob_d, blob_s)[0]
