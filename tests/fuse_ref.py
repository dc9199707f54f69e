"""An independent numpy model of point fusion (csrc/fuse.hip): fuse_core works on plain arrays, fuse_blob applies it to a stream snapshot
(csrc/snapshot_format.h) with the blob tools of tests/retire_ref.py.  The snapshot inventories a stream's whole state, so "snapshot
after the device fused" == fuse_blob(snapshot before) says the device did exactly this and nothing else.  The model restates the rule
and does not read csrc/fuse_dev.h.

One stream, nk keyframes, np points, radius in level pixels, min_views.  A point is live if not bad; cell (k, i) is valid if its valid
byte is non-zero.  For live q < p and keyframe k:
  shared(k)    both cells valid
  agree(k)     shared, equal level bytes, and d2 <= lim2 with dx = root_p[0] - root_q[0], dy = root_p[1] - root_q[1], d2 = dx*dx + dy*dy,
               lim = radius * float(1 << level), lim2 = lim*lim: float64, one rounding per operation, in that order.  The arithmetic
               below is numpy's elementwise float64 subtract, multiply and add -- the scalar operations, one per element, none fused;
               no dot, no hypot.  A NaN compares false.  A level byte outside 0..30 names no level: no agreement.
  conflict(k)  shared and not agree
  dup(p, q)    agreements >= min_views and no conflict;  partner(p) = the lowest live q < p with dup(p, q), else -1
  p is dropped into q = partner(p) iff q >= 0 and partner(q) < 0 (one level per call; all decisions on the state before the call)
A kept q, keyframe k: a valid cell stays; an empty cell with bit k of q's never-retry set stays empty; an empty cell otherwise takes
the cell (k, p) of the lowest p dropped into q whose cell is valid, source 2 (root) turned into 1 (re-find), and n_meas_kfs[q] grows by
one.  A dropped p: bad = 1 and the valid byte of each of its cells = 0; nothing else."""
import numpy as np

import retire_ref as rr

MEAS_LEVEL, MEAS_SOURCE = 17, 19
MAX_LEVEL = 30


def partners(valid, level, root, bad, radius, min_views):
    """valid [nk, np] bool, level [nk, np] int, root [nk, np, 2] float64, bad [np] -> partner [np] (-1: none)"""
    nk, n = valid.shape
    live = ~np.asarray(bad, bool)
    level = np.asarray(level, np.int64)
    ok = (level >= 0) & (level <= MAX_LEVEL)
    radius = np.float64(radius)
    lim = radius * np.left_shift(1, np.where(ok, level, 0)).astype(np.float64)
    lim2 = lim * lim
    partner = np.full(n, -1, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(1, n):
            if not live[p] or nk == 0:
                continue
            shared = valid[:, :p] & valid[:, p:p + 1]
            dx = root[:, p:p + 1, 0] - root[:, :p, 0]
            dy = root[:, p:p + 1, 1] - root[:, :p, 1]
            d2 = dx * dx + dy * dy
            agree = shared & (level[:, :p] == level[:, p:p + 1]) & ok[:, p:p + 1] & (d2 <= lim2[:, p:p + 1])
            conflict = shared & ~agree
            dup = (agree.sum(0) >= min_views) & (conflict.sum(0) == 0) & live[:p]
            hit = np.flatnonzero(dup)
            if len(hit):
                partner[p] = hit[0]
    return partner


def fuse_core(valid, level, root, bad, never_retry, n_meas_kfs, source, radius, min_views):
    """The arrays of one stream (never_retry: a Python int per point, the 128-bit set, or None without idle jobs) ->
    {"partner", "pairs" [(dropped, kept)] ascending by dropped, "taken" [(k, kept, dropped)], "valid", "bad", "n_meas_kfs", "source" (the
    arrays afterwards; level and root of a taken cell are the dropped point's), "info" {"dropped", "taken", "not_taken", "chained"}}"""
    valid = np.asarray(valid, bool)
    nk, n = valid.shape
    partner = partners(valid, np.asarray(level), np.asarray(root, np.float64).reshape(nk, n, 2), bad, radius, min_views)
    pairs = [(p, int(partner[p])) for p in range(n) if partner[p] >= 0 and partner[partner[p]] < 0]
    chained = sum(1 for p in range(n) if partner[p] >= 0 and partner[partner[p]] >= 0)
    out_valid, out_bad = valid.copy(), np.asarray(bad).astype(np.int32).copy()
    out_nmk, out_src = np.asarray(n_meas_kfs).astype(np.int32).copy(), np.asarray(source).copy()
    taken, not_taken = [], 0
    filled = set()
    for p, q in pairs:                                               # ascending p: the first to fill a cell is the lowest
        for k in range(nk):
            if not valid[k, p]:
                continue
            never = never_retry is not None and (int(never_retry[q]) >> k) & 1
            if valid[k, q] or never or (k, q) in filled:
                not_taken += 1
                continue
            filled.add((k, q))
            taken.append((k, q, p))
            out_valid[k, q] = True
            out_src[k, q] = 1 if source[k, p] == 2 else source[k, p]
            out_nmk[q] += 1
    for p, _ in pairs:
        out_bad[p] = 1
        out_valid[:, p] = False
    info = {"dropped": len(pairs), "taken": len(taken), "not_taken": not_taken, "chained": chained}
    return {"partner": partner, "pairs": pairs, "taken": taken, "valid": out_valid, "bad": out_bad, "n_meas_kfs": out_nmk, "source": out_src, "info": info}


def blob_arrays(blob):
    """-> (header, sections, the core's arrays of the blob as a dict)"""
    h, s = rr.sections(blob)
    nk, n = h.n_kf, h.n_points
    meas = s[rr.KF_MEAS].reshape(nk, n, rr.MEAS_BYTES)
    rest = s[rr.POINT_REST].reshape(n, rr.REST_BYTES)
    a = {"valid": meas[:, :, rr.MEAS_VALID] != 0, "level": meas[:, :, MEAS_LEVEL].view(np.int8).astype(np.int64),
         "root": np.ascontiguousarray(meas[:, :, :16]).view(np.float64).reshape(nk, n, 2), "source": meas[:, :, MEAS_SOURCE].view(np.int8).copy(),
         "bad": rest[:, rr.REST_BAD:rr.REST_BAD + 4].copy().view(np.int32).reshape(-1) != 0,
         "n_meas_kfs": rest[:, rr.REST_N_MEAS_KFS:rr.REST_N_MEAS_KFS + 4].copy().view(np.int32).reshape(-1), "never_retry": None}
    if h.parts & rr.PART_IDLE:
        nr = s[rr.NEVER_RETRY].view(np.uint64).reshape(n, 2)
        a["never_retry"] = [(int(nr[i, 1]) << 64) | int(nr[i, 0]) for i in range(n)]
    return h, s, a


def fuse(blob, radius, min_views):
    """-> (the blob after the fusion, info {"fused", "dropped", "taken", "not_taken", "chained", "frame"}, pairs int32 [n, 2])"""
    h, s, a = blob_arrays(blob)
    nk, n = h.n_kf, h.n_points
    st = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes())
    assert (st.n_kf, st.n_points) == (nk, n)
    r = fuse_core(a["valid"], a["level"], a["root"], a["bad"], a["never_retry"], a["n_meas_kfs"], a["source"], radius, min_views)
    meas = s[rr.KF_MEAS].reshape(nk, n, rr.MEAS_BYTES).copy()
    before = meas.copy()
    rest = s[rr.POINT_REST].reshape(n, rr.REST_BYTES).copy()
    for k, q, p in r["taken"]:
        meas[k, q] = before[k, p]                                    # the 24 bytes
        meas[k, q, MEAS_SOURCE] = np.int8(r["source"][k, q]).view(np.uint8)
    for p, _ in r["pairs"]:
        meas[:, p, rr.MEAS_VALID] = 0
        rest[p, rr.REST_BAD:rr.REST_BAD + 4] = np.array([1], np.int32).view(np.uint8)
    rest[:, rr.REST_N_MEAS_KFS:rr.REST_N_MEAS_KFS + 4] = r["n_meas_kfs"].astype(np.int32).view(np.uint8).reshape(n, 4)
    s[rr.KF_MEAS], s[rr.POINT_REST] = meas.reshape(-1), rest.reshape(-1)
    if r["pairs"]:
        st.ba_converged_recent = st.ba_converged_full = 0
        s[rr.STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    info = dict(r["info"], fused=1 if r["pairs"] else 0, frame=st.frame)
    return rr.assemble(h, s), info, np.array(r["pairs"], np.int32).reshape(-1, 2)


def fuse_blob(blob, radius, min_views):
    return fuse(blob, radius, min_views)
