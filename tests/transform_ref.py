"""An independent numpy model of the similarity transform of a stream's map (csrc/similarity_dev.h, csrc/transform.hip):
transform_blob(blob, T12, s) applies x' = R (s x) + t to a stream snapshot (csrc/snapshot_format.h), section by section.  The snapshot
inventories a stream's whole state, so "snapshot after the device transformed" == transform_blob(snapshot before) says the device did
exactly this and nothing else.  float64 throughout, the header's expression order restated (numpy fuses no multiply with an add), so the
bits are the header's.  It does not call the library.

  POINT_POS                        q = pos * s per component, then t + (R0 q0 + R1 q1 + R2 q2) per row
  POINT_REST right, down           q = v * s, then R0 q0 + R1 q1 + R2 q2 per row
  KF_POSE, STATE pose_final / start_pose / pose_cur, RELOC_INFO best_pose      C.t *= s, then pose_mul(C, pose_inverse(T))
  STATE velocity[0..2], depth_mean, depth_sigma; KF_DEPTH; TRACKDATA cam[0..2]  *= s
  every other byte                 stays
"""
import numpy as np

import retire_ref as rr

TD_CAM_BYTES = 24                # TrackData::cam leads the struct
REST_VEC_BYTES = 48              # right[3], down[3] lead the rest of MapPointDev


# ---- dev_math.h, on arrays whose last axis holds the pose12 / the 3-vector --------------------------------------------------------
def rot(T, p):
    """pose_rot: R p, row by row, summed left to right"""
    return np.stack([T[..., 3 * i] * p[..., 0] + T[..., 3 * i + 1] * p[..., 1] + T[..., 3 * i + 2] * p[..., 2] for i in range(3)], -1)


def xform(T, p):
    """pose_xform: t + R p"""
    return T[..., 9:12] + rot(T, p)


def mul(a, b):
    """pose_mul(a, b)"""
    R = [a[..., 3 * i] * b[..., j] + a[..., 3 * i + 1] * b[..., 3 + j] + a[..., 3 * i + 2] * b[..., 6 + j] for i in range(3) for j in range(3)]
    t = a[..., 9:12] + rot(a, b[..., 9:12])
    return np.concatenate([np.stack(R, -1), t], -1)


def inverse(a):
    """pose_inverse(a)"""
    Rt = np.stack([a[..., 3 * j + i] for i in range(3) for j in range(3)], -1)
    r = np.concatenate([Rt, np.zeros_like(a[..., 9:12])], -1)
    return np.concatenate([Rt, -rot(r, a[..., 9:12])], -1)


# ---- similarity_dev.h ----------------------------------------------------------------------------------------------------------
def sim_point(T, s, p):
    return xform(T, p * s)


def sim_vector(T, s, v):
    return rot(T, v * s)


def sim_pose(T, s, C):
    c = np.array(C, np.float64, copy=True)
    c[..., 9:12] = c[..., 9:12] * s
    return mul(c, inverse(np.asarray(T, np.float64)))


def compose(T, s, accT, accs):
    """the accumulated similarity after (T, s) has been applied behind (accT, accs): sim_compose -> (pose12, scale)"""
    a = np.array(accT, np.float64, copy=True)
    a[9:12] = a[9:12] * s
    return mul(np.asarray(T, np.float64), a), s * accs


def invert(T, s):
    """the similarity that undoes (T, s): x = R^T ((x' - t) / s) -> (pose12, 1 / s)"""
    T = np.asarray(T, np.float64)
    R = T[:9].reshape(3, 3)
    return np.concatenate([R.T.reshape(-1), -(R.T @ T[9:]) / s]), 1.0 / s


# ---- the blob ------------------------------------------------------------------------------------------------------------------
def _f64(a):
    return np.ascontiguousarray(a).view(np.float64)


def transform_blob(blob, T12, s=1.0):
    """-> the blob after the stream's map has been moved by x' = R (s x) + t"""
    T, s = np.asarray(T12, np.float64).reshape(12), np.float64(s)
    h, sec = rr.sections(blob)
    n, nk = h.n_points, h.n_kf
    if n:
        sec[rr.POINT_POS] = sim_point(T, s, _f64(sec[rr.POINT_POS]).reshape(n, 3)).reshape(-1).view(np.uint8)
        rest = sec[rr.POINT_REST].reshape(n, rr.REST_BYTES).copy()
        v = _f64(rest[:, :REST_VEC_BYTES]).reshape(n, 2, 3)
        rest[:, :REST_VEC_BYTES] = np.ascontiguousarray(sim_vector(T, s, v)).view(np.uint8).reshape(n, REST_VEC_BYTES)
        sec[rr.POINT_REST] = rest.reshape(-1)
        td = sec[rr.TRACKDATA].reshape(n, rr.TRACKDATA_BYTES).copy()
        cam = _f64(td[:, :TD_CAM_BYTES]).reshape(n, 3)
        td[:, :TD_CAM_BYTES] = np.ascontiguousarray(cam * s).view(np.uint8).reshape(n, TD_CAM_BYTES)
        sec[rr.TRACKDATA] = td.reshape(-1)
    if nk:
        sec[rr.KF_POSE] = sim_pose(T, s, _f64(sec[rr.KF_POSE]).reshape(nk, 12)).reshape(-1).view(np.uint8)
        sec[rr.KF_DEPTH] = (_f64(sec[rr.KF_DEPTH]) * s).view(np.uint8)
    st = rr.TrackerState.from_buffer_copy(sec[rr.STATE].tobytes())
    for name in ("pose_final", "start_pose", "pose_cur"):
        getattr(st, name)[:] = sim_pose(T, s, np.array(getattr(st, name)[:])).tolist()
    for k in range(3):
        st.velocity[k] = float(np.float64(st.velocity[k]) * s)
    st.depth_mean = float(np.float64(st.depth_mean) * s)
    st.depth_sigma = float(np.float64(st.depth_sigma) * s)
    sec[rr.STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    if h.parts & rr.PART_RELOC:
        ri = rr.RelocInfo.from_buffer_copy(sec[rr.RELOC_INFO].tobytes())
        ri.best_pose[:] = sim_pose(T, s, np.array(ri.best_pose[:])).tolist()
        sec[rr.RELOC_INFO] = np.frombuffer(bytes(ri), np.uint8).copy()
    return rr.assemble(h, sec)


# ---- helpers the tests share ---------------------------------------------------------------------------------------------------
def rotation(axis, angle):
    """Rodrigues' formula -> 3 x 3"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)])
