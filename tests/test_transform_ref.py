"""CPU test: the numpy model of the map's similarity transform (tests/transform_ref.py) on a snapshot blob built by hand: the
transform and its inverse, a composition against one transform, the composition formula of vslam_get_transform_info, and every byte the
rule does not name."""
import numpy as np

import retire_ref as rr
import transform_ref as tr
from test_retire_ref import build
from visualslam_android_amd import capi

NK, N = 4, 37
BOUND = 1e-12                    # x (1 + extent): about 30 roundings of 1.1e-16 with a wide margin


def blob0(seed=3):
    """a well-formed blob whose geometry is a small scene: points in a box of a few units, cameras around it, sane depths and velocity"""
    rng = np.random.default_rng(seed)
    b = build(NK, [(i % NK, 0, 2) for i in range(N)], [[1] * N] * NK, iter_list=list(range(0, N, 2)), parts=rr.PART_IDLE | rr.PART_RELOC)
    h, s = rr.sections(b)
    s[rr.POINT_POS] = (rng.normal(size=(N, 3)) * 2.0).reshape(-1).view(np.uint8)
    rest = s[rr.POINT_REST].reshape(N, rr.REST_BYTES).copy()
    rest[:, :48] = (rng.normal(size=(N, 6)) * 1e-3).view(np.uint8).reshape(N, 48)
    s[rr.POINT_REST] = rest.reshape(-1)
    td = s[rr.TRACKDATA].reshape(N, rr.TRACKDATA_BYTES).copy()
    td[:, :24] = (rng.normal(size=(N, 3)) + [0, 0, 4]).view(np.uint8).reshape(N, 24)
    s[rr.TRACKDATA] = td.reshape(-1)
    poses = np.stack([tr.pose12(tr.rotation(rng.normal(size=3), rng.uniform(0, 1)), rng.normal(size=3) * 3) for _ in range(NK + 4)])
    s[rr.KF_POSE] = poses[:NK].reshape(-1).view(np.uint8)
    s[rr.KF_DEPTH] = rng.uniform(1, 5, size=(NK, 2)).reshape(-1).view(np.uint8)
    st = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes())
    st.pose_final[:], st.start_pose[:], st.pose_cur[:] = poses[NK].tolist(), poses[NK + 1].tolist(), poses[NK + 2].tolist()
    st.velocity[:] = (rng.normal(size=6) * 0.01).tolist()
    st.msd_vel, st.depth_mean, st.depth_sigma, st.wiggle_depth_norm = 0.003, 4.1, 0.9, 0.02
    s[rr.STATE] = np.frombuffer(bytes(st), np.uint8).copy()
    ri = rr.RelocInfo.from_buffer_copy(s[rr.RELOC_INFO].tobytes())
    ri.best_pose[:] = poses[NK + 3].tolist()
    ri.ln_adj[:] = (rng.normal(size=6) * 0.1).tolist()
    s[rr.RELOC_INFO] = np.frombuffer(bytes(ri), np.uint8).copy()
    return rr.assemble(h, s)


def geometry(blob):
    """the lengths and poses of a blob -> (positions, pixel vectors, camera-frame points, poses [nk + 4, 12], velocity, depths)"""
    h, s = rr.sections(blob)
    st = rr.TrackerState.from_buffer_copy(s[rr.STATE].tobytes())
    ri = rr.RelocInfo.from_buffer_copy(s[rr.RELOC_INFO].tobytes())
    pos = s[rr.POINT_POS].view(np.float64).reshape(-1, 3)
    vec = np.ascontiguousarray(s[rr.POINT_REST].reshape(-1, rr.REST_BYTES)[:, :48]).view(np.float64).reshape(-1, 6)
    cam = np.ascontiguousarray(s[rr.TRACKDATA].reshape(-1, rr.TRACKDATA_BYTES)[:, :24]).view(np.float64).reshape(-1, 3)
    poses = np.concatenate([s[rr.KF_POSE].view(np.float64).reshape(-1, 12), [st.pose_final[:], st.start_pose[:], st.pose_cur[:], ri.best_pose[:]]])
    depths = np.concatenate([s[rr.KF_DEPTH].view(np.float64), [st.depth_mean, st.depth_sigma]])
    return pos, vec, cam, poses, np.array(st.velocity[:]), depths


def distance(a, b):
    """largest difference over all lengths and poses of two blobs, relative to 1 + the extent of the larger"""
    worst = 0.0
    for x, y in zip(geometry(a), geometry(b)):
        worst = max(worst, float(np.abs(x - y).max() / (1.0 + max(np.abs(x).max(), np.abs(y).max()))))
    return worst


T_A, S_A = tr.pose12(tr.rotation([1, 2, -0.5], 0.9), [0.3, -1.2, 2.0]), 1.7
T_B, S_B = tr.pose12(tr.rotation([-0.2, 0.4, 1.0], 2.6), [-4.0, 0.5, 0.25]), 0.35


def test_a_transform_and_its_inverse_bring_everything_back():
    b = blob0()
    moved = tr.transform_blob(b, T_A, S_A)
    assert distance(b, moved) > 0.1
    Ti, si = tr.invert(T_A, S_A)
    back = tr.transform_blob(moved, Ti, si)
    d = distance(b, back)
    print("round trip through (T, s) and its inverse: %.3e (bound %.0e)" % (d, BOUND))
    assert d <= BOUND


def test_two_transforms_equal_their_composition():
    b = blob0()
    ab = tr.transform_blob(tr.transform_blob(b, T_A, S_A), T_B, S_B)
    Tc, sc = tr.compose(T_B, S_B, T_A, S_A)                            # the formula of vslam_get_transform_info
    R_A, R_B = T_A[:9].reshape(3, 3), T_B[:9].reshape(3, 3)
    assert np.abs(Tc[:9].reshape(3, 3) - R_B @ R_A).max() < 1e-15 and np.abs(Tc[9:] - (S_B * R_B @ T_A[9:] + T_B[9:])).max() < 1e-14 and sc == S_B * S_A
    once = tr.transform_blob(b, Tc, sc)
    d = distance(ab, once)
    print("A then B against the composition: %.3e (bound %.0e)" % (d, BOUND))
    assert d <= BOUND
    # the meaning of the composition, on a point of its own: x'' = R_B (s_B (R_A (s_A x) + t_A)) + t_B
    x = np.array([0.7, -0.3, 2.2])
    assert np.abs(tr.sim_point(Tc, sc, x) - tr.sim_point(T_B, S_B, tr.sim_point(T_A, S_A, x))).max() <= BOUND * (1 + 10)
    # the identity behind anything is that thing
    Ti, si = tr.compose(T_A, S_A, tr.pose12(np.eye(3), np.zeros(3)), 1.0)
    assert np.abs(Ti - T_A).max() == 0 and si == S_A


def test_the_direct_meaning_of_each_row():
    """independent of the restated expression order: plain matrix arithmetic"""
    b = blob0()
    moved = tr.transform_blob(b, T_A, S_A)
    R, t = T_A[:9].reshape(3, 3), T_A[9:]
    p0, v0, c0, C0, vel0, d0 = geometry(b)
    p1, v1, c1, C1, vel1, d1 = geometry(moved)
    assert np.abs(p1 - (S_A * p0 @ R.T + t)).max() < 1e-13
    assert np.abs(v1.reshape(-1, 3) - S_A * v0.reshape(-1, 3) @ R.T).max() < 1e-15
    assert np.array_equal(c1, c0 * S_A) and np.array_equal(d1, d0 * S_A)
    assert np.array_equal(vel1[:3], vel0[:3] * S_A) and np.array_equal(vel1[3:], vel0[3:])
    for a, c in zip(C0, C1):                                          # a camera sees a moved point where it saw the point: C' x' = s C x
        Ra, ta, Rc, tc = a[:9].reshape(3, 3), a[9:], c[:9].reshape(3, 3), c[9:]
        assert np.abs(Rc - Ra @ R.T).max() < 1e-15
        assert np.abs((p1 @ Rc.T + tc) - S_A * (p0 @ Ra.T + ta)).max() < 1e-12


def test_every_byte_the_rule_does_not_name_stays():
    b = blob0()
    moved = tr.transform_blob(b, T_A, S_A)
    assert len(moved) == len(b) and capi.snapshot_info(moved).total_bytes == len(b)
    (h0, s0), (h1, s1) = rr.sections(b), rr.sections(moved)
    assert bytes(h0) == bytes(h1)
    named = {rr.STATE, rr.POINT_POS, rr.POINT_REST, rr.TRACKDATA, rr.KF_POSE, rr.KF_DEPTH, rr.RELOC_INFO}
    for i in range(rr.N_SECTIONS):
        if i not in named:
            assert np.array_equal(s0[i], s1[i]), i
    assert np.array_equal(s0[rr.POINT_REST].reshape(N, -1)[:, 48:], s1[rr.POINT_REST].reshape(N, -1)[:, 48:])
    assert np.array_equal(s0[rr.TRACKDATA].reshape(N, -1)[:, 24:], s1[rr.TRACKDATA].reshape(N, -1)[:, 24:])
    a, c = rr.TrackerState.from_buffer_copy(s0[rr.STATE].tobytes()), rr.TrackerState.from_buffer_copy(s1[rr.STATE].tobytes())
    for f in ("pose_final", "start_pose", "pose_cur"):
        getattr(a, f)[:] = getattr(c, f)[:]
    a.velocity[0:3] = c.velocity[0:3]
    a.depth_mean, a.depth_sigma = c.depth_mean, c.depth_sigma
    assert bytes(a) == bytes(c)                                      # msd_vel, wiggle_depth_norm, the rotational velocity and every count among it
    ra, rc = rr.RelocInfo.from_buffer_copy(s0[rr.RELOC_INFO].tobytes()), rr.RelocInfo.from_buffer_copy(s1[rr.RELOC_INFO].tobytes())
    ra.best_pose[:] = rc.best_pose[:]
    assert bytes(ra) == bytes(rc)
    # a rigid move leaves every `*= s` field bitwise alone; the identity leaves the whole blob alone up to the sign of a zero
    rigid = tr.transform_blob(b, T_A, 1.0)
    g0, g1 = geometry(b), geometry(rigid)
    assert np.array_equal(g0[2], g1[2]) and np.array_equal(g0[4], g1[4]) and np.array_equal(g0[5], g1[5])
    same = tr.transform_blob(b, tr.pose12(np.eye(3), np.zeros(3)), 1.0)
    assert all(np.array_equal(x, y) for x, y in zip(geometry(b), geometry(same)))
    # a blob without the optional parts, and an empty map
    bare = build(2, [], [[], []], parts=0)
    out = tr.transform_blob(bare, T_A, S_A)
    assert len(out) == len(bare) and capi.snapshot_info(out).n_points == 0
