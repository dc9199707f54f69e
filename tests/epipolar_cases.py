"""Synthetic cases for the line geometry of AddPointEpipolar (csrc/grow_dev.h epipolar_line, jni/MapMaker.cc:544-591) and for the
triangulation (reproject_vector / reproject_point, :174-200), shared by tests/test_epipolar_cases.py (CPU: the oracle's twin against a
50-digit restatement) and tests/test_gpu_epipolar_cases.py (GPU: the device == the oracle's twin, bit for bit).  No GPU is touched here.

Natural scenes leave most of this arithmetic on one side of its thresholds (tests/grow_cases.py), so the cases are poses and candidates
chosen for a branch each, and named for it.  A line case is stated in the source keyframe's frame: the target keyframe's pose relative
to the source (R, t), a candidate (level position, level), the source's scene depth (mean, sigma) and wiggle_scale.  Then
dirn = R ray, the source's centre lies at t, and the ray runs from t + dStart dirn to t + dEnd dirn.  Both poses are then moved into one
of three world frames (WORLDS), which changes no geometry and every rounding.  A case that must lie next to a threshold is tuned by
bisection on a float64 restatement (internals()) to the threshold x (1 +- NEAR); which side it lies on, and by how much, is then
asserted with 50 digits by the CPU test, never taken from here.

What every case expects (`want`): why (0 the line stands, 1 ray, 2 short segment, 3 radius), clipped, and which of the four clamps act:
"min<-2", "max<-2", "min>2", "max>2".  along points from the far end of the segment to the near end, so along . v2A - along . v2B is the
segment's length, > 0: dMinLen comes from the far end (lb), dMaxLen from the near end (la).  Hence "max<-2" implies "min<-2" and
"min>2" implies "max>2": those two clamps never act alone, and the cases hold each of them in its pair.

Triangulation cases are (AfromB, v2A, v2B).  The conditioned ones are exact projections of a point; the degenerate ones are named
for what they do to the 4 x 4 matrix.  AfromB need not be a rigid motion there: with v2A = 0 its first two rows are, negated, the third
and fourth row of the matrix, which is how the exact zeros of the t == 0.0 and y == 0.0 steps of the 2 x 2 Jacobi step are placed.
v[3] == 0.0 exactly is reached: with the identity pose and both rays on the axis the matrix has the null space (0, 0, a, b), the first
rotation (pair 2, 0) takes y == 0.0, and the column of the first smallest |m_ii| (i = 2) has no fourth component ("identity pose, rays
on the axis").  The cap of 64 sweeps is not reached by any case: no 4 x 4 input was found that needs more than a few sweeps."""
import functools

import numpy as np

import cam_cases as cc
import oracle.binding as orc
from visualslam_android_amd import capi

W, H = 64, 48
CAMS = (("ref", 0), ("wide", 0), ("pincushion", 0), ("ref", 1))           # (calibration of cam_cases, quirks); quirks = 1: largest_radius = 0
NEAR = 1e-6                                                                # relative distance of a tuned case from its threshold
CLAMPS = ("min<-2", "max<-2", "min>2", "max>2")


def cam_key(cam):
    return "%s%s" % (cam[0], ", quirks 1" if cam[1] else "")


@functools.lru_cache(maxsize=None)
def largest_radius(cam):
    return float(orc.cam_eval(cc.CALIBRATIONS[cam[0]], W, H, np.zeros((0, 2)), quirks=cam[1])[1][2])


# ---- poses --------------------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def pose12(R, t):
    return np.r_[np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64)]


def compose(a, b):
    """x -> a(b(x))"""
    Ra, Rb = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
    return pose12(Ra @ Rb, Ra @ b[9:] + a[9:])


WORLDS = (pose12(np.eye(3), (0, 0, 0)), pose12(rot((0.3, -1.0, 0.2), 37.0), (0.4, -1.3, 2.2)), pose12(rot((1.0, 0.4, -0.7), -141.0), (-3.1, 0.7, 5.9)))
Y = (0.0, 1.0, 0.0)


class LineCase:
    def __init__(self, name, cam, R, t, pos, level, depth, world, want_why, clipped=0, clamps=(), exact=()):
        """depth = (mean, sigma, wiggle_scale); exact: the thresholds this case sits on exactly (see test_epipolar_cases.THRESHOLDS)"""
        self.name, self.cam, self.level, self.world = name, cam, int(level), world
        self.want = dict(why=want_why, clipped=clipped, clamps=None if clamps is None else tuple(sorted(clamps)))   # None: not stated
        self.exact = tuple(exact)
        rel = pose12(R, t)
        row, F = np.zeros(30), capi.EPI_LINE_IN                         # the layout vslam_eval_epipolar states
        row[F["src"]] = WORLDS[world]; row[F["tgt"]] = compose(rel, WORLDS[world])
        row[F["pos"]] = pos; row[F["level"]] = level
        row[F["depth_mean"]], row[F["depth_sigma"]], row[F["wiggle_scale"]] = depth
        self.row = row

    def __repr__(self):
        return "%s [%s]" % (self.name, cam_key(self.cam))


# ---- a float64 restatement that shows the values the thresholds look at (for tuning only) -----------------------------------------------
def internals(cam, row):
    cam5 = cc.CALIBRATIONS[cam[0]]
    Rs, ts, Rt, tt = row[0:9].reshape(3, 3), row[9:12], row[12:21].reshape(3, 3), row[21:24]
    l = int(row[26])
    root = (row[24:26] + 0.5) * (1 << l) - 0.5
    u = orc.cam_unproject(cam5, W, H, root[0], root[1])
    ray = np.r_[u, 1.0] / np.sqrt(u[0] * u[0] + u[1] * u[1] + 1.0)
    dirn = Rt @ (Rs.T @ ray)
    mean, sigma, wig = row[27:30]
    ds, de = max(wig, mean - sigma), min(40 * wig, mean + sigma)
    centre = Rt @ (-(Rs.T @ ts)) + tt
    rs, re = centre + ds * dirn, centre + de * dirn
    out = dict(rs2=rs[2], re2=re[2], gap=re[2] - rs[2], dirn2=dirn[2])
    if re[2] <= rs[2] or re[2] <= 0:
        return out
    if rs[2] <= 0:
        rs = rs + dirn * (0.001 - rs[2] / dirn[2])
    a, b = rs[:2] / rs[2], re[:2] / re[2]
    al = a - b
    out["along_sq"] = al @ al
    if out["along_sq"] < 1e-8:
        return out
    al = al / np.sqrt(al @ al)
    nrm = np.array([al[1], -al[0]])
    out.update(norm_dist=a @ nrm, la=al @ a, lb=al @ b)
    return out


def tune(make, key, target, lo, hi, fn=lambda v: v):
    """the parameter x in [lo, hi] at which fn(internals(make(x))[key]) crosses target (bisection; the bracket must hold one crossing)"""
    def f(x):
        c = make(x)
        return fn(internals(c.cam, c.row)[key]) - target
    flo = f(lo)
    assert flo * f(hi) < 0, (key, target, flo, f(hi))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if f(mid) * flo > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


# ---- the line cases -------------------------------------------------------------------------------------------------------------------
CANDIDATES = (((40, 30), 0), ((5, 44), 0), ((20, 6), 1), ((3, 9), 2), ((6, 1), 3))                  # (level position, level): all four levels
DEPTHS = {"start mean-sigma, end mean+sigma": (2.0, 0.5, 0.1), "start wiggle_scale": (1.0, 0.95, 0.1),
          "end 40 wiggle_scale": (3.0, 1.5, 0.05), "start wiggle_scale, end mean+sigma": (0.5, 0.45, 0.1)}
D0 = DEPTHS["start mean-sigma, end mean+sigma"]                                                     # dStart 1.5, dEnd 2.5
R_SMALL = rot((0.2, 1.0, 0.1), 5.0)


def central(cam, level):
    """the candidate of `level` nearest to the principal point: its ray is the axis to a hundredth of a radian"""
    c5 = cc.CALIBRATIONS[cam[0]]
    c = np.array([W * c5[2] - 0.5, H * c5[3] - 0.5])
    return tuple(int(v) for v in np.round((c + 0.5) / (1 << level) - 0.5)), level



@functools.lru_cache(maxsize=None)
def line_cases():
    out, k = [], [0]

    def add(name, cam, R, t, cand, depth, why, **kw):
        c = LineCase(name, cam, R, t, cand[0], cand[1], depth, k[0] % len(WORLDS), why, **kw)
        k[0] += 1
        out.append(c)
        return c

    def probe(cam, R, t, cand, depth):
        return LineCase("probe", cam, R, t, cand[0], cand[1], depth, k[0] % len(WORLDS), 0)

    for cam in CAMS:
        lr = largest_radius(cam)
        stands = 0 if lr > 0 else 3                                     # with quirks = 1 the radius is 0: every line that gets there is outside
        # ---- the line stands: every level, every choice of dStartDepth / dEndDepth -------------------------------------------------------
        for cand in CANDIDATES:
            for dname, depth in DEPTHS.items():
                add("stands, %s, level %d" % (dname, cand[1]), cam, R_SMALL, (0.3, -0.1, 0.05), cand, depth, stands, clamps=None)
        # ---- stage 1 -----------------------------------------------------------------------------------------------------------------
        for cand in (CANDIDATES[0], CANDIDATES[3]):
            add("stage 1: dEnd < dStart (wiggle_scale 0.02)", cam, R_SMALL, (0.3, -0.1, 0.05), cand, (2.0, 0.5, 0.02), 1)
            add("stage 1: the ray points away from the target", cam, rot(Y, 120.0), (0.3, -0.1, 0.05), cand, D0, 1)
            add("stage 1: dEnd == dStart exactly", cam, R_SMALL, (0.3, -0.1, 0.05), cand, (2.0, 0.75, 0.03125), 1, exact=("gap",))
            add("stage 1: dEnd just below dStart", cam, R_SMALL, (0.3, -0.1, 0.05), cand, (2.0, 0.5, 1.5 / 40 * (1 - NEAR)), 1)
            add("stage 2: dEnd just above dStart", cam, R_SMALL, (0.3, -0.1, 0.05), cand, (2.0, 0.5, 1.5 / 40 * (1 + NEAR)), 2)
            add("stage 1: the ray ends far behind the target", cam, R_SMALL, (0.3, -0.1, -3.5), cand, D0, 1)
            for side, why in ((-1, 1), (1, None)):
                mk = lambda tz, cand=cand: probe(cam, R_SMALL, (0.3, -0.1, tz), cand, D0)
                tz = tune(mk, "re2", side * 1e-6, -3.5, 0.0)
                if why == 1:
                    add("stage 1: the ray ends 1e-6 behind the target's plane", cam, R_SMALL, (0.3, -0.1, tz), cand, D0, 1)
                else:                                                   # the end 1e-6 in front, the start clipped: a long line
                    add("clip: the ray ends 1e-6 in front of the target's plane", cam, R_SMALL, (0.3, -0.1, tz), cand, D0, None, clipped=1, clamps=None)
        # ---- the clip ----------------------------------------------------------------------------------------------------------------
        for cand in (CANDIDATES[0], CANDIDATES[2]):
            mk = lambda tz, cand=cand: probe(cam, R_SMALL, (0.02, 0.01, tz), cand, D0)
            add("clip: the start 0.5 behind the target's plane", cam, R_SMALL, (0.02, 0.01, tune(mk, "rs2", -0.5, -3.0, 0.0)), cand, D0, None, clipped=1, clamps=None)
            add("clip: the start 1e-6 behind the target's plane", cam, R_SMALL, (0.02, 0.01, tune(mk, "rs2", -1e-6, -3.0, 0.0)), cand, D0, None, clipped=1, clamps=None)
            add("no clip: the start 1e-6 in front of the target's plane", cam, R_SMALL, (0.02, 0.01, tune(mk, "rs2", 1e-6, -3.0, 0.0)), cand, D0, None, clipped=0, clamps=None)
        for lvl in (0, 2):                                              # dirn[2] = 2e-3: the division of the re-start
            cand = central(cam, lvl)
            Rg = rot(Y, tune(lambda th, cand=cand: probe(cam, rot(Y, th), (0.5, 0.01, 0.0), cand, D0), "dirn2", 2e-3, 60.0, 120.0))
            mk = lambda tz, cand=cand: probe(cam, Rg, (0.5, 0.01, tz), cand, D0)
            add("clip: dirn[2] = 2e-3, level %d" % lvl, cam, Rg, (0.5, 0.01, tune(mk, "rs2", -1e-3, -1.0, 0.0)), cand, D0, None, clipped=1, clamps=None)
        # ---- stage 2, both sides of 1e-8 -------------------------------------------------------------------------------------------------
        for cand in (CANDIDATES[1], CANDIDATES[4]):
            add("stage 2: the target at the source's own pose", cam, np.eye(3), (0.0, 0.0, 0.0), cand, D0, 2)
            mk = lambda b, cand=cand: probe(cam, np.eye(3), (b, 0.0, 0.0), cand, D0)
            add("stage 2: segment just shorter than 1e-4", cam, np.eye(3), (tune(mk, "along_sq", 1e-8 * (1 - 1e-4), 1e-5, 1e-2), 0.0, 0.0), cand, D0, 2)
            add("segment just longer than 1e-4", cam, np.eye(3), (tune(mk, "along_sq", 1e-8 * (1 + 1e-4), 1e-5, 1e-2), 0.0, 0.0), cand, D0, stands)
        # ---- stage 3, both sides of largest_radius, both signs of dNormDist ----------------------------------------------------------------
        if lr > 0:
            Rg = rot(Y, np.rad2deg(np.arctan(2.0 * lr)))               # the candidate's ray at x = 2 largest_radius of the target's plane
            for lvl in (0, 1, 3):
                cand = central(cam, lvl)
                for sgn in (1, -1):
                    # the baseline at the angle phi in the target's x-y plane: the line passes the axis at |p| sin(phi - phi_p)
                    mk = lambda phi, cand=cand: probe(cam, Rg, (0.3 * np.cos(phi), 0.3 * np.sin(phi), 0.0), cand, D0)
                    i0 = internals(cam, mk(0.0).row)
                    assert abs(i0["norm_dist"]) < 0.2 * lr, i0           # phi = 0 is almost along p: the line passes near the axis
                    for rel, why in ((1 + NEAR, 3), (1 - NEAR, 0), (1.6, 3), (0.5, 0)):
                        phi = tune(mk, "norm_dist", rel * lr, 0.0, sgn * np.pi / 2, fn=abs)
                        c = mk(phi)
                        nd = internals(cam, c.row)["norm_dist"]
                        add("%s largest_radius x %.7g, dNormDist %s 0, level %d" % ("stage 3: outside" if why else "inside", rel, "<" if nd < 0 else ">", lvl),
                            cam, Rg, (0.3 * np.cos(phi), 0.3 * np.sin(phi), 0.0), cand, D0, why, clamps=None)
        # ---- the clamps ----------------------------------------------------------------------------------------------------------------
        if lr > 0:
            Rn, Rp = rot(Y, -68.0), rot(Y, 45.0)                           # the candidate's ray at x = -2.5 / x = +1 of the target's plane
            for lvl in (0, 2):
                cand = central(cam, lvl)
                mkn = lambda tx, cand=cand: probe(cam, Rn, (tx, 0.0, 0.0), cand, D0)
                mkp = lambda tx, cand=cand: probe(cam, Rp, (tx, 0.0, 0.0), cand, D0)
                for rel, cl in ((1 + NEAR, ("min<-2",)), (1 - NEAR, ())):
                    add("clamp: far end at -1.95 x %.7g" % rel, cam, Rn, (tune(mkn, "lb", -1.95 * rel, 0.05, 1.0), 0.0, 0.0), cand, D0, 0, clamps=cl)
                for rel, cl in ((1 + NEAR, ("min<-2", "max<-2")), (1 - NEAR, ("min<-2",))):
                    add("clamp: near end at -2.05 x %.7g" % rel, cam, Rn, (tune(mkn, "la", -2.05 * rel, 0.01, 1.0), 0.0, 0.0), cand, D0, 0, clamps=cl)
                add("clamp: both ends far below -2", cam, Rn, (0.02, 0.0, 0.0), cand, D0, 0, clamps=("min<-2", "max<-2"))
                for rel, cl in ((1 + NEAR, ("max>2",)), (1 - NEAR, ())):
                    add("clamp: near end at 1.95 x %.7g" % rel, cam, Rp, (tune(mkp, "la", 1.95 * rel, 0.05, 3.0), 0.0, 0.0), cand, D0, 0, clamps=cl)
                for rel, cl in ((1 + NEAR, ("min>2", "max>2")), (1 - NEAR, ("max>2",))):
                    add("clamp: far end at 2.05 x %.7g" % rel, cam, Rp, (tune(mkp, "lb", 2.05 * rel, 0.05, 6.0), 0.0, 0.0), cand, D0, 0, clamps=cl)
                add("clamp: both ends far above 2", cam, Rp, (5.0, 0.0, 0.0), cand, D0, 0, clamps=("min>2", "max>2"))
                # the near end beyond +2 and the far end beyond -2: a start depth of 0.1 brings the near end far out
                dn = DEPTHS["start wiggle_scale"]
                mkb = lambda tx, cand=cand: probe(cam, Rn, (tx, 0.0, 0.0), cand, dn)
                for rel, cl in ((1 + NEAR, ("min<-2", "max>2")), (1 - NEAR, ("max>2",))):
                    add("clamp: far end at -1.95 x %.7g, near end beyond 2" % rel, cam, Rn, (tune(mkb, "lb", -1.95 * rel, 0.2, 1.0), 0.0, 0.0), cand, dn, 0, clamps=cl)
    return out


# ---- the triangulation cases ----------------------------------------------------------------------------------------------------------
class TriCase:
    def __init__(self, name, kind, T12, vA, vB, point=None):
        """kind: "conditioned" / "small baseline" (held to the 50-digit SVD) or "degenerate" (held to the oracle's two builds)"""
        self.name, self.kind, self.point = name, kind, point
        self.row = np.r_[np.asarray(T12, np.float64), np.asarray(vA, np.float64), np.asarray(vB, np.float64)]

    def __repr__(self):
        return self.name


def _projected(name, kind, R, t, X):
    """the exact-in-float64 projections of the point X (frame B) in B and in A = R X + t"""
    X = np.asarray(X, np.float64)
    XA = R @ X + np.asarray(t, np.float64)
    return TriCase(name, kind, pose12(R, t), XA[:2] / XA[2], X[:2] / X[2], X)


def _matrix_rows(name, row2, row3, vB=(0.0, 0.0)):
    """a degenerate case by its matrix: rows 0, 1 are (-1, 0, vB0, 0), (0, -1, vB1, 0); rows 2, 3 as given (v2A = 0)"""
    T = np.zeros(12)
    T[0:3] = [-row2[0], -row2[1], -row2[2]]; T[9] = -row2[3]
    T[3:6] = [-row3[0], -row3[1], -row3[2]]; T[10] = -row3[3]
    T[8] = 1.0
    return TriCase(name, "degenerate", T, (0.0, 0.0), vB)


@functools.lru_cache(maxsize=None)
def tri_cases():
    rng = np.random.RandomState(11)
    out = []
    for i in range(24):
        R = rot(rng.randn(3), rng.uniform(-25, 25))
        t = rng.randn(3) * (0.1, 0.1, 0.03) * (1 + 3 * (i % 3))
        X = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.6, 0.6), rng.uniform(0.8, 5.0)])
        out.append(_projected("conditioned %d" % i, "conditioned", R, t, X))
    for i in range(8):
        R = rot(rng.randn(3), rng.uniform(-2, 2)) if i % 2 else np.eye(3)
        d = rng.randn(3); d[2] *= 0.2
        X = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.6, 0.6), rng.uniform(0.8, 5.0)])
        out.append(_projected("baseline 1e-6, %d" % i, "small baseline", R, 1e-6 * d / np.linalg.norm(d), X))
    I = np.eye(3)
    out.append(TriCase("identical cameras, one ray", "degenerate", pose12(I, (0, 0, 0)), (0.3, -0.2), (0.3, -0.2)))
    out.append(TriCase("identical cameras, two rays", "degenerate", pose12(I, (0, 0, 0)), (0.3, -0.2), (0.31, -0.2)))
    out.append(TriCase("parallel rays, sideways baseline", "degenerate", pose12(I, (0.1, 0, 0)), (0.3, -0.2), (0.3, -0.2)))
    out.append(TriCase("parallel rays, rotated camera", "degenerate", pose12(rot(Y, 10.0), (0.1, 0.05, 0)),
                       tuple((rot(Y, 10.0) @ np.array([0.3, -0.2, 1.0]))[:2] / (rot(Y, 10.0) @ np.array([0.3, -0.2, 1.0]))[2]), (0.3, -0.2)))
    out.append(TriCase("identity pose, rays on the axis", "degenerate", pose12(I, (0, 0, 0)), (0.0, 0.0), (0.0, 0.0)))
    out.append(TriCase("baseline along the axis, rays on the axis", "degenerate", pose12(I, (0, 0, 0.5)), (0.0, 0.0), (0.0, 0.0)))
    # exact zeros by the matrix itself
    out.append(_matrix_rows("t == 0 at pair (2, 0), d > 0", (-0.25, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 2.0), vB=(0.5, 0.0)))
    out.append(_matrix_rows("t == 0 at pair (2, 0), d < 0", (0.75, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 2.0), vB=(0.5, 0.0)))
    out.append(_matrix_rows("t == 0 at pair (2, 0), d == 0", (0.5, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 2.0), vB=(0.5, 0.0)))
    out.append(_matrix_rows("y == 0 at pair (3, 2)", (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0, 2.0)))
    out.append(_matrix_rows("zero rows 2 and 3", (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0), vB=(0.25, -0.5)))
    out.append(_matrix_rows("diagonal already", (0.0, 0.0, 3.0, 0.0), (0.0, 0.0, 0.0, 0.5)))
    return out


def line_rows(cam):
    cs = [c for c in line_cases() if c.cam == cam]
    return cs, np.array([c.row for c in cs])


def tri_rows():
    cs = tri_cases()
    return cs, np.array([c.row for c in cs])
