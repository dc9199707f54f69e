"""CPU tests of the epipolar line geometry and the triangulation on the synthetic cases of tests/epipolar_cases.py.

a. The oracle's epipolar_line (the function its AddPointEpipolar runs, oracle/mapgrow.cpp) against a plain 50-digit restatement of
   jni/MapMaker.cc:544-591 (mpmath): why and the clipped flag equal on every case; every case stands off every threshold it is compared
   at; the continuous outputs within 8 x the worst error measured over these cases.
b. What a case is named for is what happens: why, clipped, the clamps that act; every branch has its cases, on both sides.
c. The triangulation: conditioned and small-baseline cases against a 50-digit SVD, with the same rule; the degenerate cases in the
   oracle's two builds (the product's transcendentals, glibc's) with the same bits, finite where finite.  A float64 restatement of the
   two-sided Jacobi SVD in Python, which counts the t == 0.0 and y == 0.0 steps, returns the oracle's bits and shows that the cases
   named for those steps take them.

Measured on the CPU, the oracle's worst error over the 344 line and 32 + 12 triangulation cases (test_line_geometry_against_mpmath and
test_triangulation_against_mpmath print them; the bars are 8 x these):
  along / normal, absolute                                        1.10e-14   MEASURED_DIRECTION
  dNormDist, relative to max(1, |dNormDist|)                      7.00e-14   MEASURED_NORM_DIST
  dMinLen / dMaxLen, absolute (they lie in [-2, 2])               5.56e-15   MEASURED_LEN
  the same three over the ill-conditioned cases -- an end of the segment nearer than 5e-4 to the target's image plane, or a segment
  shorter than 5e-4 (_ill): the quotient by that depth or length multiplies the roundings before it
                                                                  1.11e-12, 5.62e-11, 8.71e-13   MEASURED_*_ILL
  the depths of the ray's ends and their gap, relative to the operands' size      4.17e-16   MEASURED_DEPTH
  the squared length, relative: conditioned 1.31e-13, ill-conditioned or below 1e-8   2.03e-09   MEASURED_ALONG_SQ, _ILL
  triangulated point, relative to its norm: conditioned           1.66e-15   MEASURED_TRI
  ... baseline 1e-6 (the two smallest singular values 1e-6 apart) 1.16e-10   MEASURED_TRI_SMALL"""
import json
import os
import subprocess
import sys

import mpmath
import numpy as np

import cam_cases as cc
import epipolar_cases as ec
import oracle.binding as orc

MARGIN = 8.0
MEASURED_DIRECTION = 1.10e-14
MEASURED_NORM_DIST = 7.00e-14
MEASURED_LEN = 5.56e-15
MEASURED_DIRECTION_ILL = 1.11e-12
MEASURED_NORM_DIST_ILL = 5.62e-11
MEASURED_LEN_ILL = 8.71e-13
MEASURED_DEPTH = 4.17e-16
MEASURED_ALONG_SQ = 1.31e-13
MEASURED_ALONG_SQ_ILL = 2.03e-09
MEASURED_TRI = 1.66e-15
MEASURED_TRI_SMALL = 1.16e-10
# How far a case must stand off a threshold, relative to the size of what is compared (the larger of 1 and the operands).  The
# oracle's error at every threshold is measured: the record holds the depths of the ray's ends, the squared length and dNormDist, so each
# case's stand-off there is also held to 8 x the oracle's error on that very case; for the clamps, whose lengths come out clamped, the
# class figures of the lengths stand in.  The fixed stand-offs (asserted below to exceed 8 x the measured figures): 1e-10 for a
# conditioned case, 1e-8 at the radius and the clamps of an ill-conditioned one.  Both lie far below NEAR (1e-6), the distance at which
# epipolar_cases places a case beside a threshold.
STANDOFF = 1e-10
STANDOFF_ILL = 1e-8

mpmath.mp.dps = 50
mpf = mpmath.mpf


# ---- the 50-digit restatement ---------------------------------------------------------------------------------------------------------
def _unproject(cam5, ix, iy):
    """UnProject (jni/ATANCamera.cc:149-164) with its switch at dist_r = 0.01 -> (x, y, dist_r)"""
    fx, fy, cx, cy, w = mpf(ec.W) * mpf(cam5[0]), mpf(ec.H) * mpf(cam5[1]), mpf(ec.W) * mpf(cam5[2]) - mpf("0.5"), mpf(ec.H) * mpf(cam5[3]) - mpf("0.5"), mpf(cam5[4])
    dx, dy = (ix - cx) / fx, (iy - cy) / fy
    d = mpmath.sqrt(dx * dx + dy * dy)
    f = mpf(1) if d <= mpf("0.01") or w == 0 else mpmath.tan(w * d) / (2 * mpmath.tan(w / 2)) / d
    return dx * f, dy * f, d


def hp_line(cam, row):
    """-> (record, margins): margins[threshold] = (value - threshold, size of what is compared) for every threshold the case reaches"""
    cam5 = cc.CALIBRATIONS[cam[0]]
    lr = mpf(ec.largest_radius(cam))                                   # the double the comparison reads; its own error is tests/test_cam_cases.py's
    m = [mpf(float(v)) for v in row]
    Rs, ts, Rt, tt = m[0:9], m[9:12], m[12:21], m[21:24]
    l = int(row[26])
    root = [(m[24] + mpf("0.5")) * (1 << l) - mpf("0.5"), (m[25] + mpf("0.5")) * (1 << l) - mpf("0.5")]
    ux, uy, dist_r = _unproject(cam5, root[0], root[1])
    n = mpmath.sqrt(ux * ux + uy * uy + 1)
    ray = [ux / n, uy / n, 1 / n]
    tmp = [Rs[0 + i] * ray[0] + Rs[3 + i] * ray[1] + Rs[6 + i] * ray[2] for i in range(3)]                       # Rs^T ray
    dirn = [Rt[3 * i] * tmp[0] + Rt[3 * i + 1] * tmp[1] + Rt[3 * i + 2] * tmp[2] for i in range(3)]
    mean, sigma, wig = m[27], m[28], m[29]
    ds, de = max(wig, mean - sigma), min(40 * wig, mean + sigma)
    c_w = [-(Rs[0 + i] * ts[0] + Rs[3 + i] * ts[1] + Rs[6 + i] * ts[2]) for i in range(3)]                       # the source's centre
    centre = [tt[i] + Rt[3 * i] * c_w[0] + Rt[3 * i + 1] * c_w[1] + Rt[3 * i + 2] * c_w[2] for i in range(3)]
    rs = [centre[i] + ds * dirn[i] for i in range(3)]
    re = [centre[i] + de * dirn[i] for i in range(3)]
    size_z = max(1, abs(tt[2]) + sum(abs(v) for v in ts) + de)
    rec = dict(why=0, clipped=0, root=root, along=[mpf(0)] * 2, normal=[mpf(0)] * 2, norm_dist=mpf(0), min_len=mpf(0), max_len=mpf(0),
               start_z=rs[2], end_z=re[2], along_sq=mpf(0), size_z=size_z)
    mg = {"dist_r": (dist_r - mpf("0.01"), 1), "start depth": (wig - (mean - sigma), 1), "end depth": (40 * wig - (mean + sigma), 1), "gap": (re[2] - rs[2], size_z)}
    if re[2] <= rs[2]:
        rec["why"] = 1
        return rec, mg
    mg["re2"] = (re[2], size_z)
    if re[2] <= 0:
        rec["why"] = 1
        return rec, mg
    mg["rs2"] = (rs[2], size_z)
    if rs[2] <= 0:
        rec["clipped"] = 1
        f = mpf("0.001") - rs[2] / dirn[2]
        rs = [rs[i] + dirn[i] * f for i in range(3)]
    a, b = [rs[0] / rs[2], rs[1] / rs[2]], [re[0] / re[2], re[1] / re[2]]
    al = [a[0] - b[0], a[1] - b[1]]
    sq = al[0] * al[0] + al[1] * al[1]
    rec["along_sq"] = sq
    mg["along_sq"] = (sq / mpf("0.00000001") - 1, 1)
    if sq < mpf("0.00000001"):
        rec["why"] = 2; rec["along"] = al
        return rec, mg
    nn = mpmath.sqrt(sq)
    rec["small"] = min(rs[2], re[2], nn)
    al = [al[0] / nn, al[1] / nn]
    nrm = [al[1], -al[0]]
    nd = a[0] * nrm[0] + a[1] * nrm[1]
    rec.update(along=al, normal=nrm, norm_dist=nd)
    mg["radius"] = (abs(nd) - lr, max(1, abs(nd)))
    if abs(nd) > lr:
        rec["why"] = 3
        return rec, mg
    la, lb = al[0] * a[0] + al[1] * a[1], al[0] * b[0] + al[1] * b[1]
    lo, hi = min(la, lb) - mpf("0.05"), max(la, lb) + mpf("0.05")
    mg.update({"min<-2": (lo + 2, max(1, abs(lo))), "max<-2": (hi + 2, max(1, abs(hi))), "min>2": (lo - 2, max(1, abs(lo))), "max>2": (hi - 2, max(1, abs(hi)))})
    rec["clamps"] = tuple(sorted(k for k, on in (("min<-2", lo < -2), ("max<-2", hi < -2), ("min>2", lo > 2), ("max>2", hi > 2)) if on))
    rec["min_len"], rec["max_len"] = min(max(lo, -2), 2), min(max(hi, -2), 2)
    return rec, mg


def _ill(rec):
    """an end of the segment nearer than 5e-4 to the target's image plane (the clip itself re-starts at 1e-3 dirn[2]), or a segment
    shorter than 5e-4: the quotient by that depth, or the normalisation by that length, multiplies the roundings before it"""
    return "small" in rec and rec["small"] < mpf("5e-4")


def _abs_err(got, want):
    return max(float(abs(mpf(float(g)) - w)) for g, w in zip(got, want))


_evaluated = {}


def evaluated(cam):
    if cam not in _evaluated:
        cases, rows = ec.line_rows(cam)
        flags, out = orc.eval_epipolar(cc.CALIBRATIONS[cam[0]], ec.W, ec.H, rows, quirks=cam[1])
        _evaluated[cam] = (cases, flags, out, [hp_line(cam, c.row) for c in cases])
    return _evaluated[cam]


# ---- a ------------------------------------------------------------------------------------------------------------------------------
def test_line_geometry_against_mpmath():
    worst = dict(direction=0.0, norm_dist=0.0, length=0.0)
    worst_ill = dict(worst)
    worst_at = dict(depth=0.0, along_sq=0.0, along_sq_ill=0.0)           # the oracle's error in what the first three tests compare
    n = 0
    for cam in ec.CAMS:
        cases, flags, out, hp = evaluated(cam)
        for c, f, o, (rec, mg) in zip(cases, flags, out, hp):
            n += 1
            assert int(f[0]) == rec["why"] and int(f[1]) == rec["clipped"], (c, f, rec["why"], rec["clipped"])
            for thr, (v, size) in mg.items():                            # the stand-off at every threshold the case reaches
                if thr in c.exact:
                    assert v == 0, (c, thr, v)
                else:
                    need = STANDOFF_ILL if _ill(rec) and thr in ("radius",) + ec.CLAMPS else STANDOFF
                    assert abs(v) > need * size, (c, thr, float(v), float(size))
            assert set(c.exact) <= set(mg), (c, c.exact)
            # ... and it exceeds the oracle's own error there, measured on this case: the depths of the ray's ends, their gap, the squared
            # length and dNormDist are in the record; the clamps' lengths are not (they come out clamped): their class bound is asserted below
            od = lambda x: mpf(float(x))
            err = {"rs2": abs(od(o[9]) - rec["start_z"]), "re2": abs(od(o[10]) - rec["end_z"]), "gap": abs((od(o[10]) - od(o[9])) - (rec["end_z"] - rec["start_z"])),
                   "along_sq": abs(od(o[11]) - rec["along_sq"]) / mpf("0.00000001"), "radius": abs(abs(od(o[6])) - abs(rec["norm_dist"]))}
            for thr, e in err.items():
                if thr in mg and thr not in c.exact:
                    assert abs(mg[thr][0]) > MARGIN * e, (c, thr, float(mg[thr][0]), float(e))
            worst_at["depth"] = max(worst_at["depth"], float(max(err["rs2"], err["re2"], err["gap"]) / rec["size_z"]))
            if "along_sq" in mg and rec["along_sq"] > mpf("1e-20"):
                k = "along_sq_ill" if _ill(rec) or rec["why"] == 2 else "along_sq"
                worst_at[k] = max(worst_at[k], float(abs(od(o[11]) - rec["along_sq"]) / rec["along_sq"]))
            assert o[0] == float(rec["root"][0]) and o[1] == float(rec["root"][1]), (c, o[:2])         # exact in both
            w = worst_ill if _ill(rec) else worst
            w["direction"] = max(w["direction"], _abs_err(o[2:6], rec["along"] + rec["normal"]))
            w["norm_dist"] = max(w["norm_dist"], _abs_err(o[6:7], [rec["norm_dist"]]) / max(1.0, abs(float(rec["norm_dist"]))))
            w["length"] = max(w["length"], _abs_err(o[7:9], [rec["min_len"], rec["max_len"]]))
            if rec["why"] != 0:                                          # what an exit does not reach stays 0
                assert (o[7:9] == 0).all() and (rec["why"] == 3 or o[6] == 0) and (rec["why"] >= 2 or (o[2:6] == 0).all()), (c, o)
    print("%d line cases; worst errors of the oracle: %s; ill-conditioned cases: %s; at the first three tests: %s" % (
        n, {k: "%.3g" % v for k, v in worst.items()}, {k: "%.3g" % v for k, v in worst_ill.items()}, {k: "%.3g" % v for k, v in worst_at.items()}))
    assert worst_at["depth"] <= MARGIN * MEASURED_DEPTH and MARGIN * MEASURED_DEPTH < STANDOFF
    assert worst_at["along_sq"] <= MARGIN * MEASURED_ALONG_SQ and MARGIN * MEASURED_ALONG_SQ < STANDOFF
    assert worst_at["along_sq_ill"] <= MARGIN * MEASURED_ALONG_SQ_ILL
    assert n >= 300
    for k, b in (("direction", MEASURED_DIRECTION), ("norm_dist", MEASURED_NORM_DIST), ("length", MEASURED_LEN)):
        assert worst[k] <= MARGIN * b, (k, worst[k], b)
        assert MARGIN * b < STANDOFF                                     # the stand-off of the radius and the clamps exceeds the oracle's error there
    for k, b in (("direction", MEASURED_DIRECTION_ILL), ("norm_dist", MEASURED_NORM_DIST_ILL), ("length", MEASURED_LEN_ILL)):
        assert worst_ill[k] <= MARGIN * b, (k, worst_ill[k], b)
        assert MARGIN * b < STANDOFF_ILL


# ---- b ------------------------------------------------------------------------------------------------------------------------------
def test_every_case_does_what_it_is_named_for():
    seen = {}
    for cam in ec.CAMS:
        cases, _flags, _out, hp = evaluated(cam)
        for c, (rec, mg) in zip(cases, hp):
            w = c.want
            assert w["why"] is None or w["why"] == rec["why"], (c, w, rec["why"])
            assert w["clipped"] == rec["clipped"], (c, w, rec["clipped"])
            if rec["why"] == 0 and w["clamps"] is not None:
                assert w["clamps"] == rec["clamps"], (c, w, rec["clamps"])
            seen.setdefault(cam, []).append((c, rec, mg))
    for cam, lst in seen.items():
        lr = ec.largest_radius(cam)
        near = lambda thr, side: sum(1 for _c, _r, mg in lst if thr in mg and mg[thr][0] * side > 0 and abs(mg[thr][0]) < 1e-4 * mg[thr][1])
        count = lambda pred: sum(1 for c, r, mg in lst if pred(c, r, mg))
        assert {c.level for c, r, _mg in lst if r["why"] == (0 if lr > 0 else 3)} == {0, 1, 2, 3}, cam
        # stage 1 by either test, the exact tie, and next to zero on both sides of each
        assert count(lambda c, r, mg: r["why"] == 1 and "re2" not in mg) >= 4 and count(lambda c, r, mg: r["why"] == 1 and "re2" in mg) >= 4, cam
        assert count(lambda c, r, mg: "gap" in c.exact and r["why"] == 1) >= 1 and near("gap", 1) >= 1 and near("gap", -1) >= 1, cam
        assert near("re2", 1) >= 1 and near("re2", -1) >= 1 and near("rs2", 1) >= 1 and near("rs2", -1) >= 1, cam
        assert count(lambda c, r, mg: r["clipped"] == 1) >= 6, cam
        assert count(lambda c, r, mg: r["clipped"] == 1 and c.name.startswith("clip: dirn[2]")) >= 2, cam
        assert near("along_sq", 1) >= 1 and near("along_sq", -1) >= 1, cam
        for thr in ("start depth", "end depth"):                         # each depth taken from either source
            assert count(lambda c, r, mg: mg[thr][0] > 0) >= 5 and count(lambda c, r, mg: mg[thr][0] < 0) >= 5, (cam, thr)
        if lr > 0:
            for sign in (1, -1):                                         # both sides of the radius at both signs of dNormDist
                for side in (1, -1):
                    assert count(lambda c, r, mg: "radius" in mg and r["norm_dist"] * sign > 0 and mg["radius"][0] * side > 0 and abs(mg["radius"][0]) < 1e-5) >= 1, (cam, sign, side)
            for thr in ec.CLAMPS:
                assert near(thr, 1) >= 1 and near(thr, -1) >= 1, (cam, thr)
            sets = {r["clamps"] for _c, r, _mg in lst if r["why"] == 0}
            assert {(), ("min<-2",), ("max>2",), ("max<-2", "min<-2"), ("max>2", "min>2"), ("max>2", "min<-2")} <= sets, (cam, sets)
            assert not any(("max<-2" in s and "min<-2" not in s) or ("min>2" in s and "max>2" not in s) for s in sets)     # (the docstring's argument)
        else:
            assert lr == 0 and count(lambda c, r, mg: r["why"] == 0) == 0 and count(lambda c, r, mg: r["why"] == 3) >= 20, cam
    assert len({c for c, _q in ec.CAMS if _q == 0}) >= 2 and any(q for _c, q in ec.CAMS)


# ---- c ------------------------------------------------------------------------------------------------------------------------------
def _matrix(row):
    T, a, b = row[:12], row[12:14], row[14:16]
    PD = [[T[0], T[1], T[2], T[9]], [T[3], T[4], T[5], T[10]], [T[6], T[7], T[8], T[11]]]
    A = [[-1.0, 0.0, b[0], 0.0], [0.0, -1.0, b[1], 0.0], [a[0] * PD[2][c] - PD[0][c] for c in range(4)], [a[1] * PD[2][c] - PD[1][c] for c in range(4)]]
    return [[float(v) for v in r] for r in A]


def _svd4_py(A):
    """the two-sided Jacobi SVD of oracle/mapgrow.cpp in Python's doubles (+, *, / and sqrt round as in C++ without contraction)
    -> (vector, sweeps, steps with t == 0.0, steps with y == 0.0)"""
    sqrt = np.sqrt
    M = [list(r) for r in A]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    prec = 2.0 * 2.220446049250313e-16
    sweeps = t_zero = y_zero = 0
    for sweep in range(64):
        finished = True
        sweeps += 1
        for p in range(1, 4):
            for q in range(p):
                off, dia = max(abs(M[p][q]), abs(M[q][p])), max(abs(M[p][p]), abs(M[q][q]))
                if not off > dia * prec:
                    continue
                finished = False
                m00, m01, m10, m11 = M[p][p], M[p][q], M[q][p], M[q][q]
                t, d = m00 + m11, m10 - m01
                if t == 0.0:
                    c1, s1 = 0.0, (1.0 if d > 0.0 else -1.0); t_zero += 1
                else:
                    u = d / t
                    c1 = 1.0 / sqrt(1.0 + u * u); s1 = c1 * u
                x, y, z = c1 * m00 + s1 * m10, c1 * m01 + s1 * m11, -s1 * m01 + c1 * m11
                if y == 0.0:
                    c2, s2 = 1.0, 0.0; y_zero += 1
                else:
                    tau = (x - z) / (2.0 * abs(y)); w = sqrt(tau * tau + 1.0)
                    tt = 1.0 / (tau + w) if tau > 0.0 else 1.0 / (tau - w)
                    sign_t = 1.0 if tt > 0.0 else -1.0
                    n = 1.0 / sqrt(tt * tt + 1.0)
                    s2 = -sign_t * (y / abs(y)) * abs(tt) * n; c2 = n
                cl, sl = c1 * c2 + s1 * s2, s1 * c2 - c1 * s2
                for k in range(4):
                    a, b = M[p][k], M[q][k]
                    M[p][k] = cl * a + sl * b; M[q][k] = -sl * a + cl * b
                for X in (M, V):
                    for k in range(4):
                        a, b = X[k][p], X[k][q]
                        X[k][p] = c2 * a - s2 * b; X[k][q] = s2 * a + c2 * b
        if finished:
            break
    best = 0
    for i in range(1, 4):
        if abs(M[i][i]) < abs(M[best][best]):
            best = i
    return [V[k][best] for k in range(4)], sweeps, t_zero, y_zero


def _hp_point(row):
    A = mpmath.matrix([[mpf(v) for v in r] for r in _matrix(row)])      # the matrix as the doubles build it (its entries are exact to an ulp)
    _U, S, V = mpmath.svd_r(A, compute_uv=True)
    k = min(range(4), key=lambda i: S[i])
    v = [V[k, j] for j in range(4)]
    return [v[0] / v[3], v[1] / v[3], v[2] / v[3]], sorted(float(s) for s in S)


def test_triangulation_against_mpmath():
    cases, rows = ec.tri_rows()
    out = orc.eval_triangulation(rows)
    worst = {"conditioned": 0.0, "small baseline": 0.0}
    for c, row, o in zip(cases, rows, out):
        assert np.array_equal(o[4:7], orc.reproject_point(row[:12], row[12:14], row[14:16]), equal_nan=True), c      # the entry the suite already holds
        if c.kind == "degenerate":
            continue
        want, S = _hp_point(row)
        nrm = float(mpmath.sqrt(sum(w * w for w in want)))
        worst[c.kind] = max(worst[c.kind], _abs_err(o[4:7], want) / nrm)
        assert np.abs(np.array([float(w) for w in want]) - c.point).max() < (1e-12 if c.kind == "conditioned" else 1e-6) * nrm, (c, want, c.point)   # (the restatement finds the point)
        if c.kind == "small baseline":
            assert S[1] < 1e-5, (c, S)
    print("worst relative error of the triangulated point:", {k: "%.3g" % v for k, v in worst.items()})
    assert sum(c.kind == "conditioned" for c in cases) >= 20 and sum(c.kind == "small baseline" for c in cases) >= 8
    assert worst["conditioned"] <= MARGIN * MEASURED_TRI, worst
    assert worst["small baseline"] <= MARGIN * MEASURED_TRI_SMALL, worst


def test_jacobi_steps_with_exact_zeros_are_taken():
    cases, rows = ec.tri_rows()
    out = orc.eval_triangulation(rows)
    steps = {}
    for c, row, o in zip(cases, rows, out):
        v, sweeps, tz, yz = _svd4_py(_matrix(row))
        assert np.array_equal(np.array(v), o[:4], equal_nan=True), (c, v, o[:4])
        assert sweeps < 64, (c, sweeps)                                   # the cap is reached by no case
        steps[c.name] = (tz, yz, v[3] == 0.0)
        if v[3] == 0.0:
            assert np.array_equal(o[4:7], np.array(v[:3]) / 0.00001), c
    print({k: v for k, v in steps.items() if any(v)})
    for name in ("t == 0 at pair (2, 0), d > 0", "t == 0 at pair (2, 0), d < 0", "t == 0 at pair (2, 0), d == 0"):
        assert steps[name][0] >= 1, (name, steps[name])
    for name in ("y == 0 at pair (3, 2)", "identity pose, rays on the axis"):
        assert steps[name][1] >= 1, (name, steps[name])
    assert steps["identity pose, rays on the axis"][2]                  # v[3] == 0.0 exactly
    assert not any(any(steps[c.name]) for c in cases if c.kind != "degenerate")


def test_degenerate_triangulations_agree_in_both_builds():
    """the oracle on the product's transcendentals and on glibc's: the SVD calls none, so the bits are the same; finite stays finite"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json, warnings\nwarnings.simplefilter('ignore')\nsys.path[:0] = [%r, %r]\nimport epipolar_cases as ec, oracle.binding as orc\n"
            "o = orc.eval_triangulation(ec.tri_rows()[1])\nprint(json.dumps([[float(v).hex() for v in r] for r in o]))\n") % (root, os.path.join(root, "tests"))
    a, b = [json.loads(subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, ORC_ORACLE_VARIANT=v), text=True).strip().splitlines()[-1])
            for v in ("", "stdlibm")]
    cases, _rows = ec.tri_rows()
    n = 0
    for c, ra, rb in zip(cases, a, b):
        if c.kind != "degenerate":
            continue
        n += 1
        assert ra == rb, (c, ra, rb)
        va = np.array([float.fromhex(v) for v in ra])
        assert np.array_equal(np.isfinite(va), np.isfinite(np.array([float.fromhex(v) for v in rb]))), c
    assert n >= 10
