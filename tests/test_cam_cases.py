"""CPU tests of the camera arithmetic at calibrations other than the default (tests/cam_cases.py).

a. The oracle's Project / GetProjectionDerivs / UnProject and the host form of vslam_eval_camera against a plain 50-digit restatement
   of the smooth ATAN model (mpmath): factor = atan(k r) / (w r) with k = 2 tan(w / 2), its analytic derivative, and r = tan(w d) / k.
b. Inside the reference's switch zones, the reference's rule exactly; the derived values of cam_fill / trk_fill_params.
c. The bootstrap's unproject_with_derivs (host form) against the same restatement.
d. The scenes of cam_cases do what they claim, in the oracle alone: an edge point in every exit, quality 2 in every frame, a keyframe at
   frame 0, a growing map, the ground-truth pose within 5e-3.

The bounds of a and c are 8 x the oracle's worst error over the six calibrations, measured here on the CPU (the figures stand next to
the constants).  The margin covers the 1-2 ulp of vtan / vatan and the conditioning of tan at the wide lens's image corner."""
import functools

import mpmath
import numpy as np
import pytest

import cam_cases as cc
import oracle.binding as orc
from helpers import make_oracle, pose_err
from visualslam_android_amd import capi

F = orc.CAM_EVAL_FIELDS
W, H = cc.W, cc.H

# measured worst error of the oracle over the six calibrations at 320x240 (test_oracle_and_host_form_against_mpmath prints them):
MEASURED_IM = 1.15e-13        # image position, pixels (absolute)
MEASURED_DERIVS = 5.71e-16    # derivatives, relative to the largest entry of the 2 x 2 matrix
MEASURED_UNPROJECT = 5.43e-15  # UnProject(im) against the restatement's at the same im, relative to the radius
MEASURED_BOOT_OUT = 5.43e-15  # unproject_with_derivs: position, relative to the radius
MEASURED_BOOT_JAC = 1.17e-15  # unproject_with_derivs: derivatives, relative to the largest entry
MARGIN = 8.0


# ---- the 50-digit restatement -------------------------------------------------------------------------------------------------------
class HpCamera:
    """The smooth ATAN camera (no switch zones) at 50 digits, from the double values of cam5"""

    def __init__(self, cam5, w, h):
        mpmath.mp.dps = 50
        m = mpmath.mpf
        self.focal = (m(w) * m(cam5[0]), m(h) * m(cam5[1]))
        self.center = (m(w) * m(cam5[2]) - m("0.5"), m(h) * m(cam5[3]) - m("0.5"))
        self.w = m(cam5[4])
        self.k = 2 * mpmath.tan(self.w / 2)

    def factor(self, r):
        return m1() if self.w == 0 or r == 0 else mpmath.atan(self.k * r) / (self.w * r)

    def project(self, x, y):
        x, y = mpmath.mpf(x), mpmath.mpf(y)
        f = self.factor(mpmath.sqrt(x * x + y * y))
        return self.center[0] + self.focal[0] * x * f, self.center[1] + self.focal[1] * y * f

    def derivs(self, x, y):
        """[[d im_x / dx, d im_x / dy], [d im_y / dx, d im_y / dy]] flattened"""
        x, y = mpmath.mpf(x), mpmath.mpf(y)
        r = mpmath.sqrt(x * x + y * y)
        f = self.factor(r)
        if self.w == 0 or r == 0:
            dfx = dfy = mpmath.mpf(0)
        else:
            dfdr = self.k / ((1 + self.k * self.k * r * r) * self.w * r) - f / r
            dfx, dfy = dfdr * x / r, dfdr * y / r
        return (self.focal[0] * (f + x * dfx), self.focal[0] * (x * dfy), self.focal[1] * (y * dfx), self.focal[1] * (f + y * dfy))

    def unproject(self, ix, iy):
        dx, dy = (mpmath.mpf(ix) - self.center[0]) / self.focal[0], (mpmath.mpf(iy) - self.center[1]) / self.focal[1]
        d = mpmath.sqrt(dx * dx + dy * dy)
        g = m1() if self.w == 0 or d == 0 else mpmath.tan(self.w * d) / (self.k * d)
        return dx * g, dy * g


def m1():
    return mpmath.mpf(1)


def _err(got, want):
    return max(float(abs(mpmath.mpf(float(g)) - w_)) for g, w_ in zip(got, want))


def _errors(cam5, rows, xy):
    """worst error per quantity of the evaluated rows (n, 17) at the image-plane points xy against the restatement"""
    hp = HpCamera(cam5, W, H)
    e = dict(im=0.0, derivs=0.0, unproject=0.0, boot_out=0.0, boot_jac=0.0)
    for (x, y), o in zip(xy, rows):
        r = float(np.hypot(x, y))
        e["im"] = max(e["im"], _err(o[F["im"]], hp.project(x, y)))
        want = hp.derivs(x, y)
        e["derivs"] = max(e["derivs"], _err(o[F["derivs"]], want) / float(max(abs(v) for v in want)))
        back = hp.unproject(o[0], o[1])                              # at the evaluated im, a double: UnProject's own error
        rb = float(mpmath.sqrt(back[0] ** 2 + back[1] ** 2))
        e["unproject"] = max(e["unproject"], _err(o[F["unproject"]], back) / rb)
        e["boot_out"] = max(e["boot_out"], _err(o[F["boot_out"]], back) / rb)
        want = hp.derivs(back[0], back[1])                           # the derivatives at the un-projected point, last_factor = 1 / f
        e["boot_jac"] = max(e["boot_jac"], _err(o[F["boot_jac"]], want) / float(max(abs(v) for v in want)))
        assert abs(float(back[0]) - x) <= 1e-13 * max(r, 1) and abs(float(back[1]) - y) <= 1e-13 * max(r, 1)   # (the restatement inverts itself)
    return e


@functools.lru_cache(maxsize=None)
def _evaluated(name):
    cam5 = cc.CALIBRATIONS[name] if name in cc.CALIBRATIONS else cc.OUT_OF_MODEL
    xy = cc.all_points(cam5)
    o, do = orc.cam_eval(cam5, W, H, xy)
    g, dg = capi.eval_camera(cam5, W, H, xy, on_host=True)
    return cam5, xy, o, do, g, dg


# ---- a, c ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_and_host_form_against_mpmath():
    """3a and 3c: the smooth radii of cam_cases (0.0101 and 0.02 absolute, 0.1 .. 3.0 x largest_radius, seven angles each) at every
    calibration.  The worst errors are printed; the bound of each quantity is MARGIN x the measured constant."""
    worst_o = dict(im=0.0, derivs=0.0, unproject=0.0, boot_out=0.0, boot_jac=0.0)
    worst_g = dict(worst_o)
    for name in cc.NAMES:
        cam5 = cc.CALIBRATIONS[name]
        xy, _mult = cc.smooth_points(cam5)
        o, _do = orc.cam_eval(cam5, W, H, xy)
        g, _dg = capi.eval_camera(cam5, W, H, xy, on_host=True)
        eo, eg = _errors(cam5, o, xy), _errors(cam5, g, xy)
        print(name, "oracle", {k: "%.3g" % v for k, v in eo.items()}, "host form", {k: "%.3g" % v for k, v in eg.items()})
        for k in worst_o:
            worst_o[k], worst_g[k] = max(worst_o[k], eo[k]), max(worst_g[k], eg[k])
    print("worst, oracle:", worst_o, "host form:", worst_g)
    bound = dict(im=MEASURED_IM, derivs=MEASURED_DERIVS, unproject=MEASURED_UNPROJECT, boot_out=MEASURED_BOOT_OUT, boot_jac=MEASURED_BOOT_JAC)
    for k, b in bound.items():
        assert worst_o[k] <= MARGIN * b, ("oracle", k, worst_o[k], b)
        assert worst_g[k] <= MARGIN * b, ("host form", k, worst_g[k], b)


@pytest.mark.parametrize("name", cc.NAMES + ("out of model",))
def test_host_form_is_the_oracle_bit_for_bit(name):
    """every point of 3a-3c and the derived values; at the out-of-model calibration (radius x w passes pi / 2) as arithmetic only"""
    assert capi.CAM_EVAL_FIELDS == orc.CAM_EVAL_FIELDS and capi.CAM_DERIVED == orc.CAM_DERIVED       # one layout, stated on both sides
    cam5, xy, o, do, g, dg = _evaluated(name)
    assert np.array_equal(o, g, equal_nan=True), np.flatnonzero((o != g).any(1))
    assert np.array_equal(do, dg)
    if name == "out of model":
        assert dg[orc.CAM_DERIVED.index("largest_radius")] < 0
        return
    for (x, y), row in zip(xy[::5], o[::5]):                          # the control: the entry points the suite already holds agree
        im, d, inv, lr = orc.cam_project(cam5, W, H, x, y)
        assert np.array_equal(im, row[F["im"]]) and np.array_equal(d.ravel(), row[F["derivs"]]) and inv == row[F["invalid"]] and lr == do[2]
        assert np.array_equal(orc.cam_unproject(cam5, W, H, im[0], im[1]), row[F["unproject"]])


# ---- b ------------------------------------------------------------------------------------------------------------------------------
def _vatan(x):
    return capi.eval_transcendental("atan", [x], on_host=True)[0]


def _vtan(x):
    return capi.eval_transcendental("tan", [x], on_host=True)[0]


@pytest.mark.parametrize("name", cc.NAMES)
def test_switch_zones_follow_the_reference_rule_exactly(name):
    """jni/ATANCamera.h:136-142 (factor = 1 below r = 0.001), jni/ATANCamera.cc:198-231 (no distortion derivative below r = 0.01 or
    without distortion), :149-164 (f = 1 up to dist_r = 0.01), :133-145 (invalid beyond 1.5 x largest_radius), on the host form."""
    cam5, xy, _o, _do, g, dg = _evaluated(name)
    two_tan, winv, lr, max_r, _opd = dg
    fx, fy, cx, cy = W * cam5[0], H * cam5[1], W * cam5[2] - 0.5, H * cam5[3] - 0.5
    w = cam5[4]
    assert max_r == 1.5 * lr
    seen = dict(factor_one=0, factor_atan=0, diag=0, full=0, f_one=0, f_tan=0, valid=0, invalid=0)
    for (x, y), o in zip(xy, g):
        r = np.sqrt(x * x + y * y)
        assert o[F["r"]] == r
        if r < 0.001 or w == 0.0:
            fac = 1.0; seen["factor_one"] += 1
        else:
            fac = winv * _vatan(r * two_tan) / r; seen["factor_atan"] += 1
        assert o[F["factor"]] == fac, (name, r)
        assert o[0] == cx + fx * (x * fac) and o[1] == cy + fy * (y * fac), (name, r)
        d = o[F["derivs"]]
        if r * (0.0 if w == 0.0 else 1.0) < 0.01:
            assert d[0] == fx * fac and d[3] == fy * fac and d[1] == 0 and d[2] == 0, (name, r, d); seen["diag"] += 1
        else:
            seen["full"] += 1
            if x != 0 and y != 0 and abs(w) >= 0.01:                     # (of relative size w^2 r^2: below the rounding at tiny_w)
                assert d[1] != 0 and d[2] != 0, (name, r, d)
        assert o[F["invalid"]] == (1.0 if r > max_r else 0.0), (name, r)
        seen["invalid" if r > max_r else "valid"] += 1
        dx, dy = (o[0] - cx) * (1.0 / fx), (o[1] - cy) * (1.0 / fy)
        dist = np.sqrt(dx * dx + dy * dy)
        if dist > 0.01:
            rr = dist if w == 0.0 else _vtan(dist * w) * (1.0 / two_tan)
            f = rr / dist; seen["f_tan"] += 1
        else:
            f = 1.0; seen["f_one"] += 1
        assert o[9] == dx * f and o[10] == dy * f and o[11] == o[9] and o[12] == o[10], (name, r, dist)
        if dist <= 0.01:
            assert o[9] == dx and o[10] == dy
    assert all(v > 0 for k, v in seen.items() if not (w == 0.0 and k in ("factor_atan", "full"))), seen
    # the radii on both sides of each switch are in the set, exactly
    _zxy, zr = cc.zone_points()
    assert {0.000999, 0.001, 0.00999, 0.01} <= set(zr.tolist())
    _sxy, mult = cc.smooth_points(cam5)
    sm = g[:len(mult)]
    assert (sm[mult <= 1.4999, 4] == 0).all() and (sm[mult >= 1.5001, 4] == 1).all() and (mult == 1.4999).any() and (mult == 1.5001).any()
    # dist_r either side of 0.01 (cam_cases.unproject_zone_points)
    dxy = (g[:, :2] - np.array([cx, cy])) * np.array([1.0 / fx, 1.0 / fy])
    dist = np.sqrt(dxy[:, 0] * dxy[:, 0] + dxy[:, 1] * dxy[:, 1])
    near = (dist > 0.00998) & (dist < 0.01002)
    assert (dist[near] <= 0.01).any() and (dist[near] > 0.01).any(), dist[near]


def test_pinhole_takes_no_distortion_term_anywhere():
    """w == 0: factor 1 and a diagonal derivative at every radius (distortion_enabled = 0), UnProject the plain division"""
    cam5, xy, _o, _do, g, dg = _evaluated("pinhole")
    fx, fy = W * cam5[0], H * cam5[1]
    assert dg[0] == 0 and dg[1] == 0
    assert (g[:, 3] == 1.0).all()
    assert (g[:, 5] == fx).all() and (g[:, 8] == fy).all() and (g[:, 6] == 0).all() and (g[:, 7] == 0).all()
    assert (g[:, 13] == fx).all() and (g[:, 16] == fy).all() and (g[:, 14] == 0).all() and (g[:, 15] == 0).all()


def test_derived_values():
    cam5 = cc.CALIBRATIONS["pinhole"]
    d = cc.derived(cam5)
    v0, v1 = max(cam5[2], 1.0 - cam5[2]) / cam5[0], max(cam5[3], 1.0 - cam5[3]) / cam5[1]
    assert d["largest_radius"] == np.sqrt(v0 * v0 + v1 * v1)
    t = cc.derived(cc.CALIBRATIONS["tiny_w"])
    assert abs(d["one_pixel_dist"] - t["one_pixel_dist"]) <= 1e-6 * d["one_pixel_dist"]      # they differ by terms of order w^2
    assert abs(d["largest_radius"] - t["largest_radius"]) <= 1e-6 * d["largest_radius"]
    # cam_fill's max(c, 1 - c): pincushion takes the 1 - c side in x and the c side in y, the others' principal points differ again
    p = cc.CALIBRATIONS["pincushion"]
    assert 1 - p[2] > p[2] and p[3] > 1 - p[3]
    sides = set()
    for name in cc.NAMES:                                            # largest_radius against the restatement, whichever side is picked
        p = cc.CALIBRATIONS[name]
        sides.add((p[2] > 1 - p[2], p[3] > 1 - p[3]))
        hp = HpCamera(p, W, H)
        rr = mpmath.sqrt((mpmath.mpf(max(p[2], 1 - p[2])) / mpmath.mpf(p[0])) ** 2 + (mpmath.mpf(max(p[3], 1 - p[3])) / mpmath.mpf(p[1])) ** 2)
        want = rr if hp.w == 0 else mpmath.tan(rr * hp.w) / hp.k
        assert abs(float(want) - cc.derived(p)["largest_radius"]) < 1e-14, name
    assert len(sides) >= 3, sides                                    # (c, 1 - c), (1 - c, c) and one more are all taken
    for name in cc.NAMES:                                            # the host form derives what the oracle derives
        assert np.array_equal(capi.eval_camera(cc.CALIBRATIONS[name], W, H, np.zeros((0, 2)), on_host=True)[1], orc.cam_eval(cc.CALIBRATIONS[name], W, H, np.zeros((0, 2)))[1])
    assert cc.derived(cc.OUT_OF_MODEL)["largest_radius"] < 0


# ---- d ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_edge_points_take_every_exit(name):
    """a condition of the case module: for the pose the tracker projects with in frame 0, every calibration's scenes hold a point in
    each exit, counted with the oracle's camera and pose transform"""
    cam5 = cc.CALIBRATIONS[name]
    for seed in cc.SEEDS:
        f, m, _frames, index = cc.scene(name, seed)
        assert set(index) == set(cc.EXITS)
        for ename, i in index.items():
            kind, (z, r, im) = cc.classify(cam5, W, H, f.pose(-1), m["points"][i]["pos"])
            assert cc.takes_exit(kind, ename), (name, seed, ename, kind, z, r, im)
            if ename == "z above 0.001":
                assert 0.001 <= z < 0.001 * (1 + 1e-5)
            if ename == "z below 0.001":
                assert 0.001 * (1 - 1e-5) < z < 0.001
            if ename in ("beyond largest radius", "within largest radius"):
                lr = cc.derived(cam5)["largest_radius"]
                assert abs(r / lr - 1) < 1e-8 and (r > lr) == (ename == "beyond largest radius")
            if ename.startswith("outside") or ename.startswith("inside"):
                edge = {"left": im[0], "right": im[0] - W, "top": im[1], "bottom": im[1] - H}[ename.split()[1]]
                assert abs(edge) < 0.02, (name, ename, im)
            if ename == "r < 0.001":
                assert r < 0.001
            if ename == "r < 0.01":
                assert 0.001 <= r < 0.01


@functools.lru_cache(maxsize=None)
def _oracle_run(name, seed, patch):
    f, m, frames, index = cc.scene(name, seed)
    vp = capi.default_params(W, H, 1, patch_size=patch, grow_map=3, cam=cc.CALIBRATIONS[name])
    o = make_oracle(vp, m, f.pose(-1))
    rec = dict(n0=o.state().n_points, quality=[], kf=[], err=[], levels=set(), edge_searched=set())
    for t in range(cc.N_FRAMES):
        o.track_frame(frames[t])
        s, tr = o.state(), o.point_tracks()
        rec["quality"].append(s.quality); rec["kf"].append(s.kf_added); rec["err"].append(pose_err(s.pose, f.pose(t)))
        fnd = (tr["level"] >= 0) & (tr["found"] == 1)
        rec["levels"] |= set(tr["level"][fnd].tolist())
        if t == 0:
            rec["edge_searched"] = {e for e, i in index.items() if tr["searched"][i] == 1}
    rec["n1"] = o.state().n_points
    o.close()
    return rec


@pytest.mark.parametrize("patch", (8, 11))
@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_tracks_and_grows_the_map_at_every_calibration(name, patch):
    searched = set()
    for seed in cc.SEEDS:
        rec = _oracle_run(name, seed, patch)
        assert rec["quality"] == [2] * cc.N_FRAMES, (name, seed, rec["quality"])
        assert rec["kf"][0] == 1 and rec["n1"] > rec["n0"], (name, seed, rec["kf"], rec["n0"], rec["n1"])
        assert max(rec["err"]) < 5e-3, (name, seed, rec["err"])
        assert len(rec["levels"]) >= 3, (name, seed, rec["levels"])          # the search level is not degenerate
        searched |= rec["edge_searched"]
    # the edge points in the image are searched like any other (in one of the two scenes at least), the others never
    assert {"inside left", "inside right", "inside top", "inside bottom", "r < 0.001", "r < 0.01"} <= searched, (name, searched)
    assert not searched & {"behind", "z below 0.001", "beyond largest radius", "outside left", "outside right", "outside top", "outside bottom"}


def _in_both_builds(expr):
    """the value of the cam_cases expression in the oracle's two builds (the product's transcendentals, glibc's), each in a child process"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, json, warnings\nwarnings.simplefilter('ignore')\nsys.path[:0] = [%r, %r]\nimport cam_cases\n"
            "print(json.dumps(cam_cases.%s))\n") % (root, os.path.join(root, "tests"), expr)
    return [json.loads(subprocess.check_output([sys.executable, "-c", code], env=dict(os.environ, ORC_ORACLE_VARIANT=v), text=True).strip().splitlines()[-1])
            for v in ("", "stdlibm")]


def test_bootstrap_scene_takes_no_borderline_decision():
    """The condition behind cam_cases.BOOT_SEED: at every calibration the oracle's two builds make the same map of the bootstrap scene --
    the same number of LM trials over the adjustments that follow InitFromStereo, the same stereo points kept -- and the scene is big enough."""
    a, b = _in_both_builds("boot_records()")
    for name in cc.NAMES:
        n, ok, stereo, trials, kept = a[name]
        assert ok == 1 and n > 100 and stereo > 100 and len(kept) > 60, (name, n, ok, stereo, len(kept))
        assert a[name] == b[name], (name, a[name][:4], b[name][:4])


def test_frame0_adjustment_does_not_amplify_last_bit_differences():
    """The condition behind cam_cases.SEEDS: after frame 0 the oracle's two builds (the product's transcendentals, glibc's) agree on the
    adjusted map to a tenth of the 1e-7 bar of the re-synchronised GPU test, at every calibration with distortion (the pinhole calls no
    transcendental: its scenes are tiny_w's to 1e-7 of a pixel)."""
    both = _in_both_builds("frame0_maps()")
    runs = {"": both[0], "stdlibm": both[1]}
    worst = {}
    for key, (trials, pos, poses) in runs[""].items():
        t2, pos2, poses2 = runs["stdlibm"][key]
        assert trials == t2 and len(pos) == len(pos2) and len(poses) == len(poses2), key
        worst[key] = max(float(np.abs(np.array(pos) - np.array(pos2)).max()), float(np.abs(np.array(poses) - np.array(poses2)).max()))
    print({k: "%.1e" % v for k, v in worst.items()})
    assert max(worst.values()) <= cc.MAX_LIBM_SPREAD, {k: v for k, v in worst.items() if v > cc.MAX_LIBM_SPREAD}
    assert max(v for k, v in worst.items() if not k.startswith("pinhole")) > 0          # the two builds do differ
