"""CPU: the cases of tests/stereo_cases.py reach what they are built for -- asserted on the oracle alone, in shared-stage mode (the mode
tests/test_gpu_init_from_stereo.py compares the device with).  Nothing comes from the device; no case may be left out: a named condition
that is not reached fails here."""
import numpy as np
import pytest

import oracle.binding as orc
import stereo_cases as sc


def _mat(p):
    p = np.array(p[:])
    m = np.eye(4)
    m[:3, :3] = p[:9].reshape(3, 3); m[:3, 3] = p[9:]
    return m


def _run(case, shared=True):
    o, ok = sc.run(case, shared)
    return o, ok, o.boot_log(), o.boot_diag(), o.init_info()


def _by_name(patch):
    return {c.name: c for c in sc.one_stream_cases(patch)}


@pytest.mark.parametrize("patch", sc.PATCHES)
def test_a_residues(patch):
    """4k .. 4k + 3 matches, each match logged once; the lone last match fails behind a round whose first wavefront made a point"""
    cases = [c for c in sc.residue_cases(patch)]
    assert sorted(c.want["n"] % sc.WAVES for c in cases if "lone_failure" not in c.want) == list(range(sc.WAVES))
    for c in cases:
        o, ok, log, diag, info = _run(c)
        assert ok and len(c.matches) == c.want["n"] == len(log["code"]) and info["trails"] == c.want["n"], c.name
        assert info["stereo_points"] == int((log["code"] == sc.CODE_POINT).sum()) >= 30, c.name
        if c.want.get("lone_failure"):
            n = len(c.matches)
            assert n % sc.WAVES == 1 and log["code"][n - 1] == sc.CODE_BORDER and log["code"][n - 1 - sc.WAVES] == sc.CODE_POINT, (c.name, log["code"][-6:])
        o.close()


@pytest.mark.parametrize("patch", sc.PATCHES)
def test_b_template_border(patch):
    """half from a border: code 1; half + 1 and half + 2: the template is made (some go on to a point); rows at the start, in the middle,
    at the end of a list whose last round holds one match"""
    c = sc.border_case(patch)
    o, ok, log, diag, info = _run(c)
    rows, dist = np.array(c.want["border_rows"]), np.array(c.want["border_dist"])
    assert ok and len(rows) == 12 and rows[0] == 0 and rows[-1] == len(c.matches) - 1 and len(c.matches) % sc.WAVES == 1
    assert len(c.matches) // 3 < rows[4] < 2 * len(c.matches) // 3
    m, h = c.matches[rows], sc.half(patch)
    edge = np.minimum(np.minimum(m[:, 0], c.w - 1 - m[:, 0]), np.minimum(m[:, 1], c.h - 1 - m[:, 1]))
    assert np.array_equal(edge, h + dist) and sorted(set(dist)) == [0, 1, 2]
    code = log["code"][rows]
    assert np.all(code[dist == 0] == sc.CODE_BORDER) and np.all(code[dist > 0] != sc.CODE_BORDER), code
    assert (log["code"] == sc.CODE_BORDER).sum() == 4                  # one per border, nowhere else
    assert (code[dist == 1] == sc.CODE_POINT).any() and (code[dist == 2] == sc.CODE_POINT).any(), code
    o.close()


@pytest.mark.parametrize("patch", sc.PATCHES)
def test_c_subpixel_failures(patch):
    """flat image: all ten iterations run and do not converge; sub-pixel border: the first iteration leaves, the position is the start"""
    flat, border = sc.subpix_cases(patch)
    o, ok, log, diag, info = _run(flat)
    rows = np.array(flat.want["flat_rows"])
    assert ok and len(rows) >= 3
    assert np.all(log["code"][rows] == sc.CODE_SUBPIX) and np.all(log["its"][rows] == 10), (log["code"][rows], log["its"][rows])
    assert np.all(np.abs(log["sub"][rows] - flat.matches[rows, 2:]).max(axis=1) > 0)          # they moved, and stayed inside the image
    o.close()
    o, ok, log, diag, info = _run(border)
    rows = np.array(border.want["edge_rows"])
    assert ok and len(rows) == 4
    assert np.all(log["code"][rows] == sc.CODE_SUBPIX) and np.all(log["its"][rows] == 1), (log["code"][rows], log["its"][rows])
    assert np.array_equal(log["sub"][rows], border.matches[rows, 2:].astype(np.float64))
    b = sc.half(patch) + 1                                             # ... with a good template: the first positions keep the border
    m = border.matches[rows]
    assert np.all((m[:, 0] >= b) & (m[:, 1] >= b) & (m[:, 0] < border.w - b) & (m[:, 1] < border.h - b))
    assert np.all((m[:, 2] < b) | (m[:, 3] < b) | (m[:, 2] >= border.w - b) | (m[:, 3] >= border.h - b))
    o.close()


@pytest.mark.parametrize("patch", sc.PATCHES)
def test_d_behind_the_camera(patch):
    """a displacement of the fixed set puts the pasted block's match behind the camera after a converged sub-pixel alignment"""
    c = sc.behind_case(patch)
    assert c is not None, "no displacement of %r gives a point behind the camera" % (sc.DISPLACEMENTS,)
    o, ok, log, diag, info = _run(c)
    r = c.want["behind_row"]
    assert ok and log["code"][r] == sc.CODE_BEHIND and 1 <= log["its"][r] <= 10 and (log["code"] == sc.CODE_POINT).sum() > 50
    o.close()
    if patch == 8:                                                     # and a whole set of them: the mirrored decomposition at 320 x 240
        c = _by_name(patch)["D: 320 x 240, the mirrored decomposition"]
        o, ok, log, diag, info = _run(c)
        assert ok and (log["code"] == sc.CODE_BEHIND).sum() > 20 and (log["code"] == sc.CODE_POINT).sum() > 100
        assert o.converged() == (0, 0)                                 # the bounded fifty adjustments end unconverged
        o.close()


@pytest.mark.parametrize("patch", sc.PATCHES)
def test_e_both_false_exits(patch):
    """0 and 3 matches: HomographyInit has nothing to fit, no inlier count.  9 matches: the direct fit (no MLESAC) goes through -- nine
    is too few for the trials, not for the call.  Zero baseline: the host pipeline's ok = 0 with every match an inlier; the oracle's own
    mathematics leaves by HomographyInit's `return false` (the three singular values do not come out distinct), not by mag == 0."""
    cases = {c.name: c for c in sc.failing_cases(patch)}
    for n in (0, 3):
        o, ok, log, diag, info = _run(cases["E-i: %d matches" % n])
        assert not ok and diag["exit"] == sc.EXIT_HOST_NOT_OK and len(log["code"]) == 0
        assert info == dict(stage=2, trails=n, init_ok=0, hom_inliers=0, stereo_points=0, map_good=0), info
        assert o.state().n_keyframes == 0 and o.state().n_points == 0
        o.close()
    o, ok, log, diag, info = _run(cases["E-i: 9 matches"])
    assert ok and diag["exit"] == sc.EXIT_NONE and info["hom_inliers"] == 9 and info["stereo_points"] <= 9
    o.close()
    c = cases["E-ii: zero baseline"]
    assert np.array_equal(c.first, c.second) and np.array_equal(c.matches[:, :2], c.matches[:, 2:])
    o, ok, log, diag, info = _run(c)
    assert not ok and diag["exit"] == sc.EXIT_HOST_NOT_OK
    assert info == dict(stage=2, trails=len(c.matches), init_ok=0, hom_inliers=len(c.matches), stereo_points=0, map_good=0), info
    o.close()
    o, ok, log, diag, info = _run(c, shared=False)
    assert not ok and diag["exit"] == sc.EXIT_HOMOGRAPHY, diag
    o.close()
    c = cases["E-ii: zero baseline, a seed at which the rounding decomposes"]
    o, ok, log, diag, info = _run(c)
    assert ok and (log["code"] == sc.CODE_BEHIND).sum() > 10 and o.converged() == (0, 0)
    o.close()


@pytest.mark.parametrize("patch", sc.PATCHES)
def test_f_fewer_than_ten_points(patch):
    """fewer than ten points when CalcPlaneAligner runs: no aligner, the identity is applied, and the refresh of the pixel vectors behind it
    changes bits of every point (the adjustments have moved the points and the second keyframe since the vectors were made)"""
    c = sc.few_points_case(patch)
    o, ok, log, diag, info = _run(c)
    assert ok and len(c.matches) >= 10 and info["hom_inliers"] >= 10
    assert (log["code"] == sc.CODE_SUBPIX).sum() >= 3
    n = o.state().n_points
    assert 0 < diag["plane_points"] == n < 10 and diag["plane_have"] == 0, diag
    assert diag["pixvec_changed"] == n, diag
    o.close()


@pytest.mark.parametrize("patch", sc.PATCHES)
def test_g_mixed_batch(patch):
    """each stream's oracle ends where its role says, and the two second presses and the first press fall into the same frame"""
    streams = sc.mixed_batch(patch)
    t2 = sc.N_TRAIL_FRAMES - 1
    assert [s[0] for s in streams] == list(sc.G_ROLES) and [t2 in s[2] for s in streams] == [False, True, True, True, False]
    end, at_t2 = {}, {}
    for st in streams:
        role, frames, presses = st[:3]
        o = sc.mixed_oracle(patch, st)
        for t in range(sc.G_FRAMES):
            if t in presses:
                o.press_spacebar()
            o.track_frame(frames[t])
            if t == t2:
                at_t2[role] = (o.init_info(), o.boot_diag())
        end[role] = (o.init_info(), o.state())
        o.close()
    info, s = end["loaded map"]
    assert info["map_good"] == 1 and info["stage"] == 0 and s.quality == 2 and s.n_keyframes >= 8 and sum(s.found) > 100
    info, s = end["second press succeeds"]
    assert at_t2["second press succeeds"][0]["init_ok"] == 1 and info["map_good"] == 1 and s.quality == 2 and sum(s.found) > 50
    info, diag = at_t2["second press fails"]
    assert info["stage"] == 2 and info["init_ok"] == 0 and info["map_good"] == 0 and info["hom_inliers"] == info["trails"] > 100 and diag["exit"] == sc.EXIT_HOST_NOT_OK
    assert end["second press fails"][0] == info and end["second press fails"][1].n_keyframes == 0
    info, _ = at_t2["first press"]
    assert info["stage"] == 1 and info["trails"] > 100 and end["first press"][0]["stage"] == 1 and end["first press"][0]["trails"] >= 10
    info, s = end["never pressed"]
    assert info == dict(stage=0, trails=0, init_ok=0, hom_inliers=0, stereo_points=0, map_good=0) and s.n_keyframes == 0


def test_the_mode_matters_and_agrees_with_the_default_within_the_existing_bars():
    """On the baseline the shared-stage mode and the oracle's own mathematics end at different position bits; and they agree within the bars
    tests/test_gpu_bootstrap.py holds the device to against the default mode, each side in units of its own baseline (no new tolerance: its
    5e-3 on the relative rotation, 2e-2 on the direction of the translation, 1.5 baselines on the stereo points in the first camera's
    frame; with one fixed camera two adjustment paths end at different scales, so its absolute 1e-5 for equal trial counts is not used)."""
    for patch in sc.PATCHES:
        a, _ = sc.run(_by_name(patch)["baseline"], shared=True)
        b, _ = sc.run(_by_name(patch)["baseline"], shared=False)
        n0 = a.init_info()["stereo_points"]
        assert n0 == b.init_info()["stereo_points"] > 100 and not np.array_equal(a.points()["pos"][:n0], b.points()["pos"][:n0])      # the mode matters
        a.close(); b.close()
        # the bars belong to that file's scene (640 x 480, feeder seed 1234, the trails of its twelve frames): at 160 x 120 a pixel is four times
        # the angle, and the depth of a stereo point four times as uncertain
        frames, m = sc.base(patch, (640, 480), 1234)
        c = sc.Case("the scene of test_gpu_bootstrap.py", patch, frames[0], frames[sc.N_TRAIL_FRAMES - 1], m, [], seed=1)
        a, ok_a = sc.run(c, shared=True)
        b, ok_b = sc.run(c, shared=False)
        assert ok_a and ok_b
        ia, ib = a.init_info(), b.init_info()
        assert ia == ib and ia["stereo_points"] > 100, (ia, ib)
        ma, mb = a.keyframe_meas(1), b.keyframe_meas(1)
        ta, tb = ma["source"] == 3, mb["source"] == 3
        assert np.array_equal(ma["pt"][ta], mb["pt"][tb]) and np.array_equal(ma["root"][ta], mb["root"][tb])
        sa, sb = a.state(), b.state()
        assert sa.n_keyframes == sb.n_keyframes == 2
        assert abs(sa.n_points - sb.n_points) <= max(3, sa.n_points // 50), (sa.n_points, sb.n_points)
        n0 = ia["stereo_points"]
        pa, pb = a.points(), b.points()
        rel_a = _mat(a.keyframe_pose(1)) @ np.linalg.inv(_mat(a.keyframe_pose(0)))
        rel_b = _mat(b.keyframe_pose(1)) @ np.linalg.inv(_mat(b.keyframe_pose(0)))
        ba_, bb_ = np.linalg.norm(rel_a[:3, 3]), np.linalg.norm(rel_b[:3, 3])
        dr, dt = np.abs(rel_a[:3, :3] - rel_b[:3, :3]).max(), np.abs(rel_a[:3, 3] / ba_ - rel_b[:3, 3] / bb_).max()
        assert dr < 5e-3 and dt < 2e-2, (patch, dr, dt)
        ca = (_mat(a.keyframe_pose(0)) @ np.c_[pa["pos"][:n0], np.ones(n0)].T).T
        cb = (_mat(b.keyframe_pose(0)) @ np.c_[pb["pos"][:n0], np.ones(n0)].T).T
        d = np.abs(ca[:, :3] / ba_ - cb[:, :3] / bb_).max()
        assert d < 1.5, (patch, d)
        a.close(); b.close()


def test_the_default_mode_is_untouched_by_a_shared_run():
    """the switch is per system and off by default: an oracle that never saw it gives the bits of one that had it switched on and off again"""
    c = _by_name(8)["A: 40 matches"]
    a, _ = sc.run(c, shared=False)
    b = c.oracle(shared=True)
    b.set_shared_stages(False)
    b.init_from_stereo(c.first, c.second, c.matches)
    assert np.array_equal(a.points()["pos"], b.points()["pos"]) and np.array_equal(a.keyframe_pose(1), b.keyframe_pose(1))
    fresh = orc.OracleSystem(orc.params_from_vslam(c.params()))
    fresh.set_boot_seed(c.seed)
    fresh.init_from_stereo(c.first, c.second, c.matches)
    assert np.array_equal(a.points()["pos"], fresh.points()["pos"])
    for o in (a, b, fresh):
        o.close()
