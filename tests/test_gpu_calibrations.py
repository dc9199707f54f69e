"""GPU parity at camera calibrations other than the default (tests/cam_cases.py): a pinhole (every w == 0 branch), w = 1e-7, PTAM's
shipped default, a wide barrel lens, a pincushion lens with the principal point far off centre -- and the reference's calibration as the
control.  Everything is 320x240 or smaller.  vslam_params carries one calibration, so a system serves one calibration and its two
scenes are the streams of it; the six systems are built one after another.

1. vslam_eval_camera on the device == its host form == the oracle, bit for bit (the rule of vslam_eval_transcendental).
2. tracker, map growth and bundle adjustment, re-synchronised after every frame: bit-exact tracking, the map within 1e-7, the new
   keyframe's measurement table exact.
3. free-running with ba_sum_order = 1: the tracker and the whole map bit-exact in every frame.
4. the found points of those runs span at least three pyramid levels (level, sub-pixel flag and position are compared exactly in 2, 3).
5. the SmallBlurryImage rotation prior.
6. the bootstrap: the homography stage from integer pixels, InitFromStereo on host matches.
7. the stand-alone bundle adjustment in both summation modes, the fast one against the extended-precision first trial.

The scenes hold cam_cases' edge points: map points on both sides of every exit of TrackerData::Project (CPU conditions:
tests/test_cam_cases.py)."""
import numpy as np
import pytest

import ba_hp
import boot_cases as bc
import cam_cases as cc
import oracle.binding as orc
from ba_scene import ba_scene
from helpers import assert_map_close, assert_map_exact, assert_tracker_exact, make_oracle, pose_err, resync
from test_gpu_bundle import check_exact, load
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu
W, H = cc.W, cc.H
B = orc.BootMath


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES + ("out of model",))
def test_eval_camera_device_is_host_form_and_oracle(name):
    cam5 = cc.CALIBRATIONS[name] if name in cc.CALIBRATIONS else cc.OUT_OF_MODEL
    xy = cc.all_points(cam5)
    assert len(xy) > 64                                                   # more than one pass of the 64 lanes
    dev, dd = capi.eval_camera(cam5, W, H, xy)
    host, dh = capi.eval_camera(cam5, W, H, xy, on_host=True)
    o, do = orc.cam_eval(cam5, W, H, xy)
    for a, b, what in ((dev, host, "host form"), (dev, o, "oracle")):
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), (name, what, np.argwhere(~same)[:8].tolist())
    assert np.array_equal(dd, dh) and np.array_equal(dd, do)


# ---- 2, 3, 4 ------------------------------------------------------------------------------------------------------------------------
def run_calibration(name, patch, mode, **pkw):
    """One system at the calibration `name`, one stream per seed of cam_cases.SEEDS, against one oracle each (test_gpu_tracking.py's
    run_streams on cam_cases' scenes).  -> the pyramid levels of the found points, per stream"""
    cam5 = cc.CALIBRATIONS[name]
    sc = [cc.scene(name, sd) for sd in cc.SEEDS]
    S = len(sc)
    kw = dict(patch_size=patch, grow_map=3, cam=cam5, **pkw)
    g = capi.System(capi.default_params(W, H, S, **kw))
    os_ = []
    for s, (f, m, _fr, _ix) in enumerate(sc):
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
        os_.append(make_oracle(capi.default_params(W, H, 1, **kw), m, f.pose(-1)))
    levels = [set() for _ in range(S)]
    for t in range(cc.N_FRAMES):
        g.track_frame(np.stack([x[2][t] for x in sc]))
        for s in range(S):
            o = os_[s]
            o.track_frame(sc[s][2][t])
            tag = "%s P%d seed %d frame %d" % (name, patch, cc.SEEDS[s], t)
            assert_tracker_exact(o, g, s, tag)
            tg = g.point_tracks(s)
            levels[s] |= set(tg["level"][(tg["level"] >= 0) & (tg["found"] == 1)].tolist())
            if t == 0:
                assert o.state().kf_added == 1, tag
            if o.state().kf_added:
                if mode == "resync":
                    assert_map_close(o, g, s, tag, 1e-7)
                else:
                    assert_map_exact(o, g, s, tag)
                k_new = o.state().n_keyframes - 1
                mo, mg = o.keyframe_meas(k_new), g.keyframe_meas(s, k_new)
                assert np.array_equal(mo["pt"], mg["pt"]) and np.array_equal(mo["source"], mg["source"]) and np.array_equal(mo["level"], mg["level"]), tag
                assert np.array_equal(mo["root"], mg["root"]), (tag, np.abs(mo["root"] - mg["root"]).max())
            if mode == "resync":
                resync(o, g, s)
            assert g.state(s).quality == 2, tag
            assert pose_err(g.state(s).pose, sc[s][0].pose(t)) < 5e-3, tag      # and both follow the ground truth
    for s in range(S):
        assert g.state(s).n_keyframes > len(sc[s][1]["keyframes"]) and g.state(s).n_points > len(sc[s][1]["points"]), (name, s)
        os_[s].close()
    g.close()
    return levels


@pytest.mark.parametrize("patch", (8, 11))
@pytest.mark.parametrize("name", cc.NAMES)
def test_resynchronised_tracking_growth_and_adjustment(name, patch):
    levels = run_calibration(name, patch, "resync")
    assert all(len(lv) >= 3 for lv in levels), (name, levels)             # 4: the search level does not degenerate at this calibration


@pytest.mark.parametrize("patch", (8, 11))
@pytest.mark.parametrize("name", cc.NAMES)
def test_free_running_reference_order_is_bit_exact(name, patch):
    levels = run_calibration(name, patch, "free_exact", ba_sum_order=1)
    assert all(len(lv) >= 3 for lv in levels), (name, levels)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_small_blurry_image_rotation_prior(name):
    """use_sbi = 1: the rotation prior (its derivatives go through the camera's un-projection and projection derivatives,
    jni/SmallBlurryImage.cc:189-227) and its score == the oracle's, and the tracking that starts from it"""
    cam5 = cc.CALIBRATIONS[name]
    sc = [cc.scene(name, sd) for sd in cc.SEEDS]
    kw = dict(patch_size=8, min_frames_between_kf=1000, use_sbi=1, cam=cam5)
    g = capi.System(capi.default_params(W, H, len(sc), **kw))
    os_ = []
    for s, (f, m, _fr, _ix) in enumerate(sc):
        g.load_map(s, m); g.set_pose(s, f.pose(-1))
        os_.append(make_oracle(capi.default_params(W, H, 1, **kw), m, f.pose(-1)))
    prev = [None] * len(sc)
    moved = False
    for t in range(3):
        g.track_frame(np.stack([x[2][t] for x in sc]))
        for s, o in enumerate(os_):
            o.track_frame(sc[s][2][t])
            l3 = orc.make_keyframe_lite(sc[s][2][t])[3][0]
            _small, _tmpl, rot, score = g.read_sbi(s)
            wrot, wscore = orc.sbi_rotation(l3, prev[s] if prev[s] is not None else l3, cam5)
            assert np.array_equal(rot, wrot) and score == wscore, (name, s, t, rot, wrot, score, wscore)
            moved |= bool(np.any(np.asarray(wrot) != 0))
            prev[s] = l3
            assert_tracker_exact(o, g, s, "%s sbi seed %d frame %d" % (name, cc.SEEDS[s], t))
    assert moved                                                          # the prior is not the identity throughout
    for o in os_:
        o.close()
    g.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_homography_stage_from_integer_pixels(name):
    """the kernel's own UnProject + GetProjectionDerivs (unproject_with_derivs) on integer pixel pairs: the device's Match array == the
    oracle's, the rest of the record == the host build fed with those matches, the pose within the bar of the oracle"""
    cam5 = cc.CALIBRATIONS[name]
    g = capi.System(capi.default_params(W, H, 1, grow_map=3, bootstrap=1, max_points=512, cam=cam5))
    px = bc.pixel_scene(41, 220, list(cam5), W, H)
    assert len(px) > 150, (name, len(px))
    dev = g.probe_homography_init(0, 5, matches_xyxy=px)
    m8 = orc.boot_matches(list(cam5), W, H, px)
    got = bc.arr(dev.matches)[:8 * len(px)].reshape(-1, 8)
    assert np.array_equal(got.view(np.uint64), m8.view(np.uint64)), (name, np.abs(got - m8).max())
    if cam5[4] != 0.0:
        assert np.abs(m8[:, 5]).max() > 0                                 # the radial model's derivatives are not diagonal
    else:
        assert not m8[:, 5].any() and not m8[:, 6].any()
    host = B.homography_pipeline(m8, 5, 5.0, g.params.wiggle_scale)
    bc.assert_same_bits(dev, host, name)
    assert dev.ok == 1 and dev.n_inliers >= len(px) - 12, (name, dev.n_inliers, len(px))
    bc.check_homography_against_oracle(dev, m8, 5, name)
    g.close()


def _mat(p):
    p = np.array(p[:])
    m = np.eye(4)
    m[:3, :3] = p[:9].reshape(3, 3); m[:3, 3] = p[9:]
    return m


@pytest.mark.parametrize("name", cc.NAMES)
def test_init_from_stereo_on_host_matches(name):
    """k_boot_points (triangulation through the camera's un-projection, jni/MapMaker.cc:204-376) by one vslam_init_from_stereo on the
    oracle's own trails, as test_gpu_bootstrap.py's test_init_from_stereo_with_host_keyframes_and_matches does at the default: integers
    exactly -- inlier count, which matches become points and which of them the second keyframe still measures, their sub-pixel positions
    -- and the map in alignment-invariant quantities to the tolerance of the two sides' independent homography mathematics.  The scene
    (cam_cases.BOOT_SEED) is one whose outlier decisions are not borderline: tests/test_cam_cases.py holds the condition."""
    cam5 = cc.CALIBRATIONS[name]
    first, last, matches = cc.boot_scene(name)
    assert len(matches) > 100, (name, len(matches))
    g = capi.System(capi.default_params(W, H, 1, bootstrap=1, patch_size=8, grow_map=3, cam=cam5))
    ok_g, pose_g = g.init_from_stereo(first, last, matches)
    o, ok_o = cc.boot_oracle(name)
    assert ok_g and ok_o, name
    io, ig = o.init_info(), g.init_info(0)
    assert (io["stage"], io["init_ok"], io["map_good"], io["hom_inliers"], io["stereo_points"]) == (ig["stage"], ig["init_ok"], ig["map_good"], ig["hom_inliers"], ig["stereo_points"]), (name, io, ig)
    assert io["stereo_points"] > 100, (name, io)
    mo, mg = o.keyframe_meas(1), g.keyframe_meas(0, 1)
    tr_o, tr_g = mo["source"] == 3, mg["source"] == 3
    rel_o = _mat(o.keyframe_pose(1)) @ np.linalg.inv(_mat(o.keyframe_pose(0)))
    rel_g = _mat(g.keyframe_pose(0, 1)) @ np.linalg.inv(_mat(g.keyframe_pose(0, 0)))
    bo, bg = np.linalg.norm(rel_o[:3, 3]), np.linalg.norm(rel_g[:3, 3])
    d_rot, d_t = np.abs(rel_o[:3, :3] - rel_g[:3, :3]).max(), np.abs(rel_o[:3, 3] / bo - rel_g[:3, 3] / bg).max()
    print(name, "trails %d, stereo points %d, kept by one side only %d, rotation %.3g, translation / baseline %.3g, LM trials %d / %d"
          % (len(matches), io["stereo_points"], len(np.setxor1d(mo["pt"][tr_o], mg["pt"][tr_g])), d_rot, d_t, o.state().n_ba_trials, g.state(0).n_ba_trials))
    assert np.array_equal(mo["pt"][tr_o], mg["pt"][tr_g]) and np.array_equal(mo["root"][tr_o], mg["root"][tr_g]), name
    assert d_rot < 5e-3 and d_t < 2e-2, (name, d_rot, d_t)
    assert pose_err(pose_g, g.state(0).pose) == 0.0
    o.close()
    g.close()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("pinhole", "wide", "pincushion"))
def test_stand_alone_bundle_both_summation_modes(name):
    """The scene of test_gpu_ba_step_paths.py's first_step_outliers (4 cameras, 2 fixed, 40 points) measured through this calibration.
    ba_sum_order = 1: the oracle's bits.  ba_sum_order = 0: the first accepted trial no further from the extended-precision trial
    (tests/ba_hp.py) than its bar allows -- max|gpu - hp| <= 8 max|oracle - hp| + 16 eps max|hp| -- where the derivative's off-diagonal
    terms are large (or, at the pinhole, absent)."""
    cam5 = cc.CALIBRATIONS[name]
    sc = ba_scene(n_cams=4, n_pts=40, n_fixed=2, seed=0, cam=cam5)
    assert len(sc["meas"]) >= 100, (name, len(sc["meas"]))
    cap = (len(sc["cams_init"]), len(sc["pts_init"]), len(sc["meas"]))
    # reference order: several iterations, the oracle's bits
    g = capi.Bundle(capi.default_params(640, 480, 1, ba_max_iterations=5, ba_sum_order=1, cam=cam5), 1, *cap)
    load(g, sc)
    g.compute()
    o = orc.OracleBundle(cam5, 640, 480, max_iterations=5)
    load(o, sc)
    check_exact(o, g, 0)
    assert g.result(0)["accepted"] > 0
    o.close(); g.close()
    # fast sums: one trial against the extended-precision solve
    hp = ba_hp.first_trial(cam5, 640, 480, sc["cams_init"], sc["fixed"], sc["pts_init"], sc["meas"])
    assert hp["new_err"] < hp["cur_err"]
    g = capi.Bundle(capi.default_params(640, 480, 1, ba_max_iterations=1, ba_sum_order=0, cam=cam5), 1, *cap)
    load(g, sc)
    g.compute()
    o = orc.OracleBundle(cam5, 640, 480, max_iterations=1)
    load(o, sc)
    assert o.compute() == 1 and g.result(0)["accepted"] == 1 and g.result(0)["trials"] == 1
    assert g.result(0)["sigma2"] == o.stats()[0]
    for got, want, ref in ((g.cameras(0), hp["cams"], o.cameras()), (g.points(0), hp["pts"], o.points())):
        dg, allowed, do = ba_hp.bar(got, ref, want)
        print(name, "gpu - hp %.3g, allowed %.3g, oracle - hp %.3g" % (dg, allowed, do))
        assert dg <= allowed, (name, dg, allowed, do)
    assert np.array_equal(o.outlier_meas(), g.outlier_meas(0))
    o.close(); g.close()
