"""GPU: the relocaliser (vslam_params.relocalise; jni/Relocaliser.cc, jni/Tracker.cc:133-139, 163-175, jni/KeyFrame.cc:97-100).

The oracle has no relocaliser, but it has the pieces, and the tests compose them:
* orc.sbi_make / orc.sbi_rotation are SmallBlurryImage::MakeFromKF and ln(SE3fromSE2(IteratePosRelToTarget(target, 6))) + the final
  score on both branches (9 taps for dBlur <= 2, 17 above); tests/reloc_ref.py restates MakeFromKF and the ZMSSD in numpy (pinned to
  the oracle on both branches by tests/test_reloc_ref.py);
* the staged oracle tracker (frame_begin, search_stage, pose_stage, set_pose, set_velocity) runs TrackMap from the relocaliser's pose.

Scene: 320x240 feeder scene, two streams.  Stream 0 gets two real frames, then blank frames until lost_frames == 3, then real frames
again; stream 1 gets real frames throughout and must stay check_and_resync-exact against its own oracle in every frame.

The recovered frame's TrackMap is compared BIT FOR BIT with an oracle that has the same map, coarse_max and coarse_range doubled (what
mbJustRecoveredSoUseCoarse does, oracle/tracker.cpp:312-313), the device's mse3Best as its pose and use_sbi = 0.  Two things about that oracle:
* PatchFinder keeps a point's warped template from frame to frame and re-makes it only when the warp has changed (jni/PatchFinder.cc:79-125),
  so the frames before the loss are part of the state: a FRESH oracle searches with other templates than a tracker that has a history
  (measured on the CPU for this scene: 996 of 997 cached templates differ from fresh ones, 421 against 420 found at level 0).  The
  comparison oracle therefore sees the same frames as stream 0.  It must not get lost, so on the blank frames it runs the stages without
  the frame end and takes pose and velocity from a second oracle that runs them whole (and is == the device on every one of them).
* So that the doubled limits cannot change those earlier frames, both sides run with coarse_min_vel = 0.5: no frame but the recovered
  one has a coarse stage.  On the recovered frame the oracle is given a large velocity AFTER frame_begin (the motion model has run
  with zero effect on the pose that is then set), which is the `bTryCoarse = true` of :313.
Seed 77 and a gap of three blank frames were chosen on the CPU with that composition (relocaliser pose from orc.sbi_rotation at blur 2.0):
the recovered frame ends GOOD (found 420/451 311/354 111/151 28/44, coarse stage used, 2.4e-3 from the ground truth) and the following
frames stay within 1.3e-9 of the oracle that never lost track."""
import numpy as np
import pytest

import reloc_ref
from helpers import POSE_TOL, check_and_resync, make_oracle, make_scene, pose_err
from oracle import binding as orc
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

W, H, SEED, N_FRAMES, N_BLANK = 320, 240, 77, 10, 3
KW = dict(min_frames_between_kf=1000, coarse_min_vel=0.5)       # no keyframe, no bundle adjustment: the map stays as loaded
_scene = {}


def scene():
    if not _scene:
        _scene["s"] = make_scene(W, H, seed=SEED, n_frames=N_FRAMES, per_level=(120, 50, 20, 8))
    return _scene["s"]


def level3(gray):
    return orc.make_keyframe_lite(gray)[3][0]


def pose_mul(a, b):
    Ra, ta, Rb, tb = np.asarray(a[:9]).reshape(3, 3), np.asarray(a[9:12]), np.asarray(b[:9]).reshape(3, 3), np.asarray(b[9:12])
    return np.concatenate([(Ra @ Rb).reshape(-1), Ra @ tb + ta])


def staged(o, gray):
    o.frame_begin(gray); o.search_stage(0); o.pose_stage(0); o.search_stage(1); o.pose_stage(1)


def assess_tracking_quality(st, pose, kf_poses, wiggle_scale):
    """Tracker::AssessTrackingQuality (jni/Tracker.cc:832-878) from the frame's counts"""
    ta, tf = sum(st.attempted), sum(st.found)
    la, lf = st.attempted[2] + st.attempted[3], st.found[2] + st.found[3]
    if tf == 0 or ta == 0:
        return 0
    total = tf / ta
    large = lf / la if la > 10 else total
    q = 2 if total > 0.3 else (0 if large < 0.13 else 1)
    if q == 1:
        centre = lambda p: -np.asarray(p[:9]).reshape(3, 3).T @ np.asarray(p[9:12])
        if min(np.linalg.norm(centre(k) - centre(pose)) for k in kf_poses) > wiggle_scale * 10.0:
            q = 0
    return q


class Lost:
    """Both streams tracked up to the frame after which stream 0 has lost_frames == 3, with the oracles of the module docstring"""

    def __init__(self, blur, **extra):
        self.f, self.m, self.frames = scene()
        f, m = self.f, self.m
        self.vp = capi.default_params(W, H, 2, relocalise=1, reloc_blur=blur, **KW, **extra)
        self.g = g = capi.System(self.vp)
        one = capi.default_params(W, H, 1, **KW, **extra)
        self.o = make_oracle(one, m, f.pose(-1))                     # stream 0's frames, whole: ends lost
        self.o_ok = make_oracle(one, m, f.pose(-1))                  # stream 1
        self.o2 = make_oracle(capi.default_params(W, H, 1, coarse_max=2 * one.coarse_max, coarse_range=2 * one.coarse_range, **KW, **extra), m, f.pose(-1))
        for s in range(2):
            g.load_map(s, m); g.set_pose(s, f.pose(-1))
        self.kf_l3 = [level3(k["image"]) for k in m["keyframes"]]
        blank = np.zeros((H, W), np.uint8)
        self.t = 0
        for t in range(2 + N_BLANK):
            fr = self.frames[t] if t < 2 else blank
            self.step(fr)
            self.o.track_frame(fr)
            if t < 2:
                self.o2.track_frame(fr)
                check_and_resync(self.o, g, 0, "before the loss, frame %d" % t)
            else:
                staged(self.o2, fr)
                so, sg = self.o.state(), g.state(0)
                assert np.array_equal(np.array(self.o2.state().pose[:]), np.array(so.pose[:])), t
                assert (so.quality, so.lost_frames) == (sg.quality, sg.lost_frames) == (0, t - 1), t
                assert np.array_equal(np.array(so.pose[:]), np.array(sg.pose[:])) and np.array_equal(np.array(so.velocity[:]), np.array(sg.velocity[:])), t
                self.o2.set_pose(so.pose[:]); self.o2.set_velocity(so.velocity[:])
            assert g.reloc_info(0)["attempts"] == 0, t                 # not lost for three frames yet when the frame began
        assert g.state(0).lost_frames == 3 and "Attempting recovery" in g.message(0)

    def step(self, fr0):
        """one frame: fr0 to stream 0, the scene's frame to stream 1, which must not notice anything (part c)"""
        t = self.t
        self.g.track_frame(np.stack([fr0, self.frames[t]]))
        self.o_ok.track_frame(self.frames[t])
        check_and_resync(self.o_ok, self.g, 1, "undisturbed stream, frame %d" % t)
        self.t += 1

    def expect_images(self, cur_l3, make):
        """keyframe SBIs, the current frame's template, every ZMSSD and the best index against `make` -> (best, scores)"""
        g = self.g
        kts = []
        for k, l3 in enumerate(self.kf_l3):
            tmpl, jacs = g.keyframe_sbi(0, k)
            assert np.array_equal(tmpl, make(l3)), k
            assert np.array_equal(jacs, reloc_ref.make_jacs(tmpl)), k
            kts.append(tmpl)
        cur, scores = g.reloc_attempt(0)
        assert np.array_equal(cur, make(cur_l3))
        best, want = reloc_ref.score_keyframes(cur, kts)
        assert len(scores) == len(want) and np.array_equal(scores, want), (scores, want)
        ri = g.reloc_info(0)
        assert ri["best"] == best and ri["best_zmssd"] == want[best]
        return best, want

    def oracle_recovered_frame(self, gray, best_pose):
        """TrackMap from the relocaliser's pose with the doubled coarse stage -> the oracle's state"""
        o2 = self.o2
        o2.frame_begin(gray)
        o2.set_pose(best_pose); o2.set_velocity([100.0, 0, 0, 0, 0, 0])
        o2.search_stage(0); o2.pose_stage(0); o2.search_stage(1); o2.pose_stage(1)
        return o2.state()

    def assert_recovered_frame_exact(self, gray, tag):
        """the device's frame after an accepted recovery == the oracle composition, and only AssessTrackingQuality ran at its end"""
        g, o2 = self.g, self.o2
        ri = g.reloc_info(0)
        before = self.before
        so, sg = self.oracle_recovered_frame(gray, ri["best_pose"]), g.state(0)
        assert np.array_equal(np.array(so.pose[:]), np.array(sg.pose[:])), (tag, pose_err(so.pose, sg.pose))
        assert list(so.attempted) == list(sg.attempted) and list(so.found) == list(sg.found), (tag, list(so.attempted), list(sg.attempted), list(so.found), list(sg.found))
        assert (so.did_coarse, so.n_zmssd) == (sg.did_coarse, sg.n_zmssd), (tag, so.did_coarse, sg.did_coarse, so.n_zmssd, sg.n_zmssd)
        to, tg = o2.point_tracks(), g.point_tracks(0)
        pv = tg["level"] >= 0
        assert np.array_equal(to["searched"], tg["searched"]) and np.array_equal(to["found"][pv], tg["found"][pv]), tag
        fnd = pv & (tg["found"] == 1)
        assert np.array_equal(to["vfound"][fnd], tg["vfound"][fnd]), tag
        q = assess_tracking_quality(sg, sg.pose, [k["pose"] for k in self.m["keyframes"]], self.vp.wiggle_scale)
        assert sg.quality == q and sg.lost_frames == (before.lost_frames + 1 if q == 0 else 0), (tag, q, sg.quality, sg.lost_frames)
        assert not np.any(np.array(sg.velocity[:])) and sg.msd_velocity == before.msd_velocity, tag      # no UpdateMotionModel
        assert sg.kf_added == 0 and sg.n_keyframes == before.n_keyframes and sg.frame == before.frame + 1, tag
        return sg

    def close(self):
        self.g.close()


def test_recovery_at_blur_2_matches_the_oracle_composition():
    """a + c.  reloc_blur = 2.0 is the 9-tap branch: keyframe and current templates == orc.sbi_make, every ZMSSD and the
    best index == reloc_ref, ln(adj) and the ESM score == orc.sbi_rotation, mse3Best = exp(ln adj) * keyframe pose (1e-12 covers the
    test's own exp), then the recovered TrackMap bit for bit (module docstring; checked on the CPU beforehand to end GOOD)."""
    L = Lost(2.0)
    g, vp, t = L.g, L.vp, L.t
    gray = L.frames[t]
    L.before = g.state(0)
    L.step(gray)
    ri = g.reloc_info(0)
    assert (ri["attempts"], ri["successes"], ri["frame"]) == (1, 1, t + 1)
    cur_l3 = level3(gray)
    best, _ = L.expect_images(cur_l3, lambda l3: orc.sbi_make(l3, 2.0)[1])
    ln, score = orc.sbi_rotation(cur_l3, L.kf_l3[best], vp.cam[:], vp.quirks, 2.0)
    assert np.array_equal(ri["ln_adj"], ln) and ri["score"] == score, (ri["ln_adj"], ln, ri["score"], score)
    assert score < 9e6
    want_pose = pose_mul(orc.se3_exp(ln), g.keyframe_pose(0, best))
    assert np.abs(ri["best_pose"] - want_pose).max() < 1e-12
    sg = L.assert_recovered_frame_exact(gray, "recovered frame")
    assert sg.quality == 2 and sg.lost_frames == 0 and sg.did_coarse == 1
    assert "Tracking Map, quality good." in g.message(0)
    for t in range(L.t, N_FRAMES):                                   # and from there on it tracks like the stream that never lost track
        L.step(L.frames[t])
        s0 = g.state(0)
        assert s0.quality == 2 and s0.lost_frames == 0, t
        assert pose_err(s0.pose, L.o_ok.state().pose) < POSE_TOL, (t, pose_err(s0.pose, L.o_ok.state().pose))
        assert g.reloc_info(0)["attempts"] == 1, t
    assert g.reloc_info(1)["attempts"] == 0
    L.close()


def test_recovery_at_the_reference_blur():
    """b + c.  reloc_blur = 2.5, the reference's dBlur and the 17 x 17 branch: keyframe and current templates == reloc_ref's 17-tap
    result, ZMSSDs and best index == reloc_ref, the stream ends "Tracking Map, quality good." and is within POSE_TOL of stream 1 a
    few frames later.  ln(adj) and the ESM score == orc.sbi_rotation at blur 2.5, mse3Best = exp(ln adj) * keyframe pose."""
    L = Lost(2.5)
    g, t = L.g, L.t
    gray = L.frames[t]
    L.before = g.state(0)
    L.step(gray)
    ri = g.reloc_info(0)
    assert (ri["attempts"], ri["successes"]) == (1, 1) and ri["score"] < 9e6
    assert reloc_ref.taps_for(2.5) == 17
    cur_l3 = level3(gray)
    best, _ = L.expect_images(cur_l3, lambda l3: reloc_ref.make_from_l3(l3, 2.5)[1])
    ln, score = orc.sbi_rotation(cur_l3, L.kf_l3[best], L.vp.cam[:], L.vp.quirks, 2.5)
    assert np.array_equal(ri["ln_adj"], ln) and ri["score"] == score, (ri["ln_adj"], ln, ri["score"], score)
    assert np.abs(ri["best_pose"] - pose_mul(orc.se3_exp(ri["ln_adj"]), g.keyframe_pose(0, best))).max() < 1e-12
    L.assert_recovered_frame_exact(gray, "recovered frame, blur 2.5")
    for t in range(L.t, L.t + 4):
        L.step(L.frames[t])
    assert "Tracking Map, quality good." in g.message(0)
    d = pose_err(g.state(0).pose, g.state(1).pose)
    assert d < POSE_TOL, d
    L.close()


def test_failed_attempt_on_a_frame_of_noise():
    """d.  A frame of noise after the loss (a normal input).  The composition decides which of the two ends the reference has: a score
    >= 9e6 changes nothing but the attempt count; a score under the bar recovers into a TrackMap that the oracle composition runs too,
    and if that is BAD the stream stays lost with lost_frames still rising."""
    L = Lost(2.0)
    g, vp, t = L.g, L.vp, L.t
    noise = np.random.default_rng(5).integers(0, 256, size=(H, W)).astype(np.uint8)
    L.before = before = g.state(0)
    L.step(noise)
    ri, sg = g.reloc_info(0), g.state(0)
    cur_l3 = level3(noise)
    best, _ = L.expect_images(cur_l3, lambda l3: orc.sbi_make(l3, 2.0)[1])
    ln, score = orc.sbi_rotation(cur_l3, L.kf_l3[best], vp.cam[:], vp.quirks, 2.0)
    assert np.array_equal(ri["ln_adj"], ln) and ri["score"] == score
    assert ri["attempts"] == 1 and ri["frame"] == t + 1
    if score >= 9e6:
        assert ri["successes"] == 0
        assert np.array_equal(np.array(sg.pose[:]), np.array(before.pose[:])) and np.array_equal(np.array(sg.velocity[:]), np.array(before.velocity[:]))
        assert (sg.quality, sg.lost_frames, sg.frame) == (before.quality, before.lost_frames, before.frame + 1)
        assert list(sg.attempted) == list(before.attempted) and list(sg.found) == list(before.found)
    else:
        assert ri["successes"] == 1
        sg = L.assert_recovered_frame_exact(noise, "noise frame")
        if sg.quality == 0:
            assert sg.lost_frames == 4 and "Attempting recovery" in g.message(0)
    L.step(L.frames[L.t])                                              # no stream has faulted or hung: the next frame runs
    assert g.reloc_info(0)["attempts"] == (2 if sg.lost_frames >= 3 else 1)               # still lost: the next frame tried again
    L.close()


def test_keyframes_made_on_the_device_get_their_sbi():
    """e.  grow_map = 3: a keyframe the tracker asks for (k_add_keyframe) carries the SmallBlurryImage of its level 3, like the uploaded ones."""
    f, m, frames = make_scene(W, H, seed=SEED, n_frames=30, per_level=(120, 50, 20, 8))
    vp = capi.default_params(W, H, 1, relocalise=1, grow_map=3)
    g = capi.System(vp)
    g.load_map(0, m); g.set_pose(0, f.pose(-1))
    n0 = len(m["keyframes"])
    made = {}
    for t in range(30):
        g.track_frame(frames[t][None])
        if g.state(0).kf_added:
            made[g.state(0).n_keyframes - 1] = t
    assert made and min(made) == n0, made
    for k in range(n0):
        assert np.array_equal(g.keyframe_sbi(0, k)[0], reloc_ref.make_from_l3(level3(m["keyframes"][k]["image"]), 2.5)[1]), k
    for k, t in made.items():
        tmpl, jacs = g.keyframe_sbi(0, k)
        assert np.array_equal(tmpl, reloc_ref.make_from_l3(level3(frames[t]), 2.5)[1]), (k, t)
        assert np.array_equal(jacs, reloc_ref.make_jacs(tmpl)), (k, t)
    with pytest.raises(capi.VslamError):
        g.keyframe_sbi(0, g.state(0).n_keyframes)
    g.close()


def test_relocalise_off_changes_nothing():
    """f.  The default: vslam_attempt_recovery is a no-op that returns VSLAM_OK, the read-backs answer VSLAM_E_STATE, a lost stream stays lost."""
    f, m, frames = scene()
    vp = capi.default_params(W, H, 1, **KW)
    assert vp.relocalise == 0 and vp.reloc_blur == 2.5
    g = capi.System(vp)
    o = make_oracle(vp, m, f.pose(-1))
    g.load_map(0, m); g.set_pose(0, f.pose(-1))
    blank = np.zeros((H, W), np.uint8)
    for t in range(2 + N_BLANK + 2):
        fr = frames[t] if t < 2 or t >= 2 + N_BLANK else blank
        g.make_keyframe_lite(fr[None])
        before = g.state(0)
        g.attempt_recovery(); g.synchronize()
        after = g.state(0)
        assert bytes(before) == bytes(after), t
        g.patch_search(0); g.pose_update(0); g.patch_search(1); g.pose_update(1); g.finish_frame()
        o.track_frame(fr)
        so, sg = o.state(), g.state(0)
        assert (so.quality, so.lost_frames, so.frame) == (sg.quality, sg.lost_frames, sg.frame) and np.array_equal(np.array(so.pose[:]), np.array(sg.pose[:])), t
    assert g.state(0).lost_frames == 3 and "Attempting recovery" in g.message(0)
    for call in (lambda: g.keyframe_sbi(0, 0), lambda: g.reloc_info(0), lambda: g.reloc_attempt(0)):
        with pytest.raises(capi.VslamError, match="vslam error -4"):
            call()
    g.close()
