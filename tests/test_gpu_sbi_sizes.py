"""GPU: the SmallBlurryImage kernels (k_sbi, k_sbi_restart, k_kf_sbi, k_recover; csrc/sbi_dev.h, sbi.hip, reloc.hip) at the sizes and
keyframe counts of tests/sbi_cases.py, where their loops split: N below, at and above SBI_CHUNK and SBI_THREADS, odd W, H and N, odd
level-3 sizes, every region of sbi_lds_bytes including the launches above 48 KiB of dynamic LDS, the singular ESM of a small image
without interior pixels and of a blank frame, partial rounds, ties and the cap of the relocaliser's scoring, both blur branches.

Everything is compared with the oracle (orc.sbi_make, orc.sbi_rotation; tests/reloc_ref.py for the ZMSSD) bit for bit: this stage's
stated contract.  tests/test_sbi_cases.py is the CPU check that the table reaches what it names."""
import numpy as np
import pytest

import sbi_cases as sc
from helpers import make_scene
from oracle import binding as orc
from visualslam_android_amd import capi
from visualslam_android_amd.feeder import MapData

pytestmark = pytest.mark.gpu

E_INVALID = "vslam error -1"


def assert_sbi(g, s, want, tag):
    small, tmpl, rot, score = g.read_sbi(s)
    wsmall, wtmpl, wrot, wscore = want
    assert np.array_equal(small, wsmall), tag
    assert tmpl.dtype == wtmpl.dtype and np.array_equal(tmpl, wtmpl), (tag, float(np.abs(tmpl - wtmpl).max()))
    assert np.array_equal(rot, wrot) and score == wscore, (tag, rot, wrot, score, wscore)


@pytest.mark.parametrize("r", sc.LEGAL, ids=sc.size_id)
def test_frame_sbi_is_the_oracles(r):
    """k_sbi alone: three streams, three frames (A, A, A warped), front end only -- no map, no tracker.  After every frame the small
    image, the template, the rotation and the score of every stream == the oracle's."""
    vp = capi.default_params(r.w, r.h, sc.STREAMS, use_sbi=1)
    frames, want = sc.frames_and_expected(r, vp.cam[:], vp.quirks)
    g = capi.System(vp)
    try:
        for t in range(3):
            g.make_keyframe_lite(np.stack([frames[s][t] for s in range(sc.STREAMS)]))
            for s in range(sc.STREAMS):
                assert_sbi(g, s, want[s][t], "%s stream %d frame %d" % (sc.size_id(r), s, t))
    finally:
        g.close()


def test_blank_frame_is_the_singular_alignment():
    """A blank frame after a textured one: zero template, every product of the ESM zero, the solve singular, the update zero."""
    r = next(x for x in sc.LEGAL if sc.size_id(x) == "496x496")
    vp = capi.default_params(r.w, r.h, 2, use_sbi=1)
    frames, want = sc.frames_and_expected(r, vp.cam[:], vp.quirks)
    blank = np.zeros((r.h, r.w), np.uint8)
    l3a, l3b = sc.level3(frames[0][0]), sc.level3(blank)
    g = capi.System(vp)
    try:
        g.make_keyframe_lite(np.stack([frames[0][0], blank]))
        assert_sbi(g, 0, want[0][0], "textured")
        assert_sbi(g, 1, orc.sbi_make(l3b) + orc.sbi_rotation(l3b, l3b, vp.cam[:], vp.quirks), "blank first frame")
        g.make_keyframe_lite(np.stack([blank, frames[0][0]]))
        assert_sbi(g, 0, orc.sbi_make(l3b) + orc.sbi_rotation(l3b, l3a, vp.cam[:], vp.quirks), "blank after textured")
        assert_sbi(g, 1, orc.sbi_make(l3a) + orc.sbi_rotation(l3a, l3b, vp.cam[:], vp.quirks), "textured after blank")
        assert not g.read_sbi(0)[1].any() and g.read_sbi(1)[1].any()
    finally:
        g.close()


def test_one_column_over_the_limit_is_refused():
    """Today's behaviour at 65 x 64 small pixels, host-side argument checks both (nothing is launched with the size): use_sbi = 1 is
    refused by the first frame and the system can still be closed; relocalise = 1 is refused at creation."""
    r, = sc.REFUSED
    frame = np.stack([sc.render(sc.texture(1), r.w, r.h, 2)])
    g = capi.System(capi.default_params(r.w, r.h, 1, use_sbi=1))
    with pytest.raises(capi.VslamError, match=E_INVALID):
        g.make_keyframe_lite(frame)
    g.close()
    assert not g.h
    with pytest.raises(capi.VslamError, match=E_INVALID):
        capi.System(capi.default_params(r.w, r.h, 1, relocalise=1))
    capi.System(capi.default_params(r.w, r.h, 1)).close()                      # the size itself is a legal one


def test_restart_above_48k_of_lds():
    """k_sbi_restart at the first size that raises the dynamic-LDS limit: stream 1 is reset after two frames; its next frame is a first
    frame, both SmallBlurryImages made from it, while stream 0's is the ordinary frame-to-frame one; the frame after that is ordinary
    for both (the restart flag is spent)."""
    r = next(x for x in sc.LEGAL if "first size with the attribute" in x.hits)
    vp = capi.default_params(r.w, r.h, 2, use_sbi=1)
    cam, q = vp.cam[:], vp.quirks
    frames, want = sc.frames_and_expected(r, cam, q)
    l3 = [[sc.level3(x) for x in frames[s]] for s in range(2)]
    g = capi.System(vp)
    try:
        for t in range(2):
            g.make_keyframe_lite(np.stack([frames[0][t], frames[1][t]]))
        g.reset([1])
        g.make_keyframe_lite(np.stack([frames[0][2], frames[1][2]]))
        assert_sbi(g, 0, want[0][2], "neighbour of the reset stream")
        first = orc.sbi_make(l3[1][2]) + orc.sbi_rotation(l3[1][2], l3[1][2], cam, q)
        assert first[3] == 0.0 and want[1][2][3] > 0.0 and not np.array_equal(first[2], want[1][2][2])
        assert_sbi(g, 1, first, "reset stream, first frame")
        g.make_keyframe_lite(np.stack([frames[0][0], frames[1][0]]))
        for s in range(2):
            assert_sbi(g, s, orc.sbi_make(l3[s][0]) + orc.sbi_rotation(l3[s][0], l3[s][2], cam, q), "stream %d, the frame after" % s)
    finally:
        g.close()


# ---- the relocaliser -------------------------------------------------------------------------------------------------------------
_scenes = {}


def lost_scene(c):
    """the smallest kind of map build_map gives, at the case's size and keyframe count; its keyframe images are replaced per stream"""
    key = (c.w, c.h, c.nk)
    if key not in _scenes:
        f, m, _frames = make_scene(c.w, c.h, seed=77, n_frames=1, n_keyframes=c.nk, per_level=(60, 24, 8, 4))
        _scenes[key] = (f.pose(-1), m)
    return _scenes[key]


def pose_mul(a, b):
    Ra, ta, Rb, tb = np.asarray(a[:9]).reshape(3, 3), np.asarray(a[9:12]), np.asarray(b[:9]).reshape(3, 3), np.asarray(b[9:12])
    return np.concatenate([(Ra @ Rb).reshape(-1), Ra @ tb + ta])


@pytest.mark.parametrize("blur", sc.RELOC_BLURS)
@pytest.mark.parametrize("c", sc.RELOC_CASES, ids=lambda c: c.name)
def test_relocaliser_scoring_and_esm(c, blur):
    """k_kf_sbi and k_recover with the test's own keyframe images.  Two streams, each with its own images, are fed blank frames until
    lost_frames == 3 (the tracker never reads a keyframe image on them); then the staged frame: make_keyframe_lite, attempt_recovery,
    read everything, and the usual stages to leave the system consistent."""
    S = sc.RELOC_STREAMS
    kw = dict(relocalise=1, reloc_blur=blur, min_frames_between_kf=1000)
    if c.cap is not None:
        kw["max_keyframes"] = c.cap
    vp = capi.default_params(c.w, c.h, S, **kw)
    cam, q = vp.cam[:], vp.quirks
    start, m = lost_scene(c)
    images = sc.reloc_images(c)
    g = capi.System(vp)
    try:
        for s in range(S):
            kfs = [dict(k, image=img) for k, img in zip(m["keyframes"], images[s][0])]
            g.load_map(s, MapData(keyframes=kfs, packed=m["packed"], times=m["times"]))
            g.set_pose(s, start)
        blank = np.zeros((S, c.h, c.w), np.uint8)
        for _t in range(3):
            g.track_frame(blank)
        for s in range(S):
            st = g.state(s)
            assert (st.quality, st.lost_frames, st.n_keyframes, st.frame) == (0, 3, c.nk, 3) and g.reloc_info(s)["attempts"] == 0, s
        assert c.cap is None or g.state(0).n_keyframes == vp.max_keyframes
        g.make_keyframe_lite(np.stack([images[s][1] for s in range(S)]))
        g.attempt_recovery(); g.synchronize()
        for s in range(S):
            tag = "%s, blur %.1f, stream %d" % (c.name, blur, s)
            e = sc.reloc_expected(images[s][0], images[s][1], blur, cam, q)
            for k in range(c.nk):
                tmpl, jacs = g.keyframe_sbi(s, k)
                assert np.array_equal(tmpl, e["kf_tmpl"][k]) and np.array_equal(jacs, e["kf_jacs"][k]), (tag, k)
            cur, scores = g.reloc_attempt(s)
            assert np.array_equal(cur, e["cur"]), tag
            assert len(scores) == c.nk and np.array_equal(scores, e["zmssd"]), (tag, scores, e["zmssd"])
            for a, b in c.same:
                assert scores[a] == scores[b], (tag, a, b)
            ri = g.reloc_info(s)
            assert (ri["attempts"], ri["best"], ri["frame"]) == (1, c.best, 4) and e["best"] == c.best, (tag, ri, e["best"])
            assert ri["best_zmssd"] == e["zmssd"][c.best], tag
            assert np.array_equal(ri["ln_adj"], e["ln"]) and ri["score"] == e["score"], (tag, ri["ln_adj"], e["ln"], ri["score"], e["score"])
            want_pose = pose_mul(orc.se3_exp(e["ln"]), g.keyframe_pose(s, c.best))
            assert np.abs(ri["best_pose"] - want_pose).max() < 1e-12, tag
            assert ri["successes"] == int(e["score"] < 9e6), tag
            st = g.state(s)
            if ri["successes"]:                                      # Tracker::AttemptRecovery, jni/Tracker.cc:169-174
                assert np.array_equal(np.array(st.pose[:]), ri["best_pose"]) and not np.any(np.array(st.velocity[:])), tag
        g.patch_search(0); g.pose_update(0); g.patch_search(1); g.pose_update(1); g.finish_frame()
        assert all(g.state(s).frame == 4 for s in range(S))
    finally:
        g.close()
