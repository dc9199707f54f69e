"""CPU check of tests/sbi_cases.py: the table of sizes is what the constants of csrc/sbi_dev.h give (a constant edited without the table
fails here, instead of quietly leaving a fork of the kernels uncovered), the oracle alone gives a real alignment on every row that has
interior pixels and the singular one on the rows that have none, and the relocaliser cases of tests/test_gpu_sbi_sizes.py end at the
keyframe they name.  Run with -s to see the figures per row."""
import numpy as np
import pytest

import sbi_cases as sc
from visualslam_android_amd import capi


def check_table(c):
    for r in sc.TABLE:
        g = sc.geometry(r.w, r.h, c)
        assert (g.W, g.H, g.N, g.nch, g.last, g.lds) == (r.W, r.H, r.N, r.nch, r.last, r.lds), (r, g)
        assert g.lds == g.floats + max(g.pos, g.rec) and g.floats == 8 * g.N and g.pos == 16 * g.N and g.rec == 16 * c["SBI_CHUNK"] * c["SBI_REC"]
        for name in r.hits:
            assert sc.PROPERTIES[name](r.w, r.h, g, c), (sc.size_id(r), name)
    hit = {name for r in sc.TABLE for name in r.hits}
    assert hit == set(sc.PROPERTIES), set(sc.PROPERTIES) - hit
    assert [sc.size_id(r) for r in sc.REFUSED] == ["1040x1024"] and len(sc.LEGAL) == 14
    assert [sc.size_id(r) for r in sc.DEGENERATE] == ["48x48", "56x72"]
    for r in sc.LEGAL:
        assert r.N <= c["SBI_MAX_PIX"] and r.H <= c["SBI_THREADS"], r            # what sbi_args accepts
    # the relocaliser stages RELOC_KF_PER_ROUND keyframe templates of N floats in the ESM's working area
    per_round = c["RELOC_KF_PER_ROUND"]
    for k in sc.RELOC_CASES:
        g = sc.geometry(k.w, k.h, c)
        assert per_round * g.N * 4 <= max(g.pos, g.rec), k.name
    by = {k.name: k for k in sc.RELOC_CASES}
    assert {k.nk % per_round for k in sc.RELOC_CASES} == {1, 2, 3}                # the partial last rounds; eight keyframes, two full rounds, is test_gpu_relocalise.py
    assert by["best in a second round of one"].nk == per_round + 1 == by["best in a second round of one"].best + 1
    assert by["map at max_keyframes"].cap == by["map at max_keyframes"].nk
    g = sc.geometry(by["large LDS"].w, by["large LDS"].h, c)
    assert g.lds > sc.LDS_NO_ATTRIBUTE and per_round * g.N * 4 == g.pos > g.rec  # the staged templates fill the whole working area


def test_table_is_what_the_constants_give():
    c = sc.constants()
    check_table(c)
    for r in sc.TABLE:
        g = sc.geometry(r.w, r.h, c)
        print("  %-9s level 3 %3dx%-3d small %2dx%-2d N %4d chunks %2d last %3d  LDS %5d + max(%5d, %5d) = %5d  %s" % (
            sc.size_id(r), g.w3, g.h3, g.W, g.H, g.N, g.nch, g.last, g.floats, g.pos, g.rec, g.lds, "; ".join(r.hits)))


@pytest.mark.parametrize("name,value", [("SBI_CHUNK", 64), ("SBI_CHUNK", 256), ("SBI_THREADS", 128), ("SBI_THREADS", 512), ("SBI_MAX_PIX", 3600),
                                        ("SBI_MAX_PIX", 8192), ("SBI_REC", 16), ("RELOC_KF_PER_ROUND", 2)])
def test_an_edited_constant_fails_the_table(name, value):
    c = sc.constants()
    assert c[name] != value
    with pytest.raises(AssertionError):
        check_table(dict(c, **{name: value}))


@pytest.mark.parametrize("r", sc.LEGAL, ids=sc.size_id)
def test_oracle_on_the_rows_frames(r):
    """b + c.  Rows with interior pixels: the repeated frame aligns with score 0, the warped one with a rotation and a score that are
    not zero.  The two smallest: no pixel survives the skip test, the solve is singular, the update is zero: the rotation is the
    identity alignment's and the score 0."""
    cam = capi.default_params(r.w, r.h, 1).cam[:]
    frames, want = sc.frames_and_expected(r, cam)
    assert len(frames) == sc.STREAMS and not np.array_equal(frames[0][0], frames[1][0])
    for s in range(sc.STREAMS):
        assert np.array_equal(frames[s][0], frames[s][1]) and not np.array_equal(frames[s][0], frames[s][2])
        assert sc.level3(frames[s][0]).shape == (r.h >> 3, r.w >> 3)
        for t in range(3):
            small, tmpl, rot, score = want[s][t]
            assert small.shape == tmpl.shape == (r.H, r.W) and np.isfinite(rot).all() and np.isfinite(score)
        for t in range(2):
            assert want[s][t][3] == 0.0 and np.abs(want[s][t][2]).max() < 1e-12, (s, t, want[s][t][2:])
        rot, score = want[s][2][2:]
        print("  %-9s stream %d: warped frame rotation %s score %.6g" % (sc.size_id(r), s, np.array2string(rot[3:], precision=5), score))
        # "rotation 0" is the identity alignment's: SE3fromSE2's project / unproject round trip leaves 1e-16 in the last bits
        if r in sc.DEGENERATE:
            assert np.array_equal(rot, want[s][0][2]) and np.abs(rot).max() < 1e-15 and score == 0.0, (rot, score)
        else:
            assert r.N >= 56 and np.abs(rot[3:]).max() > 1e-6 and score > 0.0, (rot, score)


@pytest.mark.parametrize("blur", sc.RELOC_BLURS)
@pytest.mark.parametrize("c", sc.RELOC_CASES, ids=lambda c: c.name)
def test_relocaliser_cases_end_at_the_keyframe_they_name(c, blur):
    cam = capi.default_params(c.w, c.h, 1).cam[:]
    for s, (kfs, frame) in enumerate(sc.reloc_images(c)):
        assert len(kfs) == c.nk
        e = sc.reloc_expected(kfs, frame, blur, cam)
        z = e["zmssd"]
        print("  %s, blur %.1f, stream %d: ZMSSD %s best %d, ESM score %.6g" % (c.name, blur, s, np.array2string(z, precision=1), e["best"], e["score"]))
        assert e["best"] == c.best and z[c.best] == z.min() and e["score"] < 9e6
        for a, b in c.same:
            assert kfs[a] is kfs[b] and z[a] == z[b]
        others = [k for k in range(c.nk) if k != c.best and (c.best, k) not in c.same]
        assert all(z[k] > z[c.best] for k in others)
        if c.name == "tie at the minimum":
            (a, b), = c.same
            assert a == c.best < b                                      # the first of two equal minima (jni/Relocaliser.cc:53)
        if c.name == "tie above the minimum":
            (a, b), = c.same
            assert z[a] > z[c.best] and a < c.best < b                   # an equal pair on both sides of the minimum, in two rounds
