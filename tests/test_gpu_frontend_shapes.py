"""GPU parity of the front end at the sizes where its two forms split: the strip form (k_fast_slide) takes a frame whose every level
is a multiple of 4 and at least 16 wide and at least 7 high and whose source is 16-B aligned, the band form (k_pyr_fast0 / k_fast_lvl)
takes the rest.  Level images, corner lists, row LUTs, FAST scores, maximal corners and Shi-Tomasi candidates against the oracle, bit for
bit: odd and minimal sizes, one frame through both forms, streams that share a strip workgroup, corners on the borders and on the kernels'
seams, extreme thresholds, and frames too wide for 64 KiB of LDS on the band form."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import synth_image
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = (10, 15, 15, 10)                   # vslam_default_params
BARRIER = 10
MIN_ST = 70.0                            # gvdCandidateMinSTScore (jni/KeyFrame.cc:57): the oracle finds candidates with it at every size
                                         # of the sweep, on the one or two levels that have room inside the 10-px border


def strip_eligible(w, h):
    """fe_slide_ok's conditions on the shape"""
    return all(((w >> l) & 3) == 0 and (w >> l) >= 16 and (h >> l) >= 7 for l in range(4))


# ---- the oracle's answer for one frame, computed once per (frame, settings) ----------------------------------------------------------
_REF = {}


def reference(oracle, key, img, thr=THR, quirk=False, min_st=MIN_ST):
    """per level: (image, corners, lut, scores, maximal corners, candidate positions, candidate scores); key names the frame"""
    k = (key, tuple(thr), bool(quirk), min_st)
    if k not in _REF:
        out = []
        for lv, corners, lut in oracle.make_keyframe_lite(img, thr):
            sc = oracle.fast_score(lv, corners, BARRIER)
            keep = oracle.nonmax(corners, sc, quirk=quirk)
            pos, st = oracle.candidates(lv, keep, min_st, 10)
            out.append((lv, corners, lut, sc, keep, pos, st))
        _REF[k] = out
    return _REF[k]


def synth_frames(seeds, w, h):
    return np.stack([synth_image(s, w, h) for s in seeds])


def synth_refs(oracle, seeds, w, h, frames, **kw):
    return [reference(oracle, ("synth", s, w, h), frames[i], **kw) for i, s in enumerate(seeds)]


# ---- feeding frames: from the host, or from a device buffer laid out to take one form or the other ----------------------------------
MODES = {                                # name: (byte offset of the base, extra bytes per row)
    "host": None,
    "dev": (0, 0),                       # 16-B aligned and tight: the strip form where the shape allows it
    "dev+1": (1, 0),                     # the band form: base not 16-B aligned
    "dev+4": (4, 0),                     # the band form: base dword- but not 16-B aligned
    "pitch+4": (0, 4),                   # the band form: pitch not a multiple of 16
}


def feed(g, frames, mode):
    """vslam_make_keyframe_lite in the given mode; returns what has to stay alive while the frame is read back (a device source is
    not copied: level 0 is read in place).  The bytes of the buffer that are no pixels are noise."""
    if mode == "host":
        g.make_keyframe_lite(frames)
        return None
    import torch
    S, h, w = frames.shape
    off, pad = MODES[mode]
    pitch = w + pad
    sstride = h * pitch
    buf = np.random.default_rng(1).integers(0, 256, size=off + S * sstride + 16, dtype=np.uint8)
    for s in range(S):
        buf[off + s * sstride: off + (s + 1) * sstride].reshape(h, pitch)[:, :w] = frames[s]
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    g.make_keyframe_lite_device(dev.data_ptr() + off, pitch, sstride)
    g.synchronize()
    return dev


def read_lite(g, s):
    return [(g.read_level_image(s, l), g.read_corners(s, l), g.read_row_lut(s, l)) for l in range(4)]


def check_lite(g, s, ref, tag):
    got = read_lite(g, s)
    for l in range(4):
        img, corners, lut = ref[l][:3]
        assert np.array_equal(got[l][0], img), (tag, s, l, "image")
        assert np.array_equal(got[l][1], corners), (tag, s, l, "corners", len(got[l][1]), len(corners))
        assert np.array_equal(got[l][2], lut), (tag, s, l, "lut")
    return got


def check_rest(g, refs, tag):
    """fast_nonmax, then make_keyframe_rest, of the current frame of every stream"""
    out = []
    g.fast_nonmax()
    for s, ref in enumerate(refs):
        for l in range(4):
            sc, keep = ref[l][3], ref[l][4]
            got, gsc = g.read_max_corners(s, l)
            assert np.array_equal(gsc[:len(sc)], sc), (tag, s, l, "scores")
            assert np.array_equal(got, keep), (tag, s, l, "maximal corners", len(got), len(keep))
            out.append((gsc[:len(sc)].copy(), got))
    g.make_keyframe_rest(MIN_ST)
    for s, ref in enumerate(refs):
        for l in range(4):
            pos, st = ref[l][5], ref[l][6]
            gpos, gst = g.read_candidates(s, l)
            assert np.array_equal(gpos, pos), (tag, s, l, "candidates", len(gpos), len(pos))
            assert np.array_equal(gst, st), (tag, s, l, "candidate scores")
            out.append((gpos.copy(), gst.copy()))
    return out


def check_all(g, refs, tag):
    got = [check_lite(g, s, ref, tag) for s, ref in enumerate(refs)]
    return got, check_rest(g, refs, tag)


def assert_same_results(a, b, tag):
    """two nested lists / tuples of arrays, as check_all returns them"""
    if isinstance(a, np.ndarray):
        assert np.array_equal(a, b), tag
    else:
        assert len(a) == len(b), tag
        for x, y in zip(a, b):
            assert_same_results(x, y, tag)


# ---- 1. shape sweep, host input -----------------------------------------------------------------------------------------------------
SWEEP = [                                # (w, h, form)
    (48, 48, "band"),                    # the vslam_create minimum: level 3 is 6x6 and has no FAST row
    (49, 51, "band"),                    # odd width and height
    (63, 48, "band"),                    # odd width
    (127, 56, "band"),                   # one column short of the strip limit
    (128, 55, "band"),                   # strip width, level-3 height 6
    (131, 77, "band"),                   # odd width, odd halvings
    (203, 77, "band"),
    (128, 56, "strip"),                  # the strip form's smallest size: level 3 is 16x7
    (160, 63, "strip"),                  # odd halvings 63 -> 31 -> 15 -> 7
    (224, 100, "strip"),                 # level-3 width 28, no multiple of 16
    (256, 57, "strip"),                  # odd height
    (288, 70, "strip"),                  # odd halvings 35 -> 17
]
SWEEP_SEEDS = (9, 10, 11)
QUIRK_SHAPES = [(131, 77), (160, 63)]    # Q_NONMAX_RIGHT_NEIGHBOUR on one band-form and one strip-form shape


def run_sweep_shape(oracle, w, h, quirk):
    frames = synth_frames(SWEEP_SEEDS, w, h)
    refs = synth_refs(oracle, SWEEP_SEEDS, w, h, frames, quirk=bool(quirk))
    for ref in refs:
        for l in range(4):
            assert len(ref[l][1]) < max(256, ((w >> l) * (h >> l)) // 2), (l, "the oracle's count exceeds the default capacity")
    g = capi.System(capi.default_params(w, h, len(SWEEP_SEEDS), quirks=quirk))
    other = synth_frames([s + 50 for s in SWEEP_SEEDS], w, h)
    g.make_keyframe_lite(other)          # both front-end buffers hold another frame's masks, counts and lists before the checked frame
    g.make_keyframe_lite(other[::-1].copy())
    g.make_keyframe_lite(frames)
    check_all(g, refs, (w, h))
    g.close()
    return sum(len(ref[l][5]) for ref in refs for l in range(4))


@pytest.mark.parametrize("w,h,form", SWEEP)
def test_shape_sweep(oracle, w, h, form):
    assert strip_eligible(w, h) == (form == "strip")
    run_sweep_shape(oracle, w, h, 0)


@pytest.mark.parametrize("w,h", QUIRK_SHAPES)
def test_shape_sweep_nonmax_quirk(oracle, w, h):
    run_sweep_shape(oracle, w, h, capi.Q_NONMAX_RIGHT_NEIGHBOUR)


def test_shape_sweep_has_candidates(oracle):
    """the candidate comparison of the sweep is not vacuous: the oracle, which test_shape_sweep holds the device to, finds candidates on
    band-form and on strip-form shapes"""
    n = {"band": 0, "strip": 0}
    for w, h, form in SWEEP:
        frames = synth_frames(SWEEP_SEEDS, w, h)
        n[form] += sum(len(ref[l][5]) for ref in synth_refs(oracle, SWEEP_SEEDS, w, h, frames) for l in range(4))
    assert n["band"] > 20 and n["strip"] > 20, n


# ---- 2. one frame through both forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,S", [(128, 56, 5), (256, 57, 5), (224, 100, 5), (640, 480, 1)])
def test_both_forms_agree(oracle, w, h, S):
    assert strip_eligible(w, h)
    seeds = [20 + s for s in range(S)]
    frames = synth_frames(seeds, w, h)
    refs = synth_refs(oracle, seeds, w, h, frames)
    g = capi.System(capi.default_params(w, h, S))
    first = None
    for mode in MODES:                   # host and "dev" take the strip form, the other three the band form
        keep = feed(g, frames, mode)
        got = check_all(g, refs, (w, h, mode))
        del keep
        if first is None:
            first = got
        else:
            assert_same_results(first, got, (w, h, mode))
    g.close()


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from visualslam_android_amd import capi
w, h = 128, 56
g = capi.System(capi.default_params(w, h, 1))
buf = torch.from_numpy(np.full(w * h + 16, 90, np.uint8)).cuda()
assert buf.data_ptr() % 16 == 0
g.make_keyframe_lite_device(buf.data_ptr(), w, w * h)
g.synchronize()
g.make_keyframe_lite_device(buf.data_ptr() + 1, w, w * h)
g.synchronize()
g.close()
print("child done")
"""


def test_dispatch_follows_the_alignment():
    """An aligned device frame takes the strip form and the same frame one byte further on does not: VSLAM_FE_DEBUG (read once per
    process, hence the child) makes fe_launch_slide announce itself on stderr."""
    env = dict(os.environ, VSLAM_FE_DEBUG="1")
    env.pop("VSLAM_FE_BANDS", None)
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
    assert out.returncode == 0 and "child done" in out.stdout, out.stderr[-2000:]
    assert len([l for l in out.stderr.splitlines() if l.startswith("fe slide:")]) == 1, out.stderr[-2000:]


# ---- 3. streams sharing a strip workgroup -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,S", [(128, 56, 7), (160, 63, 11)])
def test_streams_sharing_a_workgroup(oracle, w, h, S):
    """A strip workgroup owns 256 / (w / 16) bands of consecutive frames: at these sizes it holds strips of several streams (32 and 25
    bands; a stream has 1..4) and the last workgroup is part empty.  Every stream against the oracle; permuted streams give permuted results."""
    assert strip_eligible(w, h)
    seeds = [40 + s for s in range(S)]
    frames = synth_frames(seeds, w, h)
    refs = synth_refs(oracle, seeds, w, h, frames)
    g = capi.System(capi.default_params(w, h, S))
    g.make_keyframe_lite(frames)
    check_all(g, refs, (w, h, "in order"))
    perm = [(3 * s + 2) % S for s in range(S)]                       # S is coprime to 3: a permutation without fixed neighbours
    assert sorted(perm) == list(range(S))
    g.make_keyframe_lite(frames[perm].copy())
    check_all(g, [refs[p] for p in perm], (w, h, "permuted"))
    g.close()


# ---- 4. corners on the borders and seams --------------------------------------------------------------------------------------------
def dot_image(w, h):
    """flat 50 with single pixels of 200 on the first and last legal columns and rows, one outside them, and on the kernels' seams:
    strip edges (multiples of 16), wavefront and mask-word edges (64, 128), band edges (16, 32, ...), the seven-row rounds"""
    xs = sorted({x for x in (0, 2, 3, 15, 16, 31, 32, 63, 64, 127, 128, w - 4, w - 3, w - 1) if 0 <= x < w})
    ys = sorted({y for y in (0, 2, 3, 9, 15, 16, 23, 31, 32, 47, 48, 63, 64, h - 4, h - 3, h - 1) if 0 <= y < h})
    img = np.full((h, w), 50, np.uint8)
    for y in ys:
        for x in xs:
            img[y, x] = 200
    want = [(y << 16) | x for y in ys for x in xs if 3 <= x < w - 3 and 3 <= y < h - 3]
    return img, np.array(want, np.uint32)


@pytest.mark.parametrize("w,h,mode", [(160, 72, "host"), (160, 72, "dev+1"), (131, 77, "host")])
def test_dots_on_borders_and_seams(oracle, w, h, mode):
    """An isolated dot is a FAST corner and nothing around it is one: the level-0 list is exactly the dots FAST may look at
    (cvfast.cpp:6113-6117), whatever strip, wavefront, mask word, band or round they fall on; the same for dark dots on a bright frame."""
    img, want = dot_image(w, h)
    if (w, h) == (160, 72):
        assert len(want) == 120
    frames = np.stack([img, 250 - img])                               # 50 on 200
    refs = [reference(oracle, ("dots", w, h), frames[0]), reference(oracle, ("dots inverted", w, h), frames[1])]
    assert np.array_equal(refs[0][0][1], want) and np.array_equal(refs[1][0][1], want)
    g = capi.System(capi.default_params(w, h, 2))
    keep = feed(g, frames, mode)
    for s in range(2):
        assert np.array_equal(g.read_corners(s, 0), want), (s, sorted(set(g.read_corners(s, 0).tolist()) ^ set(want.tolist())))
    check_all(g, refs, (w, h, mode))
    del keep
    g.close()


# ---- 5. thresholds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [(1,) * 4, (40,) * 4, (120,) * 4, (255,) * 4, (3, 180, 1, 60)])
@pytest.mark.parametrize("w,h,mode", [(160, 72, "host"), (160, 72, "dev+4"), (131, 77, "host")])
def test_thresholds(oracle, w, h, mode, thr):
    seeds = (9, 10)
    frames = synth_frames(seeds, w, h)
    refs = synth_refs(oracle, seeds, w, h, frames, thr=thr)
    n0 = len(refs[0][0][1])
    assert n0 < (w * h) // 2
    if (w, h) == (160, 72) and len(set(thr)) == 1:                   # the frame these settings were chosen on: many, some, few, none
        assert n0 == {1: 2488, 40: 96, 120: 9, 255: 0}[thr[0]]      # (nothing is 255 brighter or darker than a byte)
    g = capi.System(capi.default_params(w, h, len(seeds), fast_threshold=list(thr)))
    keep = feed(g, frames, mode)
    check_all(g, refs, (w, h, mode, thr))
    del keep
    g.close()


# ---- 7. frames wider than 64 KiB of LDS on the band form -----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,mode", [(1928, 48, "host"), (4095, 49, "host"), (4096, 56, "host"), (4096, 56, "dev+1")])
def test_wide_frames(oracle, w, h, mode):
    """The band kernels stage a band at its full width: (16 + 6) * lp0 + 8 * lp1 + 4 * lp2 + 16 * nchunk * 8 + 8 * lp0 + 32 bytes of
    dynamic LDS, 71,872 B at 1928 and 151,584 B at 4095 and 4096, above the 64 KiB a kernel gets without raising its limit and
    below the CU's 160 KiB.  4096x56 from the host takes the strip form, everything else here the band form."""
    assert strip_eligible(w, h) == (w == 4096)
    frames = synth_frames([60], w, h)
    refs = synth_refs(oracle, [60], w, h, frames)
    for l in range(4):
        assert 0 < len(refs[0][l][1]) < ((w >> l) * (h >> l)) // 2 or (h >> l) < 7
    g = capi.System(capi.default_params(w, h, 1))
    keep = feed(g, frames, mode)
    check_all(g, refs, (w, h, mode))
    del keep
    g.close()


def test_wide_keyframe_upload(oracle):
    """a keyframe uploaded with grow_map always takes the band form (fe_keyframe_corners): its stored corner lists at a width above 1,760"""
    w, h = 1928, 48
    img = synth_image(61, w, h)
    vp = capi.default_params(w, h, 1, grow_map=3, max_keyframes=2)
    g = capi.System(vp)
    pose = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
    assert g.add_keyframe(0, pose, 1, img, 1.0, 0.1) == 0
    want = oracle.make_keyframe_lite(img, THR)
    for l in range(4):
        corners = want[l][1][:min(vp.max_corners[l], (16384, 8192, 4096, 2048)[l])]
        assert np.array_equal(g.keyframe_corners(0, 0, l), corners), l
    assert len(want[0][1]) > 1000
    g.close()
