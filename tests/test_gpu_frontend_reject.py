"""GPU parity of the front end on frames built for the strip kernel's packed quick reject and the wavefront compaction
(tests/frontend_reject_cases.py): pixel values on the predicate's edges, a 0 / 255 checkerboard, a gradient whose compass pixels differ
from their centre by exactly t and t + 1, at the sizes where the strip loop's rounds and the compaction's bands split.  Level images,
corner lists, row LUTs and corner counts against the oracle, bit for bit.  tests/test_frontend_reject_cases.py shows on the CPU that the
oracle's lists are not empty."""
import numpy as np
import pytest

import frontend_reject_cases as fc
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu


def feed(g, frames, pad):
    """host input, or a 16-B aligned device buffer whose rows are pad bytes longer than the frame (noise in the padding)"""
    if pad is None:
        g.make_keyframe_lite(frames)
        return None
    import torch
    S, h, w = frames.shape
    pitch = w + pad
    buf = np.random.default_rng(1).integers(0, 256, size=S * h * pitch + 16, dtype=np.uint8)
    for s in range(S):
        buf[s * h * pitch: (s + 1) * h * pitch].reshape(h, pitch)[:, :w] = frames[s]
    dev = torch.from_numpy(buf).cuda()
    assert dev.data_ptr() % 16 == 0
    g.make_keyframe_lite_device(dev.data_ptr(), pitch, h * pitch)
    g.synchronize()
    return dev


def check(g, s, want, tag):
    for l, (img, corners, lut) in enumerate(want):
        got = g.read_corners(s, l)
        assert np.array_equal(g.read_level_image(s, l), img), (tag, s, l, "image")
        assert len(got) == len(corners), (tag, s, l, "count", len(got), len(corners))
        assert np.array_equal(got, corners), (tag, s, l, "corners")
        assert np.array_equal(g.read_row_lut(s, l), lut), (tag, s, l, "lut")


@pytest.mark.parametrize("kind", sorted(fc.KINDS))
@pytest.mark.parametrize("w,h,S,pad", fc.SHAPES)
def test_edge_frames_bit_exact(oracle, kind, w, h, S, pad):
    frames = fc.frames_of(kind, w, h, S)
    g = capi.System(capi.default_params(w, h, S))
    g.make_keyframe_lite(frames[::-1].copy() ^ 0x55)     # the buffers hold another frame's masks, counts and lists first
    g.make_keyframe_lite(frames[::-1].copy())
    keep = feed(g, frames, pad)
    for s in range(S):
        want = oracle.make_keyframe_lite(frames[s], fc.THR)
        assert all(len(c) > 0 for _, c, _ in want)
        check(g, s, want, (kind, w, h, pad))
    del keep
    g.close()


def test_corners_on_a_compaction_seam(oracle):
    """every level-0 corner in the last row of one compaction band or the first row of the next"""
    w, h = fc.SEAM_SHAPE
    img = fc.seam_image(w, h)
    frames = np.stack([img, img[:, ::-1].copy()])
    g = capi.System(capi.default_params(w, h, 2, fast_threshold=list(fc.SEAM_THR)))
    g.make_keyframe_lite(frames)
    for s in range(2):
        want = oracle.make_keyframe_lite(frames[s], fc.SEAM_THR)
        r = fc.compact_rows(w)
        assert set((want[0][1] >> 16).tolist()) == {r - 1, r} and all(len(c) > 0 for _, c, _ in want)
        check(g, s, want, "seam")
    g.close()


def test_empty_frame(oracle):
    w, h = 128, 65
    frames = np.full((2, h, w), 90, np.uint8)
    g = capi.System(capi.default_params(w, h, 2))
    g.make_keyframe_lite(fc.frames_of("edges", w, h, 2))  # full lists first: the empty frame has to take them down
    g.make_keyframe_lite(fc.frames_of("edges", w, h, 2))
    g.make_keyframe_lite(frames)
    for s in range(2):
        want = oracle.make_keyframe_lite(frames[s], fc.THR)
        assert all(len(c) == 0 for _, c, _ in want)
        check(g, s, want, "empty")
    g.close()


def test_overflow_clamps_and_is_reported(oracle):
    """more corners than the capacity: the flag is raised (reading the list fails) and the row LUT is the oracle's, clamped"""
    w, h, cap = 128, 56, 16
    frames = np.stack([fc.edges_image(5, w, h)])
    want = oracle.make_keyframe_lite(frames[0], fc.THR)
    assert len(want[0][1]) > cap
    g = capi.System(capi.default_params(w, h, 1, max_corners=[cap] * 4))
    g.make_keyframe_lite(frames)
    with pytest.raises(capi.VslamError):
        g.read_corners(0, 0)
    for l in range(4):
        assert np.array_equal(g.read_row_lut(0, l), np.minimum(want[l][2], cap)), l
    g.close()
