"""CPU: the frames of tests/frontend_reject_cases.py are worth comparing.  The oracle alone finds corners in every non-empty case at
every level (a GPU test that compares empty lists hides a failure), the seam frame's level-0 corners lie in the two rows it is named for,
and the overflow frame exceeds the capacity the GPU test gives it."""
import numpy as np
import pytest

import frontend_reject_cases as fc


@pytest.mark.parametrize("kind", sorted(fc.KINDS))
def test_every_level_has_corners(oracle, kind):
    for w, h, S, _ in fc.SHAPES:
        frames = fc.frames_of(kind, w, h, S)
        for s in range(S):
            for l, (_, corners, _) in enumerate(oracle.make_keyframe_lite(frames[s], fc.THR)):
                assert 0 < len(corners) < max(256, ((w >> l) * (h >> l)) // 2), (kind, w, h, s, l, len(corners))


def test_edge_frames_sit_on_the_predicate(oracle):
    """the edge-value frame holds compass differences of exactly t and t + 1, the gradient frame nothing else"""
    t = fc.THR[0]
    g = fc._walk(200, t, 0)
    assert set(np.abs(g[3:] - g[:-3]).tolist()) == {t, t + 1} and g.min() >= 0 and g.max() <= 120
    e = fc.edges_image(3, 128, 56).astype(int)
    d = np.abs(e[:, 3:] - e[:, :-3])
    assert (d == t).any() and (d == t + 1).any() and (d == t - 1).any() and (d == 255).any()


def test_seam_and_overflow_frames(oracle):
    w, h = fc.SEAM_SHAPE
    r = fc.compact_rows(w)
    want = oracle.make_keyframe_lite(fc.seam_image(w, h), fc.SEAM_THR)
    assert all(len(c) > 0 for _, c, _ in want)
    rows = set((want[0][1] >> 16).tolist())
    assert rows == {r - 1, r}, rows
    noisy = fc.edges_image(5, 128, 56)
    assert len(oracle.make_keyframe_lite(noisy, fc.THR)[0][1]) > 16
