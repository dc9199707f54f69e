"""CPU: the numpy restatement the relocaliser's GPU tests compare against (tests/reloc_ref.py) is pinned to the oracle on both
branches of the SmallBlurryImage -- 9 taps and 17, two independent restatements that agree bit for bit -- and has the properties its
other half, the ZMSSD, must have."""
import numpy as np
import pytest

import reloc_ref
from helpers import make_scene
from oracle import binding as orc


def level3_images(w, h, seed, n=3):
    _f, m, frames = make_scene(w, h, seed=seed, n_frames=n, n_keyframes=2, per_level=(120, 50, 20, 8))
    return [orc.make_keyframe_lite(fr)[3][0] for fr in list(frames) + [k["image"] for k in m["keyframes"]]]


@pytest.mark.parametrize("w,h,seed", [(320, 240, 12), (640, 480, 31)])
@pytest.mark.parametrize("sigma", [0.75, 2.0])
def test_nine_tap_restatement_is_the_oracles(w, h, seed, sigma):
    for l3 in level3_images(w, h, seed):
        small, tmpl = reloc_ref.make_from_l3(l3, sigma, taps=9)
        wsmall, wtmpl = orc.sbi_make(l3, sigma)
        assert np.array_equal(small, wsmall)
        assert tmpl.dtype == np.float32 and np.array_equal(tmpl, wtmpl), float(np.abs(tmpl - wtmpl).max())


def smooth_level3(w3, h3, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h3, 0:w3]
    img = 120 + 50 * np.sin(x / 7.0 + 0.3) * np.cos(y / 5.0) + 30 * np.sin((x + 2 * y) / 11.0)
    return np.clip(img + rng.normal(0, 4.0, img.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("w3,h3", [(6, 6), (7, 9), (17, 15), (33, 17), (62, 62), (128, 66), (160, 90)])
@pytest.mark.parametrize("blur", [0.75, 2.0, 2.5, 4.0])
def test_both_branches_are_the_oracles_at_small_and_odd_sizes(w3, h3, blur):
    """numpy and C++ state the blur independently; they agree at both tap counts, at level-3 sizes whose last row and column are
    dropped, and at small images narrower than the 17 taps, which then reach past both borders at once"""
    l3 = smooth_level3(w3, h3, 100 * w3 + h3)
    small, tmpl = reloc_ref.make_from_l3(l3, blur)
    wsmall, wtmpl = orc.sbi_make(l3, blur)
    assert small.shape == (h3 // 2, w3 // 2) and np.array_equal(small, wsmall)
    assert tmpl.dtype == np.float32 and np.array_equal(tmpl, wtmpl), float(np.abs(tmpl - wtmpl).max())
    if blur > 2.0:                                                        # ... and the 17 taps are not the 9 with another sigma
        assert not np.array_equal(tmpl, reloc_ref.make_from_l3(l3, blur, taps=9)[1])


def test_branch_follows_the_blur():
    assert reloc_ref.taps_for(0.75) == 9 and reloc_ref.taps_for(2.0) == 9 and reloc_ref.taps_for(2.5) == 17   # jni/SmallBlurryImage.cc:51-54
    l3 = level3_images(320, 240, 12, 1)[0]
    t9, t17 = reloc_ref.make_from_l3(l3, 2.5, taps=9)[1], reloc_ref.make_from_l3(l3, 2.5)[1]
    assert t9.shape == t17.shape == (15, 20) and not np.array_equal(t9, t17)
    flat = np.full((30, 40), 77, np.uint8)
    assert np.abs(reloc_ref.make_from_l3(flat, 2.5)[1]).max() == 0.0


@pytest.mark.parametrize("taps,sigma", [(9, 0.75), (9, 2.0), (17, 2.5), (17, 4.0)])
def test_kernel_weights_sum_to_one_within_a_float_ulp(taps, sigma):
    k = reloc_ref.gauss_kernel(taps, sigma)
    assert k.dtype == np.float32 and len(k) == taps and np.array_equal(k, k[::-1]) and k[taps // 2] == k.max()
    # every weight is rounded to float once: the exact sum is within taps half-ulps of the weights, far less than one ulp of 1.0f
    assert abs(float(k.astype(np.float64).sum()) - 1.0) <= float(np.spacing(np.float32(1.0)))


def test_zmssd_properties():
    imgs = level3_images(320, 240, 77)
    t = [reloc_ref.make_from_l3(x, 2.5)[1] for x in imgs]
    for a in t:
        assert reloc_ref.zmssd(a, a) == 0.0
    for a in t:
        for b in t:
            assert reloc_ref.zmssd(a, b) == reloc_ref.zmssd(b, a)        # (a - b)^2 == (b - a)^2 term by term, same order
    assert reloc_ref.zmssd(t[0], t[1]) > 0.0
    # the order is the reference's: columns outer, rows inner
    d = (t[0] - t[1]).astype(np.float64)
    acc = 0.0
    for x in range(d.shape[1]):
        for y in range(d.shape[0]):
            acc += d[y, x] * d[y, x]
    assert acc == reloc_ref.zmssd(t[0], t[1])
    best, scores = reloc_ref.score_keyframes(t[0], [t[2], t[0], t[0], t[1]])
    assert best == 1 and scores[1] == 0.0 and scores[2] == 0.0           # the first strict minimum (jni/Relocaliser.cc:53)


def test_jacs_are_central_differences_with_a_zero_border():
    t = reloc_ref.make_from_l3(level3_images(320, 240, 12, 1)[0], 2.0)[1]
    j = reloc_ref.make_jacs(t)
    assert j.shape == t.shape + (2,) and j.dtype == np.float32
    assert j[5, 7, 0] == t[5, 8] - t[5, 6] and j[5, 7, 1] == t[6, 7] - t[4, 7]
    assert not j[0].any() and not j[-1].any() and not j[:, 0].any() and not j[:, -1].any()
