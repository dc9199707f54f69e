"""numpy restatement of the relocaliser's image arithmetic, used only by the tests (the oracle has no relocaliser; its
SmallBlurryImage, oracle/sbi.cpp, is a second statement of the same blur in C++):

  * SmallBlurryImage::MakeFromKF (jni/SmallBlurryImage.cc:20-55) with either branch of :51-54, cv::GaussianBlur(9x9) for
    dBlur <= 2 and (17x17) above, restated as oracle/sbi.cpp restates it: cv::getGaussianKernel's weights (exp in
    double, stored and normalised in float) and a row pass then a column pass with a replicated border, every pixel
    k[c]*x0 + sum_j k[c+j]*(x[+j] + x[-j]) accumulated tap by tap in float32;
  * MakeJacs (:58-79);
  * SmallBlurryImage::ZMSSD (:82-94): the difference in float32, squared and summed in float64, columns outer, rows inner.

test_reloc_ref.py pins both forms to orc.sbi_make bit for bit."""
import math

import numpy as np


def taps_for(blur):
    return 9 if blur <= 2.0 else 17                                   # jni/SmallBlurryImage.cc:51-54


def gauss_kernel(taps, sigma):
    """cv::getGaussianKernel(taps, sigma, CV_32F)"""
    half = taps // 2
    scale2x = -0.5 / (sigma * sigma)
    k = np.array([np.float32(math.exp(scale2x * (i - float(half)) * (i - float(half)))) for i in range(taps)], np.float32)
    total = 0.0
    for v in k:
        total += float(v)
    inv = 1.0 / total
    return np.array([np.float32(float(v) * inv) for v in k], np.float32)


def halfsample(img):
    a = img.astype(np.uint32)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def _pass(t, k, axis):
    half = len(k) // 2
    n = t.shape[axis]
    idx = np.arange(n)
    take = lambda i: np.take(t, np.clip(i, 0, n - 1), axis=axis)
    acc = k[half] * t
    for j in range(1, half + 1):
        acc = acc + k[half + j] * (take(idx + j) + take(idx - j))
        assert acc.dtype == np.float32
    return acc


def make_from_l3(level3, blur, taps=None):
    """-> (mimSmall u8, mimTemplate float32)"""
    l3 = np.ascontiguousarray(level3, np.uint8)
    h3, w3 = l3.shape
    small = halfsample(l3[:h3 // 2 * 2, :w3 // 2 * 2])
    mean = np.float32(int(small.sum(dtype=np.uint64)) & 0xFFFFFFFF) / np.float32(small.size)
    t = small.astype(np.float32) - mean
    k = gauss_kernel(taps or taps_for(blur), blur)
    return small, _pass(_pass(t, k, 1), k, 0)


def make_jacs(tmpl):
    j = np.zeros(tmpl.shape + (2,), np.float32)
    j[1:-1, 1:-1, 0] = tmpl[1:-1, 2:] - tmpl[1:-1, :-2]
    j[1:-1, 1:-1, 1] = tmpl[2:, 1:-1] - tmpl[:-2, 1:-1]
    return j


def zmssd(a, b):
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float64)
    sq = (d * d).T.reshape(-1)                                         # x outer, y inner
    return float(np.cumsum(sq)[-1])                                    # cumsum adds one after the other


def score_keyframes(cur_tmpl, kf_tmpls):
    """Relocaliser::ScoreKFs (jni/Relocaliser.cc:46-58) -> (mnBest, every ZMSSD)"""
    scores = np.array([zmssd(cur_tmpl, t) for t in kf_tmpls])
    best, best_score = -1, 99999999999999.9
    for i, s in enumerate(scores):
        if s < best_score:
            best, best_score = i, s
    return best, scores
