"""Frames for the strip kernel's packed quick reject and the wavefront compaction (tests/test_gpu_frontend_reject.py compares them on the
GPU, tests/test_frontend_reject_cases.py checks on the CPU that the oracle finds corners in them at every level).  Pure numpy, seeded."""
import numpy as np

THR = (10, 15, 15, 10)                   # vslam_default_params
COMPACT_WORDS = 256                      # frontend.hip: a compaction band is 256 // nchunk rows of nchunk = ceil(w / 64) mask words


def compact_rows(w):
    return COMPACT_WORDS // ((w + 63) // 64)


def edge_values(t):
    return np.array([0, 1, t - 1, t, t + 1, 128, 254 - t, 255 - t, 254, 255], np.uint8)


def anchors(img, seed):
    """8x8 squares of 255 in the middle of flat 24x24 patches of 0, aligned to 8 and inside the rows and columns FAST looks at on level 3:
    their corners are FAST corners on level 0 and each square is still one bright pixel on level 3, so no level's list is empty"""
    h, w = img.shape
    rng = np.random.default_rng(1000 + seed)
    for _ in range(3):
        x3, y3 = int(rng.integers(3, (w >> 3) - 3)), int(rng.integers(3, max(4, (h >> 3) - 3)))
        img[8 * y3 - 8: 8 * y3 + 16, 8 * x3 - 8: 8 * x3 + 16] = 0
        img[8 * y3: 8 * y3 + 8, 8 * x3: 8 * x3 + 8] = 255
    return img


def edges_image(seed, w, h, t=THR[0]):
    """every pixel drawn from the values on the predicate's edges: differences of exactly 0, 1, t - 1, t, t + 1, ... between a centre and
    its compass pixels, and so many quick-reject survivors that a round of the strip kernel overflows its list and goes row by row"""
    rng = np.random.default_rng(seed)
    return anchors(edge_values(t)[rng.integers(0, 10, size=(h, w))], seed)


def checker_image(seed, w, h):
    """0 / 255 checkerboard: every compass pixel differs from its centre by 255, every pixel survives the quick reject, none is a corner"""
    yy, xx = np.mgrid[0:h, 0:w]
    return anchors((((xx + yy) & 1) * 255).astype(np.uint8), seed)


def _walk(n, t, phase):
    """f with f[i + 3] - f[i] alternately t and t + 1 in absolute value, kept inside 0..120 by turning round"""
    f = np.zeros(n + 3, np.int64)
    for r in range(3):
        v, sign, k = 40 * r, 1, phase + r
        for i in range(r, n + 3, 3):
            f[i] = v
            step = t + (k & 1)
            k += 1
            if not 0 <= v + sign * step <= 120:
                sign = -sign
            v += sign * step
    return f[:n]


def gradient_image(seed, w, h, t=THR[0]):
    """f(x) + g(y): a pixel and each of its four compass pixels differ by exactly t or t + 1, the two sides of the predicate's '> t'"""
    img = (_walk(w, t, seed)[None, :] + _walk(h, t, seed + 1)[:, None]).astype(np.uint8)
    return anchors(img, seed)


KINDS = {"edges": edges_image, "checker": checker_image, "gradient": gradient_image}

# (w, h, streams, row padding of a device source or None for host input).  Level widths / heights:
SHAPES = [
    (128, 56, 1, None),                  # 128 64 32 16 / 56 28 14 7: the smallest strip-form frame, level 3 sixteen wide and seven high
    (128, 63, 3, None),                  # 63 31 15 7: a strip ends inside a nine-row round
    (128, 65, 1, 16),                    # 65 32 16 8, padded pitch (still the strip form)
    (384, 72, 3, None),                  # 384 192 96 48 / 72 36 18 9
    (256, 128, 1, None),                 # 256 128 64 32 / 128 64 32 16
    (132, 65, 3, None),                  # 132 66 33 16: the band form in front of the wavefront compaction
    (132, 65, 1, 4),                     # the same from a device source with a padded pitch
]


def frames_of(kind, w, h, S):
    return np.stack([KINDS[kind](7 * s + len(kind), w, h) for s in range(S)])


def seam_image(w, h):
    """level-0 corners only in the last row of the first compaction band and the first row of the second: 2x2 squares of 255 on 0 across
    that seam (each of the four pixels is an isolated-dot corner).  With thresholds (10, 15, 15, 5) the squares' means 128, 32 and 8
    are corners on levels 1..3 too."""
    r = compact_rows(w)
    assert r + 16 <= h and r % 8 == 0
    img = np.zeros((h, w), np.uint8)
    for x in range(8, w - 8, 16):
        img[r - 1: r + 1, x: x + 2] = 255
    return img


SEAM_THR = (10, 15, 15, 5)
SEAM_SHAPE = (128, 264)                  # two mask words a row: bands of 128 rows, three bands on level 0
