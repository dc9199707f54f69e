"""GPU test: the radix select behind the Tukey median (csrc/dev_math.h block_radix_select, run by vslam_eval_select in the tracker's
workgroup with the values in LDS and in the bundle adjustment's with the values in device memory) returns the order statistic that
numpy.partition returns, bit for bit, at the sizes where its loops and batches split and on contents that stress its digits."""
import numpy as np
import pytest

from visualslam_android_amd import capi

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096, 4097, 16000)   # 4097: the bundle adjustment's BATCH = 16 form
LDS_CAP = 4096                                                                          # form 0 holds the values in LDS


def u2d(bits):
    return np.asarray(bits, np.uint64).view(np.float64)


def all_equal(rng, n, k):
    return np.full(n, 3.0625)


def two_values(rng, n, k):
    return np.where(rng.integers(0, 2, n) == 0, 0.75, 0.7500000000000001)


def both_sides_of_two(rng, n, k):                    # bit 62 differs
    return rng.uniform(0.5, 8.0, n)


def zeros_and_denormals(rng, n, k):
    v = u2d(rng.integers(0, 1 << 20, n))             # denormals
    v[rng.integers(0, 3, n) == 0] = 0.0
    v[rng.integers(0, 5, n) == 0] = 1e-3
    return v


def run_around_k(rng, n, k):
    v = np.sort(10.0 ** rng.uniform(-6, 4, n))
    v[max(0, k - 40):k + 41] = v[k]
    return rng.permutation(v)


def third_infinite(rng, n, k):                       # the bundle adjustment's markers: never selected (k counts the finite ones)
    v = 10.0 ** rng.uniform(-6, 4, n)
    v[rng.permutation(n)[:n // 3]] = np.inf
    return v


def lowest_byte(rng, n, k):                          # equal down to the lowest mantissa byte
    return u2d(np.uint64(0x4008123456789A00) + rng.integers(0, 256, n).astype(np.uint64))


def lowest_byte_wide(rng, n, k):                     # the same cluster inside a wide range: every digit is walked down to the last byte
    v = lowest_byte(rng, n, k)
    if n >= 3:
        v[0] = 1e-6; v[n - 1] = 1e4
    return v


CONTENTS = (all_equal, two_values, both_sides_of_two, zeros_and_denormals, run_around_k, third_infinite, lowest_byte, lowest_byte_wide)


@pytest.mark.gpu
@pytest.mark.parametrize("content", CONTENTS, ids=lambda f: f.__name__)
def test_select_returns_numpys_order_statistic(content):
    rng = np.random.default_rng(7)
    bad = []
    for n in SIZES:
        nsel = n - n // 3 if content is third_infinite else n          # the entries that can be selected
        for k in sorted({0, nsel // 2, nsel - 1}):
            v = content(rng, n, k)
            assert (v >= 0).all() and np.isfinite(v).sum() == nsel
            want = np.partition(v, k)[k]
            for form in (0, 1):
                if form == 0 and n > LDS_CAP:
                    continue
                got = capi.eval_select(v, k, form)
                if np.float64(got).view(np.int64) != np.float64(want).view(np.int64):
                    bad.append((n, k, form, got, want))
    print(content.__name__, "mismatches", len(bad))
    assert not bad, bad[:8]
