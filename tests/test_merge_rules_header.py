"""CPU: csrc/merge_dev.h, the index rules the merge kernel works by, compiled for the host and held to tests/merge_ref.py bit for bit.
tests/merge_rules_check.cpp is a stand-alone program with its own main; it is compiled here for the host only with AddressSanitizer and
UndefinedBehaviorSanitizer on the host code (-Xarch_host: no device code is built or instrumented) and run as a plain program: nothing is
loaded into Python, nothing is preloaded.  A shift of a 64-bit word by 64 is undefined behaviour and the kind of defect this is for: the
keyframe counts 0, 1, 63, 64, 65, 127 and 128 are all among the cases, on both sides."""
import itertools
import os
import subprocess

import numpy as np

import merge_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
M64 = (1 << 64) - 1


def cases():
    """rows of (w0, w1, nk_s, nk_d, flags, k, p, np_d, stored_d, j, fq_cap, fq_n, max_points)"""
    rng = np.random.default_rng(20250611)
    ends = (1, 1 << 63, (1 << 63) | 1, M64, 0)                       # bits at both ends of a word
    sets = [(a, b) for a in ends for b in ends] + [(int(rng.integers(0, M64, dtype=np.uint64)), int(rng.integers(0, M64, dtype=np.uint64))) for _ in range(6)]
    counts = (0, 1, 63, 64, 65, 127, 128)
    rows = []
    for (w0, w1), nk_s, nk_d in itertools.product(sets, counts, counts):
        cap = int(rng.choice([1, 7, 8192]))
        rows.append((w0, w1, nk_s, nk_d, int(rng.integers(64)), int(rng.integers(128)), int(rng.integers(4096)), int(rng.integers(4096)),
                     int(rng.integers(cap + 1)), int(rng.integers(cap + 1)), cap, int(rng.integers(-2, 2 * cap + 2)), int(rng.integers(1, 5000))))
    for flags in range(64):                                          # every combination of the six flag bits
        rows.append((0, 0, 1, 1, flags, 0, 0, 0, 0, 0, 8192, 0, 1))
    for stored_d, j, cap, fq_n in ((0, 0, 1, 0), (0, 1, 1, 1), (8191, 0, 8192, 8192), (8191, 1, 8192, 8193), (8192, 0, 8192, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1, 8192, -1)):
        rows.append((0, 0, 3, 2, 0, 127, 2 ** 24 - 1, 2 ** 24, stored_d, j, cap, fq_n, 2 ** 25))
    return rows


def test_header_equals_the_numpy_restatement(tmp_path):
    assert os.path.exists(HIPCC), "hipcc is needed to build tests/merge_rules_check.cpp for the host"
    exe = str(tmp_path / "merge_rules_check")
    subprocess.run([HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", os.path.join(ROOT, "tests", "merge_rules_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    c = cases()
    text = "".join(" ".join(str(x) for x in row) + "\n" for row in c)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1].split() == ["cases", str(len(c))]
    bad = []
    for row, line in zip(c, lines):
        w0, w1, nk_s, nk_d, flags, k, p, np_d, stored_d, j, cap, fq_n, maxp = row
        got = tuple(int(x) for x in line.split())
        slot = stored_d + j
        want = mr.shift_set(w0, w1, nk_s, nk_d) + (flags & mr.KEEP_FLAGS,) + mr.queue_entry(k, p, nk_d, np_d) + \
            (slot if slot < cap else -1, min(max(fq_n, 0), cap), (nk_d + k) * maxp + np_d + p)
        if got != want:
            bad.append((row, got, want))
    assert not bad, bad[:5]
    # the named properties: nothing above the source's count comes along; a shift by 0 is the identity on the masked set; by 64 the low
    # word becomes the high word
    assert mr.shift_set(M64, M64, 64, 0) == (M64, 0) and mr.shift_set(M64, M64, 128, 64) == (0, M64) and mr.shift_set(1, 0, 1, 127) == (0, 1 << 63)
    assert mr.shift_set(M64, M64, 0, 5) == (0, 0) and mr.shift_set(1 << 63, 1, 65, 1) == (0, 3)
