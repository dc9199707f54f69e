"""CPU: csrc/fuse_dev.h, the rule the fusion kernels work by, compiled for the host and held to tests/fuse_ref.py.
tests/fuse_rules_check.cpp is a stand-alone program with its own main; it is compiled here for the host only with AddressSanitizer and
UndefinedBehaviorSanitizer on the host code (-Xarch_host: no device code is built or instrumented) and run as a plain program: nothing is
loaded into Python, nothing is preloaded.  A few thousand random small cases, and the never-retry bit test at keyframe counts 63, 64, 65,
127 and 128 (a shift of a 64-bit word by 64 is undefined behaviour and the kind of defect this is for)."""
import os
import struct
import subprocess

import numpy as np

import fuse_ref as fr
from fuse_cases import random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
M64 = (1 << 64) - 1


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def cases():
    rng = np.random.default_rng(20251021)
    out = [random_case(rng, int(rng.integers(0, 6)), int(rng.integers(0, 9))) for _ in range(3000)]
    for nk in (63, 64, 65, 127, 128):                                # point 1 is point 0's copy everywhere it is measured; 2 is 0's too
        for trial in range(4):
            c = random_case(rng, nk, 3)
            c["root"][:] = 48.0
            c["level"][:] = 1
            c["bad"][:] = False
            c["valid"] = rng.random((nk, 3)) < 0.5
            c["valid"][:3, :] = True
            c["min_views"] = 2
            c["never_retry"] = [int(rng.integers(0, M64, dtype=np.uint64)) | (int(rng.integers(0, M64, dtype=np.uint64)) << 64) if trial else (1 << 128) - 1 for _ in range(3)]
            if trial == 1:
                c["never_retry"][0] = (1 << 63) | (1 << 64) | (1 << 127) | 1
            out.append(c)
    return out


def text_of(c):
    nk, n = c["valid"].shape
    lines = ["%d %d %d %d" % (nk, n, c["min_views"], bits(c["radius"]))]
    for k in range(nk):
        for i in range(n):
            lines.append("%d %d %d %d %d" % (c["valid"][k, i], c["level"][k, i], c["source"][k, i], bits(c["root"][k, i, 0]), bits(c["root"][k, i, 1])))
    for i in range(n):
        nr = c["never_retry"][i]
        lines.append("%d %d %d" % (c["bad"][i], nr & M64, nr >> 64))
    return "\n".join(lines) + "\n"


def test_header_equals_the_numpy_model(tmp_path):
    assert os.path.exists(HIPCC), "hipcc is needed to build tests/fuse_rules_check.cpp for the host"
    exe = str(tmp_path / "fuse_rules_check")
    subprocess.run([HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", os.path.join(ROOT, "tests", "fuse_rules_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    cs = cases()
    r = subprocess.run([exe], input="".join(text_of(c) for c in cs), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1].split() == ["cases", str(len(cs))]
    bad, n_pairs, n_taken, n_chained, n_never = [], 0, 0, 0, 0
    for ci, (c, line) in enumerate(zip(cs, lines)):
        want = fr.fuse_core(c["valid"], c["level"], c["root"], c["bad"], c["never_retry"], c["n_meas_kfs"], c["source"], c["radius"], c["min_views"])
        n = c["valid"].shape[1]
        into = [-1] * n
        for p, q in want["pairs"]:
            into[p] = q
        taken = sorted((k, q, p, int(want["source"][k, q])) for k, q, p in want["taken"])
        text = "P" + "".join(" %d" % x for x in want["partner"]) + " D" + "".join(" %d" % x for x in into) + " T" + \
            "".join(" %d %d %d %d" % t for t in taken) + " N %d" % want["info"]["not_taken"]
        if text != line:
            bad.append((ci, text, line))
        n_pairs += len(want["pairs"]); n_taken += len(taken); n_chained += want["info"]["chained"]
        n_never += sum(1 for p, q in want["pairs"] for k in range(c["valid"].shape[0]) if c["valid"][k, p] and not c["valid"][k, q] and (c["never_retry"][q] >> k) & 1)
    assert not bad, bad[:3]
    # the cases reach what they are for
    assert n_pairs > 500 and n_taken > 200 and n_chained > 20 and n_never > 50, (n_pairs, n_taken, n_chained, n_never)
