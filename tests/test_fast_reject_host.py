"""CPU: csrc/fast_reject_dev.h, the packed quick reject of the FAST strip kernel, compiled for the host and held to the predicate in
plain integers.  tests/fast_reject_check.cpp is a stand-alone program with its own main; it is compiled here with g++ twice, plain and
under AddressSanitizer and UndefinedBehaviorSanitizer (runtimes linked statically), and run as a plain program: nothing is loaded into
Python, nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_DWORDS = 256 * 5 * 11 ** 4   # centres x thresholds x four compass pixels of eleven values each
N_ROWS = 5 * 40000


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]],
                         ids=["plain", "sanitized"])
def test_packed_reject_equals_the_plain_predicate(tmp_path, flags):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/fast_reject_check.cpp"
    exe = str(tmp_path / "fast_reject_check")
    subprocess.run([cxx, "-std=c++17", *flags, "-Wall", "-Werror", os.path.join(ROOT, "tests", "fast_reject_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    r4 = [l for l in lines if l[0] == "R4"][0]
    r16 = [l for l in lines if l[0] == "R16"][0]
    # every case was run, and both answers occur often: a check that only ever saw "reject" would prove little
    assert int(r4[1]) == N_DWORDS and 0.05 * 4 * N_DWORDS < int(r4[2]) < 0.95 * 4 * N_DWORDS, r4
    assert int(r16[1]) == N_ROWS and 0.05 * 16 * N_ROWS < int(r16[2]) < 0.95 * 16 * N_ROWS, r16
    assert ["ok"] in lines
