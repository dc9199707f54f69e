"""CPU: csrc/snapshot_format.h, the host layout code behind vslam_snapshot_info and both planners of snapshot.hip, under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/snapshot_format_check.cpp is a stand-alone program with its own main: it builds
the section table for sizes 48 x 48 .. 4096 x 4096, 0 .. the format's largest keyframe and point counts and every combination of the
optional parts, round-trips each through the validator, feeds the validator every truncation length of one header, and headers with
each offset, size and count field pushed past the end.  It is compiled here with g++, the sanitizers' runtimes linked statically, and run as a plain program:
nothing is loaded into Python and nothing is preloaded."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_code_is_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/snapshot_format_check.cpp"
    exe = str(tmp_path / "snapshot_format_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "snapshot_format_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert int(r.stdout.split()[1]) > 10000
