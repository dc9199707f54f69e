"""CPU: csrc/overlay_dev.h, the header the render kernel draws by, compiled for the host and held to tests/overlay_ref.py.
tests/overlay_dev_check.cpp is a stand-alone program with its own main; it is compiled here with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer (runtimes linked statically) and run as a plain program: nothing is loaded into Python, nothing is preloaded."""
import os
import shutil
import subprocess

import overlay_ref as ov

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_equals_the_numpy_restatement(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/overlay_dev_check.cpp"
    exe = str(tmp_path / "overlay_dev_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "overlay_dev_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [l.split() for l in r.stdout.splitlines()]
    n_lines = 0
    for rec in lines:
        if rec[0] == "L":
            dx, dy, n, h = (int(x) for x in rec[1:])
            p = ov.line_pixels(5, -3, 5 + dx, -3 + dy)
            want = 0
            for x, y in p.tolist():
                want = (want * 1000003 + (x + 100) * 65537 + (y + 100)) % (1 << 64)
            assert (n, h) == (len(p), want), (dx, dy)
            n_lines += 1
        elif rec[0] == "D":
            v = [int(x) for x in rec[1:]]
            assert v[0] == 21 and sorted(zip(v[1::2], v[2::2])) == sorted(map(tuple, ov.disc_pixels(0, 0).tolist()))
        elif rec[0] == "M":
            v = [int(x) for x in rec[1:]]
            assert sorted(zip(v[0::2], v[1::2])) == sorted(map(tuple, ov.mark_pixels(0, 0).tolist()))
        elif rec[0] == "C":
            v = [int(x) for x in rec[1:]]
            rgb = (ov.LEVEL_COLOURS + (ov.TRAIL_COLOUR, ov.MARK_COLOUR))[v[0]]
            assert tuple(v[1:5]) == rgb + (255,) and tuple(v[5:9]) == rgb + (0,), v
    assert n_lines == 81 * 81 and ["R", "ok"] in lines and sum(1 for rec in lines if rec[0] == "C") == 6
