"""CPU: csrc/similarity_dev.h, the header the transform kernel works by, compiled for the host and held to tests/transform_ref.py
bit for bit.  tests/similarity_check.cpp is a stand-alone program with its own main; it is compiled here for the host only, without
fused multiply-adds (as the library is), with AddressSanitizer and UndefinedBehaviorSanitizer on the host code (-Xarch_host: no device
code is built or instrumented), and run as a plain program: nothing
is loaded into Python, nothing is preloaded."""
import os
import subprocess

import numpy as np

import transform_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def cases():
    """[n, 31]: T (pose12), s, a point, a vector, a pose.  Random rotations about random axes and the named cases: s = 1, T = identity,
    s a power of two, a rotation by pi; poses and points of the sizes a map holds, and some far larger."""
    rng = np.random.default_rng(20240607)
    rows = []

    def add(R, t, s):
        C = tr.pose12(tr.rotation(rng.normal(size=3), rng.uniform(0, np.pi)), rng.normal(size=3) * rng.choice([0.1, 1.0, 50.0]))
        rows.append(np.concatenate([tr.pose12(R, t), [s], rng.normal(size=3) * rng.choice([0.01, 1.0, 1e3]), rng.normal(size=3) * 1e-3, C]))

    for _ in range(200):
        add(tr.rotation(rng.normal(size=3), rng.uniform(-np.pi, np.pi)), rng.normal(size=3) * 3, float(np.exp(rng.uniform(-3, 3))))
    for _ in range(20):
        add(tr.rotation(rng.normal(size=3), rng.uniform(-np.pi, np.pi)), rng.normal(size=3), 1.0)               # rigid
        add(np.eye(3), np.zeros(3), float(np.exp(rng.uniform(-3, 3))))                                        # a pure rescale
        add(np.eye(3), np.zeros(3), 1.0)                                                                      # nothing
        add(tr.rotation(rng.normal(size=3), rng.uniform(-np.pi, np.pi)), rng.normal(size=3), float(2.0 ** rng.integers(-4, 5)))
        add(tr.rotation(rng.normal(size=3), np.pi), rng.normal(size=3), float(np.exp(rng.uniform(-1, 1))))      # a half turn
    add(tr.rotation([0, 0, 1], np.pi), [1, 2, 3], 1.7)
    return np.array(rows)


def test_header_equals_the_numpy_restatement(tmp_path):
    assert os.path.exists(HIPCC), "hipcc is needed to build tests/similarity_check.cpp for the host"
    exe, fin, fout = str(tmp_path / "similarity_check"), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    subprocess.run([HIPCC, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Werror", os.path.join(ROOT, "tests", "similarity_check.cpp"), "-o", exe], check=True, cwd=ROOT)
    c = cases()
    c.tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.split() == ["cases", str(len(c))]
    got = np.fromfile(fout, np.float64).reshape(len(c), 44)
    T, s, p, v, C = c[:, :12], c[:, 12], c[:, 13:16], c[:, 16:19], c[:, 19:31]
    bad = 0
    for i in range(len(c)):
        accT, accs = tr.compose(T[i], s[i], C[i], abs(v[i, 0]) + 0.5)
        want = np.concatenate([tr.inverse(T[i]), tr.sim_point(T[i], s[i], p[i]), tr.sim_vector(T[i], s[i], v[i]), tr.sim_pose(T[i], s[i], C[i]),
                               [p[i, 0] * s[i]], accT, [accs]])
        bad += int((want.view(np.uint64) != got[i].view(np.uint64)).sum())
    assert bad == 0, bad
    # with s == 1 a length is untouched; with T the identity and s == 1 a point and a vector keep their bits (x * 1 + 0 + 0 is x, up to
    # the sign of a zero); with s a power of two the scaling is exact
    one = s == 1.0
    assert one.sum() >= 40 and np.array_equal(got[one, 30], p[one, 0])
    ident = one & (np.abs(T - tr.pose12(np.eye(3), np.zeros(3))).max(axis=1) == 0)
    assert ident.sum() >= 20 and np.array_equal(got[ident, 12:15], p[ident]) and np.array_equal(got[ident, 15:18], v[ident])
    assert np.array_equal(got[ident, 18:30], C[ident])
