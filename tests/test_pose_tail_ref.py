"""CPU test of the reference side of tests/test_gpu_pose_tail.py: the Python transcription of lu_solve_n returns the bits of the
oracle's solve (orc::lu_solve, oracle/ptam_math.hpp, compiled here with the oracle's flags) on every case, and the cases are what
their names say."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_tail_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = """
#include "ptam_math.hpp"
extern "C" int shim_lu_solve(double* A, double* b, int n) { return orc::lu_solve(A, b, n) ? 1 : 0; }
"""


@pytest.fixture(scope="module")
def oracle_solve(tmp_path_factory):
    d = tmp_path_factory.mktemp("orc_solve")
    src, so = str(d / "shim.cpp"), str(d / "libshim.so")
    open(src, "w").write(SHIM)
    subprocess.check_call(["g++", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-std=c++17", "-shared", "-I", os.path.join(ROOT, "oracle"), src, "-o", so])
    lib = C.CDLL(so)

    def solve(Cm, v):
        A = np.array(Cm, np.float64).reshape(36).copy()
        b = np.array(v, np.float64).copy()
        ok = lib.shim_lu_solve(A.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), 6)
        return bool(ok), b
    return solve


@pytest.mark.parametrize("name", list(ref.CASES))
def test_transcription_returns_the_oracles_bits(oracle_solve, name):
    sums, _pose, _what = ref.CASES[name]
    Cm, v = ref.system_from_sums(sums)
    ok_o, x_o = oracle_solve(Cm, v)
    x_t, ok_t, _piv = ref.solve_update(sums)
    assert ok_o == ok_t
    if ok_o:
        assert np.array_equal(x_o.view(np.int64), x_t.view(np.int64)), (name, x_o, x_t)
    else:
        assert not x_t.any()


def test_cases_are_what_they_claim():
    assert {"spd", "swap_every_step", "tie_keeps_row", "tie_first_of_equals", "zero_column_first", "zero_column_later", "zero_vector",
            "rotation_1e-9", "rotation_near_pi"} <= set(ref.CASES)
    for name, (sums, _pose, what) in ref.CASES.items():
        x, ok, piv = ref.solve_update(sums)
        if what == "singular":
            assert not ok and not x.any(), name
            continue
        assert ok, name
        if what == "swaps":
            assert all(piv[k] != k for k in range(5)), (name, piv)
        elif what is not None:
            assert piv[:len(what)] == what, (name, piv)
    Cm, v = ref.system_from_sums(ref.CASES["spd"][0])
    x = np.linalg.solve(np.array(Cm).reshape(6, 6), np.array(v))
    assert np.allclose(x, ref.solve_update(ref.CASES["spd"][0])[0], rtol=1e-9, atol=0)
    assert not ref.solve_update(ref.CASES["zero_vector"][0])[0].any()
    for name, lo, hi in (("rotation_1e-9", 0.0, 1e-8), ("rotation_5e-4", 1e-8, 1e-6), ("rotation_2e-2", 1e-6, 1.0), ("rotation_near_pi", 9.8, 9.87)):
        w = ref.solve_update(ref.CASES[name][0])[0][3:]
        assert lo <= float(w @ w) < hi, (name, float(w @ w))


def test_pose_mul_is_the_matrix_product():
    rng = np.random.default_rng(2)
    a, b = rng.uniform(-1, 1, 12), rng.uniform(-1, 1, 12)
    r = ref.pose_mul(a, b)
    A, B = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
    assert np.allclose(r[:9].reshape(3, 3), A @ B, rtol=0, atol=1e-15) and np.allclose(r[9:], a[9:] + A @ b[9:], rtol=0, atol=1e-15)
