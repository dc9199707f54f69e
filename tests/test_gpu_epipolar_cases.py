"""GPU parity of the epipolar line geometry and the triangulation on the synthetic cases of tests/epipolar_cases.py: what
vslam_eval_epipolar returns -- epipolar_line, reproject_vector and reproject_point of csrc/grow_dev.h, the device functions k_epipolar
and the stereo bootstrap run -- must equal what the oracle's twins return (oracle/mapgrow.cpp: the function its AddPointEpipolar runs),
every integer and every double, bit for bit, a NaN for a NaN.  The oracle's side is held to 50 digits by tests/test_epipolar_cases.py.

A handle carries one calibration, so each camera of epipolar_cases.CAMS (two lenses, the pincushion one, and the reference's with
quirks = 1, where largest_radius is 0) gets a 64x48 system of three streams of its own; one launch per system evaluates its line cases and
every triangulation case."""
import numpy as np
import pytest

import cam_cases as cc
import epipolar_cases as ec
import oracle.binding as orc
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("cam", ec.CAMS, ids=[ec.cam_key(c) for c in ec.CAMS])
def test_device_record_is_the_oracle_twin_bit_for_bit(cam):
    cam5 = cc.CALIBRATIONS[cam[0]]
    cases, rows = ec.line_rows(cam)
    tcases, trows = ec.tri_rows()
    assert len(rows) + len(trows) > 64                                    # more than one workgroup, and one that holds both kinds
    want_flags, want_out = orc.eval_epipolar(cam5, ec.W, ec.H, rows, quirks=cam[1])
    want_tri = orc.eval_triangulation(trows)
    g = capi.System(capi.default_params(ec.W, ec.H, 3, cam=cam5, quirks=cam[1]))
    try:
        flags, out, tri = g.eval_epipolar(rows, trows)
        alone = g.eval_epipolar(lines=rows[:5])                            # either kind on its own, and nothing at all
        talone = g.eval_epipolar(tri=trows[-3:])
        nothing = g.eval_epipolar()
    finally:
        g.close()
    bad = np.flatnonzero((flags != want_flags).any(1))
    assert len(bad) == 0, [(cases[i], flags[i].tolist(), want_flags[i].tolist()) for i in bad[:8]]
    same = _same_bits(out, want_out)
    assert same.all(), [(cases[i], out[i].tolist(), want_out[i].tolist()) for i in np.flatnonzero(~same.all(1))[:4]]
    same = _same_bits(tri, want_tri)
    assert same.all(), [(tcases[i], tri[i].tolist(), want_tri[i].tolist()) for i in np.flatnonzero(~same.all(1))[:4]]
    assert np.array_equal(alone[0], want_flags[:5]) and _same_bits(alone[1], want_out[:5]).all() and alone[2].shape == (0, 7)
    assert _same_bits(talone[2], want_tri[-3:]).all() and talone[0].shape == (0, 2)
    assert nothing[0].shape == (0, 2) and nothing[1].shape == (0, capi.EPI_LINE_DOUBLES) and nothing[2].shape == (0, 7)


def test_eval_epipolar_turns_bad_arguments_away():
    g = capi.System(capi.default_params(ec.W, ec.H, 2))
    try:
        row = ec.line_rows(ec.CAMS[0])[1][:1].copy()
        for level in (-1.0, 4.0, 0.5, np.nan):
            row[0, 26] = level
            with pytest.raises(capi.VslamError, match="level"):
                g.eval_epipolar(lines=row)
    finally:
        g.close()
