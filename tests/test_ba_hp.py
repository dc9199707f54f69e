"""CPU check of the extended-precision one-trial reference (tests/ba_hp.py) against the oracle's fp64 Bundle: the same first
Levenberg-Marquardt trial to ~1e-12 relative, so the yardstick of the fast summation mode is itself validated without a GPU."""
import numpy as np
import pytest

import ba_hp
from ba_paths_scene import CAM, HP_NFREE, hp_scene


def oracle_one_trial(oracle, sc):
    o = oracle.OracleBundle(CAM, 640, 480, max_iterations=1)
    for pose, fixed in zip(sc["cams_init"], sc["fixed"]):
        o.add_camera(pose, fixed)
    for p in sc["pts_init"]:
        o.add_point(p)
    for (c, p, xy, s2) in sc["meas"]:
        o.add_meas(c, p, xy, s2)
    acc = o.compute()
    return o, acc


@pytest.mark.parametrize("key", [str(n) for n in HP_NFREE] + ["config3"])
def test_extended_precision_trial_matches_oracle(oracle, key):
    sc = hp_scene(key)
    o, acc = oracle_one_trial(oracle, sc)
    hp = ba_hp.first_trial(CAM, 640, 480, sc["cams_init"], sc["fixed"], sc["pts_init"], sc["meas"])
    assert acc == 1 and hp["new_err"] < hp["cur_err"]                     # the first trial is accepted on both sides
    s2, lam, trials = o.stats()
    assert trials == 1 and abs(float(hp["sigma2"]) - s2) <= 1e-12 * s2        # err2 = (found - projection)^2 cancels ~300 px to ~1 px
    assert hp["n_free"] == (int(key) if key != "config3" else 4)
    for got, want in ((o.cameras(), hp["cams"]), (o.points(), hp["pts"])):
        rel = float(np.abs(np.asarray(got, dtype=np.longdouble) - want).max() / np.abs(want).max())
        assert rel < 1e-12, (key, rel)
    # the update itself (trial - start) agrees to ~1e-9 of its size: the comparison above is not only the start state's bits
    du_o = o.points() - sc["pts_init"]
    du_h = np.asarray(hp["pts"] - np.asarray(sc["pts_init"], dtype=np.longdouble), dtype=np.float64)
    assert np.abs(du_o - du_h).max() <= 1e-8 * np.abs(du_h).max()
