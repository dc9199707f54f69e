"""The hand-built maps of tests/mapmaker_cases.py reach what they are named for, by the oracle alone (no GPU): the adjusted set, the fixed
set, the problem's point and measurement counts, the outlier list, the points that turn bad part-way through the outlier walk, the
never-retry bits of keyframes >= 64 and the return value.  tests/test_gpu_mapmaker_edges.py compares the device with the oracle on the
same cases; without this file a case could stop reaching its branch of k_ba_select / k_ba_assemble / k_ba_writeback unnoticed.

What a case wants comes from its construction (mapmaker_cases.problem_of, apply_outliers: plain restatements on the visibility matrix),
never from the oracle's answer.  One line per group is printed with the counts it reached."""
import numpy as np
import pytest

import mapmaker_cases as mc
from oracle import binding as orc


def meas_set(o, nk):
    return {(k, int(p)) for k in range(nk) for p in o.keyframe_meas(k, cap=4096)["pt"]}


def vis_of(case):
    m = case.map()
    v = np.zeros((len(m["keyframes"]), len(m["points"])), bool)
    for x in m["meas"]:
        v[x[0], x[1]] = True
    return v


def check_problem(lp, want, tag):
    if "adjusted" in want:
        assert lp["adjusted"] == list(want["adjusted"]), (tag, lp["adjusted"], want["adjusted"])
    if "fixed" in want:
        assert lp["fixed"] == list(want["fixed"]), (tag, lp["fixed"], want["fixed"])
    if "points" in want:
        assert np.array_equal(lp["points"], want["points"]), tag
    if "n_meas" in want:
        assert lp["n_meas"] == want["n_meas"], (tag, lp["n_meas"], want["n_meas"])
    if "n_meas_over" in want:
        assert lp["n_meas"] > want["n_meas_over"], (tag, lp["n_meas"])


def run_case(case):
    """-> the oracle left open, what it did per job (return value or None, the last problem if the job built one), and KeyFrameLinearDist of
    the case's tied keyframes on the loaded poses, before an adjustment moves them"""
    o = mc.oracle_for(case)
    nk, log = o.state().n_keyframes, []
    ties = [o.keyframe_linear_dist(case.want["tie"][0], k) for k in case.want["tie"][1]] if "tie" in case.want else None
    for job in case.jobs:
        runs = o.last_problem()["runs"]
        before = meas_set(o, nk) if "walk" in case.want and not log else None
        ret = mc.run_job(o, job)
        lp = o.last_problem()
        log.append({"job": job, "ret": ret, "lp": lp if lp["runs"] > runs else None, "before": before,
                    "after": meas_set(o, nk) if before is not None else None, "mm": o.point_mapmaker_data() if before is not None else None,
                    "bad": set(np.flatnonzero(o.points()["bad"]).tolist()), "queue": sorted(map(tuple, o.failure_queue().tolist()))})
    return o, log, ties


@pytest.mark.parametrize("group", mc.GROUPS)
def test_cases_reach_what_they_are_named_for(group):
    reached = []
    for case in mc.by_group(group):
        tag, want = case.name, case.want
        o, log, d = run_case(case)
        last = log[-1]
        if want.get("ran") is False:
            assert last["lp"] is None and last["ret"] == want["ret"], (tag, last["ret"])
            assert o.converged()[0] == 1, tag                                                  # :803-807 sets mbBundleConverged_Recent
        elif any(k in want for k in ("adjusted", "fixed", "points", "n_meas", "n_meas_over")):
            assert last["lp"] is not None, tag
            check_problem(last["lp"], want, tag)
        if "ret" in want:
            assert all(e["ret"] == want["ret"] for e in log), (tag, [e["ret"] for e in log])
        if "ret_first" in want:
            assert log[0]["ret"] == want["ret_first"] and log[0]["lp"]["accepted"] == want["ret_first"], (tag, log[0]["ret"])
        if "tie" in want:
            newest, ks = want["tie"]
            assert len({np.float64(x).tobytes() for x in d}) == 1, (tag, d)                    # equal bit for bit
            assert min(ks) in last["lp"]["adjusted"] and not set(ks[1:]) & set(last["lp"]["adjusted"]), (tag, last["lp"]["adjusted"])
        outl = set()
        for e in log:
            if e["lp"] is not None:
                outl |= {tuple(x) for x in e["lp"]["outliers"].tolist()}
        if "outliers" in want:
            assert outl == want["outliers"], (tag, len(outl), len(want["outliers"]), sorted(outl ^ want["outliers"])[:8])
        if "outliers_first_job" in want:
            assert {tuple(x) for x in log[0]["lp"]["outliers"].tolist()} == want["outliers_first_job"], tag
        if "n_outliers" in want:
            assert len(log[0]["lp"]["outliers"]) == want["n_outliers"], (tag, len(log[0]["lp"]["outliers"]))
        if "walk" in want:                                # the first job's walk over its outlier list == the plain model's
            e, w = log[0], want["walk"]
            assert e["lp"]["outliers"].tolist() == sorted(map(list, e["lp"]["outliers"].tolist())), tag     # one Bundle step rejected them all: keyframe-major order
            assert e["lp"]["bad_mid_walk"] == w["bad_mid_walk"], (tag, e["lp"]["bad_mid_walk"], w["bad_mid_walk"])
            assert e["bad"] == w["bad"] | {p for p, f in case.flags.items() if f[0]}, (tag, e["bad"], w["bad"])
            gone = e["before"] - e["after"]                # HandleBadPoints takes the bad points' measurements too
            assert {x for x in gone if x[1] not in e["bad"]} == {x for x in w["erased"] if x[1] not in e["bad"]}, tag
            assert e["queue"] == w["queue"], (tag, e["queue"][:5], w["queue"][:5])
            never = {(p, k) for p in range(len(e["mm"]["never_retry"])) for k in range(128) if (int(e["mm"]["never_retry"][p, k >> 6]) >> (k & 63)) & 1}
            assert never == w["never"], (tag, sorted(never)[:5], sorted(w["never"])[:5])
            vis = vis_of(case)
            nkfs = vis.sum(0) - np.array([sum(1 for x in w["erased"] if x[1] == p) for p in range(vis.shape[1])])
            assert np.array_equal(e["mm"]["n_meas_kfs"], nkfs), tag
        if "bad_mid_walk" in want:
            assert log[0]["lp"]["bad_mid_walk"] == want["bad_mid_walk"], tag
        if "never_retry_high" in want:
            nr = o.point_mapmaker_data()["never_retry"]
            high = {(p, 64 + k) for p in range(len(nr)) for k in range(64) if (int(nr[p, 1]) >> k) & 1}
            assert high == want["never_retry_high"], (tag, high)
        if "bad" in want:
            assert log[-1]["bad"] == want["bad"], (tag, log[-1]["bad"])
        if "idle" in want:
            st = o.idle_stats()
            assert {k: st[k] for k in want["idle"]} == want["idle"], (tag, st)
        if case.device_refuses:                           # the job that follows the device's refusal, on a fresh oracle (the device's map is untouched)
            o2 = mc.oracle_for(case)
            mc.run_job(o2, case.then)
            check_problem(o2.last_problem(), case.then_want, tag + " / then")
            o2.close()
        lp = last["lp"]
        reached.append("%s: %s" % (tag, "no problem (ret %s)" % last["ret"] if lp is None else
                                   "%d adjusted, %d fixed, %d points, %d measurements, %d outliers, %d bad part-way, accepted %d" %
                                   (len(lp["adjusted"]), len(lp["fixed"]), len(lp["points"]), lp["n_meas"], len(outl), sum(e["lp"]["bad_mid_walk"] for e in log if e["lp"]), lp["accepted"])))
        o.close()
    print("\n%s: %d cases\n  " % (group, len(reached)) + "\n  ".join(reached))


def test_outlier_lists_on_either_side_of_the_lds_copy():
    n = sorted(c.want["n_outliers"] for c in mc.by_group("write-back") if "n_outliers" in c.want)
    assert n == [mc.LDS_OUTLIERS, mc.LDS_OUTLIERS + 1]


def test_every_row_of_the_table_has_a_case():
    """the structural rows, on the cases' own construction (what each case reaches is asserted above)"""
    cs = {c.name: c for c in mc.cases()}
    nk = {name: len(c.map()["keyframes"]) for name, c in cs.items() if c.group == "select"}
    assert {64, 65, 128} <= set(nk.values())
    npts = sorted(len(c.map()["points"]) for c in mc.by_group("assemble") if c.name.startswith("n_points"))
    assert npts == [mc.BA_THREADS - 1, mc.BA_THREADS, mc.BA_THREADS + 1, 2 * mc.BA_THREADS + 1]
    walk = next(c for c in mc.by_group("write-back") if "outliers_first_job" in c.want)
    per_point = {}
    for k, p in walk.want["outliers_first_job"]:
        per_point[p] = per_point.get(p, 0) + 1
    assert {2, 3, 4} <= set(per_point.values())
    m = walk.map()
    src = {(x[0], x[1]): x[6] for x in m["meas"]}
    assert {src[kp] for kp in walk.want["outliers_first_job"]} == set(range(5))               # an outlier of every source
    jobs = {c.jobs[0] if len(c.jobs) == 1 else c.jobs for c in mc.by_group("bad points")}
    assert {"recent", "all", ("idle", 0)} <= jobs
    flags = set(mc.BAD_FLAGS.values())
    assert {(0, 5, 20), (0, 20, 20), (0, 30, 20), (0, 5, 21), (0, 21, 21), (0, 30, 21)} <= flags   # n_out 20 | 21 with n_in below, equal, above
    t = mc.batch_templates()
    assert mc.BATCH_STREAMS == 65 and len(t) == 5 and t[4].map() is None
    assert {mc.batch_template_of(s) for s in range(mc.BATCH_STREAMS)} == set(range(5))
    last = mc.batch_template_of(mc.BATCH_STREAMS - 1)        # the one stream of k_ba_select's second block must have work to do
    assert t[last].map() is not None and last in mc.BATCH_ORACLE_TEMPLATES


def test_project_is_the_oracles_camera():
    rng = np.random.default_rng(5)
    X = np.stack([rng.uniform(-1.5, 1.5, 50), rng.uniform(-1, 1, 50), rng.uniform(3.5, 4.5, 50)], 1)
    pose = np.concatenate([np.eye(3).ravel(), [0.1, -0.05, 0.2]])
    uv = mc.project(pose, X)
    cam = list(mc.capi.default_params(mc.W, mc.H).cam)
    for i in range(len(X)):
        c = X[i] + pose[9:]
        im, _d, _inv, _lr = orc.cam_project(cam, mc.W, mc.H, c[0] / c[2], c[1] / c[2])
        assert np.abs(im - uv[i]).max() < 1e-9, (i, im, uv[i])


def test_batch_templates_run_on_the_oracle():
    """the batch's maps under the batch's parameters: below the minimum, a tied window, outliers (the refused one has no oracle)"""
    t = mc.batch_templates()
    for i in mc.BATCH_ORACLE_TEMPLATES:
        o = mc.oracle_for(t[i])
        rets = [mc.run_job(o, j) for j in t[i].jobs]
        if i == 0:
            assert rets[0] == -2 and rets[2] == -2 and rets[1] >= 0, rets
        else:
            assert min(rets) >= 0, rets
        if i == 3:
            assert len(o.failure_queue()) > 0 and o.points()["bad"].sum() > 0
        if i == mc.batch_template_of(mc.BATCH_STREAMS - 1):   # stream 64's map: every job builds a problem, the first one has outliers to write back
            assert o.last_problem()["runs"] == len(t[i].jobs) and len(o.failure_queue()) > 0, o.last_problem()["runs"]
        o.close()
