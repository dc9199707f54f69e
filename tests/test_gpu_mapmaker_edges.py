"""The map-maker's driver kernels (csrc/ba.hip: k_ba_select, k_ba_assemble, k_ba_writeback with handle_bad_points) == the oracle on the
hand-built maps of tests/mapmaker_cases.py, which stand where those kernels branch (tests/test_mapmaker_cases.py shows on the oracle
alone that every case reaches its branch).  The stand-alone bundle tests (test_gpu_bundle_paths.py, test_gpu_ba_step_paths.py) go
through vslam_bundle_* and never run these three kernels; the sequence tests run them on natural scenes only.

With ba_sum_order = 1 everything is compared bit for bit after every job of a case: the state's counters, both converged flags, every
keyframe pose, the points (pos, bad, n_in, n_out), every keyframe's measurement rows, the idle statistics, the sizes of the assembled
problem, and -- through a stream snapshot, as they have no read-back of their own -- n_meas_kfs, the never-retry words and the failure
queue (sorted: the device's order is arbitrary by design).  Where the device refuses a problem the oracle has no limit for (more than
65536 measurements, more than 64 adjustable cameras in a BundleAdjustAll), ba_accepted is -3, the stream's snapshot is unchanged but
for that field, and a job that fits then equals the oracle.  With ba_sum_order = 0 the select and assemble groups (no corrupted
measurement: their structure is integer logic) must give the same structure exactly and poses and points within the 1e-8 of
test_gpu_bundle_paths.test_bundle_adjust_all_sixteen_keyframes.

No upload sets bad, n_in or n_out: the oracle takes them through set_point_flags, the device through a patched snapshot (patch_flags)."""
import re

import numpy as np
import pytest

import mapmaker_cases as mc
import retire_ref as rr
from helpers import pose_err
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

FAST_TOL = 1e-8


def patch_flags(g, s, flags):
    """bad, n_in and n_out of the given points, written into the stream's snapshot and restored"""
    if not flags:
        return
    h, secs = rr.sections(g.snapshot(s))
    rest = secs[rr.POINT_REST].reshape(h.n_points, rr.REST_BYTES).copy()
    for pt, (bad, n_in, n_out) in flags.items():
        rest[pt, rr.REST_BAD:rr.REST_BAD + 12] = np.array([bad, n_in, n_out], np.int32).view(np.uint8)     # bad, n_in, n_out are consecutive ints
    secs[rr.POINT_REST] = rest.reshape(-1)
    g.restore(s, rr.assemble(h, secs))


def load(g, s, case):
    if case.map() is None:
        return
    g.load_map(s, case.map())
    patch_flags(g, s, case.flags)


def device_record(g, s):
    st = g.state(s)
    h, secs = rr.sections(g.snapshot(s))
    ts = rr.TrackerState.from_buffer_copy(secs[rr.STATE].tobytes())
    n, nk = st.n_points, st.n_keyframes
    rest = secs[rr.POINT_REST].reshape(n, rr.REST_BYTES)
    rows = [g.keyframe_meas(s, k, cap=max(n, 1)) for k in range(nk)]
    return {"n_keyframes": nk, "n_points": n, "ba_accepted": st.ba_accepted, "n_ba_trials": st.n_ba_trials,
            "converged": (ts.ba_converged_recent, ts.ba_converged_full),
            "kf_poses": np.stack([g.keyframe_pose(s, k) for k in range(nk)]) if nk else np.zeros((0, 12)),
            "points": g.points(s), "rows": rows, "idle": g.idle_stats(s),
            "n_meas_kfs": rest[:, rr.REST_N_MEAS_KFS:rr.REST_N_MEAS_KFS + 4].copy().view(np.int32).reshape(-1),
            "never_retry": secs[rr.NEVER_RETRY].view(np.uint64).reshape(-1, 2), "queue": secs[rr.FAIL_QUEUE].view(np.int32).reshape(-1, 2).tolist(),
            "fq_n": ts.fq_n}


def oracle_record(o):
    st = o.state()
    n, nk = st.n_points, st.n_keyframes
    mm = o.point_mapmaker_data()
    return {"n_keyframes": nk, "n_points": n, "ba_accepted": st.ba_accepted, "n_ba_trials": st.n_ba_trials, "converged": o.converged(),
            "kf_poses": np.stack([o.keyframe_pose(k) for k in range(nk)]) if nk else np.zeros((0, 12)),
            "points": o.points(), "rows": [o.keyframe_meas(k, cap=max(n, 1)) for k in range(nk)], "idle": o.idle_stats(),
            "n_meas_kfs": mm["n_meas_kfs"], "never_retry": mm["never_retry"], "queue": sorted(o.failure_queue().tolist()), "fq_n": len(o.failure_queue())}


def assert_same(a, b, tag, tol=None, accepted=True):
    """a == b: every field bit for bit; with tol, poses and point positions within it and everything else exactly"""
    for key in ("n_keyframes", "n_points", "n_ba_trials", "converged", "idle", "fq_n", "queue") + (("ba_accepted",) if accepted else ()):
        assert a[key] == b[key], (tag, key, a[key], b[key])
    for key in ("bad", "n_in", "n_out"):
        assert np.array_equal(a["points"][key], b["points"][key]), (tag, key, np.flatnonzero(a["points"][key] != b["points"][key])[:8])
    assert np.array_equal(a["n_meas_kfs"], b["n_meas_kfs"]), (tag, np.flatnonzero(a["n_meas_kfs"] != b["n_meas_kfs"])[:8])
    assert np.array_equal(a["never_retry"], b["never_retry"]), (tag, np.flatnonzero((a["never_retry"] != b["never_retry"]).any(1))[:8])
    for k, (ra, rb) in enumerate(zip(a["rows"], b["rows"])):
        for key in ("pt", "level", "root", "source"):
            assert np.array_equal(ra[key], rb[key]), (tag, "measurement row", k, key, len(ra[key]), len(rb[key]))
    if tol is None:
        assert np.array_equal(a["kf_poses"], b["kf_poses"]), (tag, np.abs(a["kf_poses"] - b["kf_poses"]).max())
        assert np.array_equal(a["points"]["pos"], b["points"]["pos"]), (tag, np.abs(a["points"]["pos"] - b["points"]["pos"]).max())
    else:
        for k in range(a["n_keyframes"]):
            assert pose_err(a["kf_poses"][k], b["kf_poses"][k]) < tol, (tag, k, pose_err(a["kf_poses"][k], b["kf_poses"][k]))
        assert a["n_points"] == 0 or np.abs(a["points"]["pos"] - b["points"]["pos"]).max() < tol, (tag, np.abs(a["points"]["pos"] - b["points"]["pos"]).max())


def assert_problem_sizes(g, s, lp, tag):
    """the sizes of the problem k_ba_assemble built == the oracle's"""
    bs = g.bundle_stats(s)
    n_free = sum(1 for k in lp["adjusted"] if not lp["kf_fixed"][k])
    want = {"cams": len(lp["adjusted"]) + len(lp["fixed"]), "free_cams": n_free, "points": len(lp["points"]), "meas": lp["n_meas"]}
    assert {k: bs[k] for k in want} == want, (tag, bs, want)


def run_both(case, o, g, s, job, tag, tol=None):
    """one job on both sides, then everything compared"""
    runs = o.last_problem()["runs"]
    ret = mc.run_job(o, job)
    mc.run_job(g, job, stream=s)
    a, b = oracle_record(o), device_record(g, s)
    lp = o.last_problem()
    built = lp["runs"] > runs
    assert_same(a, b, tag, tol, accepted=built)
    if ret is not None:
        assert b["ba_accepted"] == ret, (tag, b["ba_accepted"], ret)
    if built:
        lp["kf_fixed"] = [bool(k["fixed"]) for k in case.map()["keyframes"]]
        assert_problem_sizes(g, s, lp, tag)


def state_but_accepted(sec):
    st = rr.TrackerState.from_buffer_copy(sec.tobytes())
    acc = st.ba_accepted
    st.ba_accepted = 0
    return bytes(st), acc


def run_case(case, mode, tol=None):
    o = mc.oracle_for(case, ba_sum_order=mode)
    g = capi.System(case.params(ba_sum_order=mode))
    load(g, 0, case)
    try:
        assert_same(oracle_record(o), device_record(g, 0), case.name + " / loaded", accepted=False)
        jobs = case.jobs[:-1] if case.device_refuses else case.jobs
        for i, job in enumerate(jobs):
            run_both(case, o, g, 0, job, "%s / job %d %s" % (case.name, i, job), tol)
        if case.device_refuses:
            before = g.snapshot(0).copy()
            trials = g.state(0).n_ba_trials
            mc.run_job(g, case.jobs[-1], stream=0)
            after = g.snapshot(0)
            st = g.state(0)
            assert st.ba_accepted == -3 and st.n_ba_trials == trials, (case.name, st.ba_accepted, st.n_ba_trials, trials)
            (hb, sb), (ha, sa) = rr.sections(before), rr.sections(after)
            assert bytes(hb) == bytes(ha), case.name
            for i in range(rr.N_SECTIONS):
                if i != rr.STATE:
                    assert np.array_equal(sb[i], sa[i]), (case.name, "snapshot section", i)
            assert state_but_accepted(sb[rr.STATE])[0] == state_but_accepted(sa[rr.STATE])[0] and state_but_accepted(sa[rr.STATE])[1] == -3, case.name
            o.close()
            o = mc.oracle_for(case, ba_sum_order=mode)         # the oracle of the untouched map: the job that fits
            for job in jobs:
                mc.run_job(o, job)
            run_both(case, o, g, 0, case.then, case.name + " / after the refusal: " + str(case.then), tol)
    finally:
        g.close()
        o.close()


def _ids(cases):
    return [re.sub(r"[^A-Za-z0-9]+", "_", c.name).strip("_") for c in cases]


@pytest.mark.parametrize("case", mc.by_group("select"), ids=_ids(mc.by_group("select")))
def test_select(case):
    run_case(case, 1)


@pytest.mark.parametrize("case", mc.by_group("assemble"), ids=_ids(mc.by_group("assemble")))
def test_assemble(case):
    run_case(case, 1)


@pytest.mark.parametrize("case", mc.by_group("capacity"), ids=_ids(mc.by_group("capacity")))
def test_capacity(case):
    run_case(case, 1)


@pytest.mark.parametrize("case", mc.by_group("write-back"), ids=_ids(mc.by_group("write-back")))
def test_writeback(case):
    run_case(case, 1)


@pytest.mark.parametrize("case", mc.by_group("bad points"), ids=_ids(mc.by_group("bad points")))
def test_bad_points(case):
    run_case(case, 1)


FAST = [c for c in mc.cases() if c.fast]


@pytest.mark.parametrize("case", FAST, ids=_ids(FAST))
def test_fast_sums_same_structure(case):
    """ba_sum_order = 0: the same problem, the same counters and measurement rows; poses and points within FAST_TOL"""
    assert case.group in ("select", "assemble")
    run_case(case, 0, FAST_TOL)


def test_batch_of_65_streams():
    """65 streams with mixed maps in one system: every stream == the same map adjusted alone in a one-stream system, bit for bit, after every
    job; three of them are also held against the oracle"""
    t = mc.batch_templates()
    S = mc.BATCH_STREAMS
    alone = {}
    for i, case in enumerate(t):
        g1 = capi.System(case.params(1))
        load(g1, 0, case)
        recs = []
        o = mc.oracle_for(case) if i in mc.BATCH_ORACLE_TEMPLATES else None
        for j, job in enumerate(mc.BATCH_JOBS):
            mc.run_job(g1, job, stream=0)
            recs.append(device_record(g1, 0))
            if o is not None:
                ret = mc.run_job(o, job)
                assert_same(oracle_record(o), recs[-1], "%s / alone, job %d" % (case.name, j), accepted=ret is None or ret >= -1)
                assert recs[-1]["ba_accepted"] == ret, (case.name, j, recs[-1]["ba_accepted"], ret)
        if o is not None:
            o.close()
        g1.close()
        alone[i] = recs
    assert alone[1][1]["ba_accepted"] == -3 and alone[1][0]["ba_accepted"] >= 0 and alone[1][2]["ba_accepted"] >= 0   # the refused BundleAdjustAll between two Recents
    assert alone[0][0]["ba_accepted"] == -2
    g = capi.System(t[0].params(S))
    try:
        for s in range(S):
            load(g, s, t[mc.batch_template_of(s)])
        for j, job in enumerate(mc.BATCH_JOBS):
            mc.run_job(g, job, stream=0)
            for s in range(S):
                assert_same(alone[mc.batch_template_of(s)][j], device_record(g, s), "stream %d (%s), job %d" % (s, t[mc.batch_template_of(s)].name, j))
    finally:
        g.close()
