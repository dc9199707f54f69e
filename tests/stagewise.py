"""The stage-wise comparison of tests/test_gpu_tracker_counts.py, tests/test_gpu_frame_tail.py and tests/test_gpu_template_edges.py: cases (tracker_cases.Case) as the streams
of one System, each beside its own oracle, compared with == after every search and pose stage and after the frame."""
import numpy as np

import tracker_cases as tc
from helpers import assert_tracker_exact, pose_err, resync
from visualslam_android_amd import capi


def assert_stage_exact(o, g, s, tag):
    """after a search or pose stage: counters, searched and found sets, positions and the pose estimate == the oracle's"""
    so, sg = o.state(), g.state(s)
    to, tg = o.point_tracks(), g.point_tracks(s)
    pv = tg["level"] >= 0
    assert np.array_equal(to["level"] >= 0, pv) and np.array_equal(to["level"][pv], tg["level"][pv]), tag
    assert np.array_equal(to["searched"], tg["searched"]) and np.array_equal(to["found"][pv], tg["found"][pv]), tag
    fnd = pv & (tg["found"] == 1)
    assert np.array_equal(to["vfound"][fnd], tg["vfound"][fnd]) and np.array_equal(to["image"][fnd], tg["image"][fnd]), tag
    assert list(so.attempted) == list(sg.attempted) and list(so.found) == list(sg.found), (tag, list(so.attempted), list(sg.attempted), list(so.found), list(sg.found))
    assert so.n_zmssd == sg.n_zmssd and so.did_coarse == sg.did_coarse, (tag, so.n_zmssd, sg.n_zmssd, so.did_coarse, sg.did_coarse)
    assert np.array_equal(np.array(so.pose[:]), np.array(sg.pose[:])), (tag, pose_err(so.pose, sg.pose))


def run_group(cases, patch, after_fine_pose=None, n_frames=tc.N_FRAMES, before_frame=None, after_stage=None):
    """the cases as the streams of one System, stage by stage against one oracle each.  before_frame(o, g, s, case, t) prepares both sides
    for frame t (a pose of the case's own, say); after_stage(o, g, s, tag) compares more after every search and pose stage."""
    S = len(cases)
    g = capi.System(cases[0].params(S, patch))
    assert all(c.pkw == cases[0].pkw and c.size == cases[0].size for c in cases)          # the parameters are system-wide
    oracles = []
    for s, c in enumerate(cases):
        c.load(g, s)
        oracles.append(c.oracle(patch))
    for t in range(n_frames):
        if before_frame:
            for s, (o, c) in enumerate(zip(oracles, cases)):
                before_frame(o, g, s, c, t)
        g.make_keyframe_lite(np.stack([c.frame(t) for c in cases]))
        for o, c in zip(oracles, cases):
            o.frame_begin(c.frame(t))
        for stage in (0, 1):
            g.patch_search(stage)
            for s, (o, c) in enumerate(zip(oracles, cases)):
                o.search_stage(stage)
                assert_stage_exact(o, g, s, "%s, %dx%d patches, frame %d, search %d" % (c.name, patch, patch, t, stage))
                if after_stage:
                    after_stage(o, g, s, "%s, %dx%d patches, frame %d, search %d" % (c.name, patch, patch, t, stage))
            g.pose_update(stage)
            for s, (o, c) in enumerate(zip(oracles, cases)):
                o.pose_stage(stage)
                assert_stage_exact(o, g, s, "%s, %dx%d patches, frame %d, pose %d" % (c.name, patch, patch, t, stage))
                if after_stage:
                    after_stage(o, g, s, "%s, %dx%d patches, frame %d, pose %d" % (c.name, patch, patch, t, stage))
        g.finish_frame()
        for s, (o, c) in enumerate(zip(oracles, cases)):
            o.frame_end()
            tag = "%s, %dx%d patches, frame %d" % (c.name, patch, patch, t)
            assert_tracker_exact(o, g, s, tag)
            if t == 0:
                for key in ("n_points", "did_coarse"):                                    # the case is the one the CPU test vouched for
                    if key in c.target:
                        assert getattr(g.state(s), key) == c.target[key], (tag, key)
            if after_fine_pose:
                after_fine_pose(o, g, s, tag)
            resync(o, g, s)
    for o in oracles:
        o.close()
    g.close()
