"""CPU checks of many_stream_cases.py: the restatement of the front end's strip-height choice, pinned to the figures it gives for 256
compute units; the replication pattern; the streams and offsets the GPU tests rely on."""
import many_stream_cases as mc
from test_gpu_frontend_shapes import strip_eligible


def test_pick_at_256_compute_units():
    """the smallest S per height, per launch (level 0; levels 1..3), and the rows of the benchmark's configurations"""
    assert mc.smallest_streams(2080, 256, 256, 0) == {16: 1, 24: 65, 32: 94, 40: 129, 48: 147, 56: 187, 64: 205}
    assert mc.smallest_streams(2080, 256, 256, 1) == {16: 1, 24: 304, 32: 400, 48: 608, 64: 911}
    assert mc.smallest_streams(640, 480, 256, 0) == {16: 1, 24: 205, 32: 308, 40: 410, 48: 513, 56: 615, 64: 683}
    lv = mc.smallest_streams(640, 480, 256, 1, s_max=1300)
    assert lv[24] == 621 and lv[40] == 1242
    assert mc.pick(640, 480, 3072, 256) == (48, 40)                  # the benchmark
    assert mc.pick(1280, 720, 2048, 256) == (48, 24)                 # BASELINE configs[3]
    assert mc.pick(640, 480, 192, 256) == (16, 16)                   # the largest run of the rest of the suite
    assert mc.pick(320, 240, 577, 256) == (16, 16)                   # the tracker tests of test_gpu_many_streams.py
    assert mc.pick(640, 480, 3072, 0) == (48, 40)                    # no count from the device: 256 is assumed


def test_pick_is_the_first_minimum_of_the_cost():
    """against the cost written out: rounds of 4 n_cu resident workgroups x (R + 6) row steps"""
    for w, h, S, n in ((2080, 250, 147, 256), (640, 250, 385, 304), (640, 480, 1242, 256)):
        for launch, levels in ((0, (0,)), (1, (1, 2, 3))):
            cost = {}
            for R in mc.HEIGHTS:
                wgs = sum(-(-S * -(-(h >> l) // R) // mc.bands_per_workgroup(w >> l)) for l in levels)
                cost[R] = -(-wgs // (4 * n)) * (R + 6)
            best = min(cost.values())
            assert mc.pick(w, h, S, n)[launch] == min(R for R in cost if cost[R] == best)


def test_the_sweep_covers_the_heights():
    for n in (256, 304, 64):                                         # whatever the device, as long as the smallest S exists below 4096
        plan = mc.sweep_plan(n)
        assert {p[3][0] for p in plan} >= set(mc.LEVEL0_HEIGHTS)
        assert {p[3][1] for p in plan} >= set(mc.LEVELS_HEIGHTS)
    plan = mc.sweep_plan(256)
    assert [p[2] for p in plan] == [65, 129, 147, 187, 94, 205, 385, 304, 608, 911, 1242]
    for w, h, S, R in plan:
        assert strip_eligible(w, h) and S > mc.K
    heights = [[R[0]] + [R[1]] * 3 for *_x, R in plan]
    partial = [mc.partial_last_strip(p[1], r) for p, r in zip(plan, heights)]
    assert any(all(x) for x in partial)                              # a partial last strip on every level
    assert sum(not any(x) for x in partial) >= 2                     # and heights every strip divides: 2080x256 at 32 and at 64
    bpw = [[mc.bands_per_workgroup(p[0] >> l) for l in range(4)] for p in plan]
    assert any(b[0] == 1 for b in bpw) and any(b[0] > 1 for b in bpw)   # one strip per workgroup, and strips of several streams


def test_replication_has_no_equal_neighbours():
    idx = [mc.replica(s) for s in range(8192)]
    assert all(a != b for a, b in zip(idx, idx[1:]))
    assert set(idx[:6]) == set(range(mc.K))
    assert any(idx[s] != idx[s + 64] for s in range(64))             # a workgroup of lanes is no copy of the one before
    assert (5 * 63 + 63 // 64) % 3 == (5 * 64 + 64 // 64) % 3        # why the shift at a workgroup edge is 2 and not 1
    for s in range(0, 8192 - 64, 64):
        assert sorted(idx[s:s + 64].count(k) for k in range(mc.K)) in ([21, 21, 22],)


def test_fixed_streams_and_offsets():
    assert mc.tracker_streams(256) == 577
    assert mc.fixed_streams(577, 256) == [0, 63, 64, 65, 127, 128, 511, 512, 513, 576]
    assert mc.fixed_streams(mc.tracker_streams(64), 64) == [0, 63, 64, 65, 127, 128, 129, 192]
    S, streams = mc.offset_streams(640, 480, 128)
    stride = mc.keyframe_image_stride(640, 480, 0, 128)
    assert stride == 128 * 640 * 480 and (S, streams) == (112, [0, 54, 55, 109, 110, 111])
    assert 54 * stride < (1 << 31) < 55 * stride and 109 * stride < (1 << 32) < 110 * stride
    S, streams = mc.measurement_offset_streams(128, 4096)
    stride = mc.measurement_table_stride(128, 4096)
    assert stride == 12582912 and (S, streams) == (344, [0, 170, 171, 341, 342, 343])
    assert 170 * stride < (1 << 31) < 171 * stride and 341 * stride < (1 << 32) < 342 * stride
