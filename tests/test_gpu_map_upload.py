"""The per-item map upload and read-back calls of the C ABI against the bulk ones: the same map uploaded both ways is the same map,
bit for bit, before and after tracking; a refused bulk upload changes nothing."""
import numpy as np
import pytest

from helpers import make_scene
from oracle import binding as orc
from visualslam_android_amd import capi

pytestmark = pytest.mark.gpu

W, H, N_FRAMES = 320, 240, 2


def upload_per_item(g, s, m):
    """System.load_map through vslam_map_add_keyframe / _point / _measurement, one item per call"""
    pk = m["packed"]
    for k, kf in enumerate(m["keyframes"]):
        assert g.add_keyframe(s, kf["pose"], kf["fixed"], kf["image"], kf["depth_mean"], kf["depth_sigma"]) == k
    for i in range(len(pk["pos"])):
        assert g.add_point(s, pk["pos"][i], int(pk["src_kf"][i]), int(pk["level"][i]), int(pk["ir"][i, 0]), int(pk["ir"][i, 1]), pk["right"][i], pk["down"][i]) == i
    for i in range(len(pk["m_kf"])):
        root = np.ascontiguousarray(pk["m_root"][i], np.float64)
        capi._check(g.lib.vslam_map_add_measurement(g.h, s, int(pk["m_kf"][i]), int(pk["m_pt"][i]), int(pk["m_level"][i]), root.ctypes.data,
                                                    int(pk["m_subpix"][i]), int(pk["m_source"][i])))
    capi._check(g.lib.vslam_map_set_good(g.h, s))


def assert_same_dict(a, b, tag):
    assert a.keys() == b.keys(), tag
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (tag, key)


def assert_same_map(ga, gb, grow, tag):
    sa, sb = ga.states(0, 1)[0], gb.state(0)                      # vslam_get_states on one side, vslam_get_state on the other
    assert bytes(sa) == bytes(sb), tag
    assert bytes(ga.state(0)) == bytes(sa) and bytes(gb.states(0, 1)[0]) == bytes(sb), tag
    assert_same_dict(ga.points(0), gb.points(0), tag)
    for k in range(sa.n_keyframes):
        assert np.array_equal(ga.keyframe_pose(0, k), gb.keyframe_pose(0, k)), (tag, k)
        assert_same_dict(ga.keyframe_meas(0, k), gb.keyframe_meas(0, k), (tag, k))
        for x, y in zip(ga.keyframe_sbi(0, k), gb.keyframe_sbi(0, k)):     # what is read back of the stored level images: the
            assert np.array_equal(x, y), (tag, k)                           # SmallBlurryImage and, with grow_map, the corner lists
        for l in range(4 if grow else 0):
            assert np.array_equal(ga.keyframe_corners(0, k, l), gb.keyframe_corners(0, k, l)), (tag, k, l)
    return sa


KCAP_MAX = (16384, 8192, 4096, 2048)                               # a keyframe's stored corner list per level (vslam_c.h, vslam_get_keyframe_corners)


def assert_keyframe_corners_equal_oracle(g, m, vp, tag):
    """Level::vCorners of every uploaded keyframe (the band form of the front end on the stored image) == the oracle's FAST corners of that
    image, cut in raster order at the keyframe capacity as k_store_kf_corners cuts them"""
    thr = tuple(vp.fast_threshold[l] for l in range(4))
    total = 0
    for k, kf in enumerate(m["keyframes"]):
        want = orc.make_keyframe_lite(np.ascontiguousarray(kf["image"], np.uint8), thr)
        for l in range(4):
            kcap = min(vp.max_corners[l], KCAP_MAX[l])
            corners = want[l][1][:kcap]
            assert np.array_equal(g.keyframe_corners(0, k, l), corners), (tag, k, l)
            total += len(corners)
    assert total > 100 * len(m["keyframes"]), (tag, total)


@pytest.mark.parametrize("grow", [0, 3])
def test_per_item_upload_equals_bulk_upload(grow):
    f, m, frames = make_scene(W, H, seed=5, n_frames=N_FRAMES, per_level=(120, 50, 20, 8))
    vp = capi.default_params(W, H, 1, grow_map=grow, relocalise=1)
    ga, gb = capi.System(vp), capi.System(vp)
    ga.load_map(0, m)
    upload_per_item(gb, 0, m)
    st = assert_same_map(ga, gb, grow, "uploaded")
    if grow:
        assert_keyframe_corners_equal_oracle(ga, m, vp, "uploaded")
    assert st.n_keyframes == len(m["keyframes"]) and st.n_points == len(m["packed"]["pos"]) > 100
    assert sum(len(ga.keyframe_meas(0, k)["pt"]) for k in range(st.n_keyframes)) == len(m["packed"]["m_kf"])
    for g in (ga, gb):
        g.set_pose(0, f.pose(-1))
    for t in range(N_FRAMES):
        for g in (ga, gb):
            g.track_frame(frames[t][None])
    st = assert_same_map(ga, gb, grow, "tracked")
    assert sum(st.found) > 50
    bulk = ga.templates(0, st.n_points)                           # vslam_get_templates against vslam_get_template, point by point
    assert_same_dict(bulk, gb.templates(0, st.n_points), "templates")
    assert bulk["have"].sum() > 50
    for i in range(st.n_points):
        one = gb.template(0, i)
        for key in ("tmpl", "sum", "sumsq", "bad", "have"):
            assert np.array_equal(bulk[key][i], one[key]), (i, key)
    ga.close(); gb.close()


def test_refused_bulk_measurement_upload_changes_nothing():
    """A list whose LAST entry names a point that does not exist: the error comes back and no measurement of the list is in the map."""
    _f, m, _frames = make_scene(W, H, seed=5, n_frames=N_FRAMES, per_level=(120, 50, 20, 8))
    g = capi.System(capi.default_params(W, H, 1))
    g.load_map(0, m)
    st = g.state(0)
    before = [g.keyframe_meas(0, k) for k in range(st.n_keyframes)]
    npts_before = g.points(0)
    pairs = set(zip(m["packed"]["m_kf"].tolist(), m["packed"]["m_pt"].tolist()))
    new = [(k, p) for k in range(st.n_keyframes) for p in range(st.n_points) if (k, p) not in pairs][:5]   # five slots that are empty
    assert len(new) == 5
    kf = np.array([k for k, _ in new] + [0], np.int32)
    pt = np.array([p for _, p in new] + [st.n_points], np.int32)      # the last one: one past the last point
    lv = np.zeros(6, np.int32); sp = np.zeros(6, np.int32); src = np.zeros(6, np.int32)
    root = np.full((6, 2), 17.5)
    rc = g.lib.vslam_map_add_measurements(g.h, 0, 6, kf.ctypes.data, pt.ctypes.data, lv.ctypes.data, root.ctypes.data, sp.ctypes.data, src.ctypes.data)
    assert rc == -1                                                   # VSLAM_E_INVALID
    assert b"bad entry 5" in g.lib.vslam_last_error()
    for k in range(st.n_keyframes):
        assert_same_dict(before[k], g.keyframe_meas(0, k), k)
    assert_same_dict(npts_before, g.points(0), "points")
    assert bytes(st) == bytes(g.state(0))
    capi._check(g.lib.vslam_map_add_measurements(g.h, 0, 5, kf.ctypes.data, pt.ctypes.data, lv.ctypes.data, root.ctypes.data, sp.ctypes.data, src.ctypes.data))
    assert sum(len(g.keyframe_meas(0, k)["pt"]) for k in range(st.n_keyframes)) == sum(len(b["pt"]) for b in before) + 5   # and without it, accepted
    g.close()
