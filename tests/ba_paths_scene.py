"""Seeded bundle-adjustment scenes that steer the device Bundle down a chosen code path (tests only).

Unlike visualslam_android_amd/ba_scene.py (whose outputs the bench depends on), this generator takes an explicit fixed-camera
mask, explicit per-point tracks (which cameras see a point: long tracks in one region, points seen once or only by fixed
cameras), duplicated (camera, point) measurements, tie-heavy observations (groups of identical points) and a shuffled
measurement order.  Cameras sit on a ring at about 1.6 in front of a 1.2 x 0.9 x 0.5 box of points, so any number of them up to
the 128 a problem holds sees every point.
"""
import numpy as np

from ba_scene import CAM, project  # noqa: F401


def _rot(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def paths_scene(n_cams, n_pts, fixed=(0,), tracks=None, visibility=1.0, pixel_noise=0.5, outlier_frac=0.0, seed=0,
                init_noise=(0.01, 0.5 * np.pi / 180, 0.02), tie_group=1, quantize=False, shuffle=False, duplicates=0):
    """fixed: indices of the fixed cameras (or a bool mask of n_cams).  tracks: optional {point: [cameras]} overriding the random
    visibility of those points.  tie_group = k > 1: points come in groups of k identical copies (same truth, same start, same
    observations), so the squared errors tie k ways.  quantize: observations rounded to whole pixels.  duplicates: that many
    measurements appended again as a second (camera, point) measurement with a different position.  Returns the dict of
    ba_scene plus "fixed" as a list of bools."""
    rng = np.random.default_rng(seed)
    fx = np.zeros(n_cams, bool)
    if len(fixed) == n_cams and all(isinstance(x, (bool, np.bool_)) for x in fixed):
        fx[:] = fixed
    else:
        fx[list(fixed)] = True
    n_base = (n_pts + tie_group - 1) // tie_group
    base = np.stack([rng.uniform(-0.6, 0.6, n_base), rng.uniform(-0.45, 0.45, n_base), rng.uniform(-0.25, 0.25, n_base)], 1)
    tracks = tracks or {}
    for i in tracks:                              # a point with an explicit track sits near the middle: every camera sees it
        base[i // tie_group] = rng.uniform(-0.1, 0.1, 3)
    pts = np.repeat(base, tie_group, 0)[:n_pts]
    cams = []
    for j in range(n_cams):
        a = 2 * np.pi * j / max(n_cams, 1)
        C = np.array([0.25 * np.cos(a), 0.25 * np.sin(a), -1.6 - 0.002 * j])
        R = _rot(rng.normal(0, 0.02, 3))
        cams.append(np.concatenate([R.ravel(), -R @ C]))
    cams = np.array(cams)
    obs = {}                                      # (group representative point, camera) -> observation, shared by a tie group
    meas = []
    for i in range(n_pts):
        rep = i - i % tie_group
        cams_i = tracks.get(i)
        if cams_i is None:
            cams_i = [j for j in range(n_cams) if rng.uniform() <= visibility]
        for j in cams_i:
            key = (rep, j)
            if key not in obs:
                xy, z = project(cams[j], pts[i])
                if z <= 0.1 or not (5 < xy[0] < 635 and 5 < xy[1] < 475):
                    obs[key] = None
                else:
                    level = int(rng.integers(0, 4))
                    if pixel_noise > 0:
                        xy = xy + rng.normal(0, pixel_noise, 2)
                    if rng.uniform() < outlier_frac:
                        xy = xy + rng.choice([-20.0, 20.0], 2)
                    if quantize:
                        xy = np.round(xy)
                    obs[key] = (xy, float((1 << level) ** 2))
            if obs[key] is not None:
                meas.append((j, i, obs[key][0].copy(), obs[key][1]))
    drng = np.random.default_rng(seed + 7919)      # its own stream: the scene without the duplicates is otherwise the same
    for k in range(duplicates):
        c, p, xy, s2 = meas[int(drng.integers(0, len(meas)))]
        meas.append((c, p, xy + drng.normal(0, 1.0, 2), s2))
    if shuffle:
        meas = [meas[i] for i in rng.permutation(len(meas))]
    cams_init = cams.copy()
    for j in range(n_cams):
        if fx[j]:
            continue
        R, t = cams[j][:9].reshape(3, 3), cams[j][9:]
        dR = _rot(rng.normal(0, init_noise[1], 3))
        cams_init[j] = np.concatenate([(dR @ R).ravel(), dR @ t + rng.normal(0, init_noise[0], 3)])
    pts_init = np.repeat(base + rng.normal(0, init_noise[2], base.shape), tie_group, 0)[:n_pts]
    return {"cams_true": cams, "pts_true": pts, "cams_init": cams_init, "pts_init": pts_init, "fixed": [bool(x) for x in fx],
            "meas": meas}


def arrays(sc):
    """The scene as vslam_bundle_set_problem's arrays: cams, fixed, pts, meas_cam, meas_pt, meas_xy, meas_sigma2."""
    m = sc["meas"]
    return (np.asarray(sc["cams_init"]), np.asarray(sc["fixed"], np.int32), np.asarray(sc["pts_init"]),
            np.array([x[0] for x in m], np.int32), np.array([x[1] for x in m], np.int32),
            np.array([x[2] for x in m], np.float64).reshape(-1, 2), np.array([x[3] for x in m], np.float64))


# The one-trial scenes of the extended-precision comparison (tests/ba_hp.py): adjustable cameras -> scene.  Two fixed cameras,
# modest point counts (the reference solve is dense), first trial accepted; "config3" is BASELINE.json configs[2].
HP_NFREE = (1, 5, 6, 10, 11, 32)


def hp_scene(key):
    if key == "config3":
        from ba_scene import ba_scene
        return ba_scene(n_cams=5, n_pts=300, pixel_noise=0.5, outlier_frac=0.05, seed=1, n_fixed=1)
    nfree = int(key)
    return paths_scene(nfree + 2, 40 if nfree > 10 else 60, fixed=(0, nfree + 1), visibility=0.7, pixel_noise=0.5,
                       outlier_frac=0.02, seed=100 + nfree)
