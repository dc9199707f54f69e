"""Camera calibrations other than the default, shared by tests/test_cam_cases.py (CPU: the camera arithmetic against a 50-digit
restatement, the scenes' conditions in the oracle) and tests/test_gpu_calibrations.py (GPU: the device == the oracle at every
calibration).  No GPU is touched here.

vslam_params.cam (normalised fx, fy, cx, cy and the ATAN distortion w) is read by every projecting kernel through CamModel.  With the
reference's calibration (w = -0.0134) the lens is almost a pinhole: the w == 0 branches are never taken, the distortion derivative is
1e-4 of the diagonal, tan / atan run at arguments near 0.01 and cam_fill's max(c, 1 - c) always picks the same side.  Each calibration
below reaches what its comment names.

Edge points.  A feeder map holds points that project well inside the image.  add_edge_points() adds map points placed, for the pose the
tracker projects with in frame 0, on both sides of every exit of TrackerData::Project (jni/TrackerData.h:69-87; csrc/track.hip
td_project) and of ReFindInSingleKeyFrame's projection (jni/MapMaker.cc:979-996): behind the camera, z either side of 0.001, r^2 either
side of largest_radius^2, just outside and just inside each image border, and inside the camera's switch zones r < 0.001 and r < 0.01.
An edge point takes the source keyframe, level and patch axes of the real map point that projects nearest to it, so those in the image
are searched like any other, and a measurement (its exact projection, as feeder.build_map gives) in every keyframe that sees it.  A point
with a single measurement would leave its depth to the damping of the bundle adjustment alone, which no map of the reference holds."""
import functools

import numpy as np

import oracle.binding as orc
from helpers import make_scene

W, H = 320, 240
REF = (0.841906, 1.10893, 0.505171, 0.470265, -0.0133843)     # jni/ATANCamera.cc:20-24
CALIBRATIONS = {
    "ref": REF,                                               # control: agrees with what the suite already holds
    "pinhole": REF[:4] + (0.0,),                              # every w == 0 branch, distortion_enabled = 0
    "tiny_w": REF[:4] + (1e-7,),                              # the distortion path with winv = 1e7 and two_tan = 1e-7
    "ptam_default": (0.5, 0.75, 0.5, 0.5, 0.1),               # PTAM's shipped default
    "wide": (0.58, 0.77, 0.52, 0.46, 0.93),                   # strong barrel distortion, largest_radius 1.77, off-centre
    "pincushion": (0.9, 1.2, 0.38, 0.60, -0.45),              # negative w of real size; cam_fill takes the 1 - c side in x, the c side in y
}
NAMES = tuple(CALIBRATIONS)
# radius x w passes pi / 2 at the image corner: largest_radius comes out negative and nothing is ever searched.  Pure arithmetic only.
OUT_OF_MODEL = (0.45, 0.60, 0.5, 0.5, 1.2)
# The feeder seeds of a calibration's two scenes.  The re-synchronised test holds the device's adjusted map to 1e-7 of the oracle's although
# the two take their sums in different orders; that bar means something only where the adjustment itself does not blow last-bit
# differences up to its size.  How much a scene's frame-0 adjustment does so is measured in the oracle alone, between its two builds
# (the product's transcendentals / glibc's: they differ in last bits).  Measured after frame 0, worst of points and keyframe poses:
#   seed 5:   ref, patch 11: 5e-7 between the builds (device against oracle: 4.2e-7, 19 LM trials); ptam_default, patch 8: 8e-7 (2.5e-7, 20)
#   seed 77:  ptam_default, patch 8 and 11: 1e-7 (2.4e-7 and 1.7e-7, 20 trials each)
#   seeds 1234 and 23: at most 1e-9 at every calibration and patch size (device against oracle: at most 2.7e-9)
# -- an adjustment that is still moving weakly constrained new points when it reaches its 20 iterations.  tests/test_cam_cases.py
# asserts MAX_LIBM_SPREAD, a tenth of the bar.
SEEDS = (1234, 23)
MAX_LIBM_SPREAD = 1e-8
N_FRAMES = 6
# The bootstrap scene (InitFromStereo on host matches): the oracle's trails over BOOT_FRAMES frames of this feeder seed.  Which stereo
# points survive the adjustments that follow InitFromStereo hangs on outlier decisions; the GPU test compares that set exactly, which needs
# a scene where the decisions are not borderline.  Condition, in the oracle alone (tests/test_cam_cases.py): its two builds take the same
# number of LM trials and keep the same points at every calibration.  Of the seeds 5, 7, 23, 31, 77, 99, 1234, 4321 only 23 meets it (with
# seed 5 the two builds keep different sets at ref; with the others they differ in the number of trials at one calibration or more).
BOOT_SEED = 23
BOOT_FRAMES = 12

RADII_ABS = (0.0101, 0.02)                                    # just outside the derivative switch, absolute
RADII_REL = (0.1, 0.5, 0.999, 1.0, 1.2, 1.4999, 1.5001, 3.0)  # x largest_radius
ANGLES = (0.0, 0.7, 1.5707963267948966, 2.4, 3.3, 4.1, 5.6)
ZONE_RADII = (0.0, 5e-4, 0.000999, 0.001, 0.0011, 0.00999, 0.01)


def derived(cam5, w=W, h=H):
    return dict(zip(orc.CAM_DERIVED, orc.cam_eval(cam5, w, h, np.zeros((0, 2)))[1]))


def smooth_points(cam5, w=W, h=H):
    """(n, 2) image-plane points outside the reference's switch zones: RADII_ABS and RADII_REL x largest_radius at ANGLES; with each its
    radius as the multiple of largest_radius (nan for the absolute ones)"""
    lr = abs(derived(cam5, w, h)["largest_radius"])
    radii = [(r, np.nan) for r in RADII_ABS] + [(m * lr, m) for m in RADII_REL]
    xy = np.array([[r * np.cos(a), r * np.sin(a)] for r, _m in radii for a in ANGLES])
    return xy, np.array([m for _r, m in radii for _a in ANGLES])


def zone_points():
    """(n, 2) image-plane points at ZONE_RADII (exactly: along the axes, where sqrt(x * x) == x) and their radii"""
    xy, rr = [], []
    for r in ZONE_RADII:
        for d in ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)):
            xy.append((r * d[0], r * d[1])); rr.append(r)
    return np.array(xy), np.array(rr)


UNPROJECT_ZONE = (0.00999, 0.01001)                           # dist_r either side of UnProject's switch


def unproject_zone_points(cam5):
    """(n, 2) image-plane points whose projections lie at the distorted radii UNPROJECT_ZONE from the principal point (to 1e-4
    relative: near the centre the factor is two_tan / w)"""
    w = cam5[4]
    scale = 1.0 if w == 0.0 else w / (2.0 * np.tan(w / 2.0))
    return np.array([[d * scale * np.cos(a), d * scale * np.sin(a)] for d in UNPROJECT_ZONE for a in ANGLES[:4]])


def all_points(cam5, w=W, h=H):
    """the smooth points first, then the switch-zone ones"""
    return np.concatenate([smooth_points(cam5, w, h)[0], zone_points()[0], unproject_zone_points(cam5)])


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
def pose_xform(pose12, pos):
    """pose_xform of csrc/dev_math.h / mySE3 * v (jni/RT.h:492-499), operation by operation"""
    R, t = pose12[:9], pose12[9:]
    return np.array([t[i] + (R[3 * i] * pos[0] + R[3 * i + 1] * pos[1] + R[3 * i + 2] * pos[2]) for i in range(3)])


EXITS = ("behind", "z below 0.001", "z above 0.001", "beyond largest radius", "within largest radius", "outside left", "outside right",
         "outside top", "outside bottom", "inside left", "inside right", "inside top", "inside bottom", "r < 0.001", "r < 0.01")


def classify(cam5, w, h, pose12, pos):
    """The exit of TrackerData::Project that the map point pos takes at pose12, from the oracle's camera: one of "behind" (z < 0),
    "z < 0.001", "radius", "invalid", "outside" (with the border), or "in image"; and (z, r, im)"""
    lr = derived(cam5, w, h)["largest_radius"]
    c = pose_xform(pose12, pos)
    if c[2] < 0.001:
        return ("behind" if c[2] < 0 else "z < 0.001"), (c[2], None, None)
    x, y = c[0] / c[2], c[1] / c[2]
    if x * x + y * y > lr * lr:
        return "radius", (c[2], np.sqrt(x * x + y * y), None)
    im, _d, inv, _lr = orc.cam_project(cam5, w, h, x, y)
    r = np.sqrt(x * x + y * y)
    if inv:
        return "invalid", (c[2], r, im)
    for cond, name in ((im[0] < 0, "outside left"), (im[0] > w, "outside right"), (im[1] < 0, "outside top"), (im[1] > h, "outside bottom")):
        if cond:
            return name, (c[2], r, im)
    return "in image", (c[2], r, im)


def edge_targets(cam5, w, h):
    """name -> camera-frame position (x, y, z) of the edge point, from the oracle's camera"""
    lr = derived(cam5, w, h)["largest_radius"]
    fx, fy, cx, cy = w * cam5[0], h * cam5[1], w * cam5[2] - 0.5, h * cam5[3] - 0.5
    # the direction of the image corner farthest from the principal point, where largest_radius is taken
    far = np.array([(0.0 if cam5[2] > 1 - cam5[2] else w) - cx, (0.0 if cam5[3] > 1 - cam5[3] else h) - cy]) / np.array([fx, fy])
    far /= np.linalg.norm(far)
    depth = 1.5
    out = {}

    def at(name, xy, z=depth):
        out[name] = np.array([xy[0] * z, xy[1] * z, z])

    pc = orc.cam_unproject(cam5, w, h, cx + 30.0, cy - 20.0)          # a direction well inside the image
    at("behind", pc, -depth)
    at("z below 0.001", pc, 0.001 * (1 - 1e-6))
    at("z above 0.001", pc, 0.001 * (1 + 1e-6))
    at("beyond largest radius", far * lr * (1 + 1e-9))
    at("within largest radius", far * lr * (1 - 1e-9))
    eps = 0.01                                                          # pixels
    for name, ix, iy in (("left", -eps, cy + 11.0), ("right", w + eps, cy - 13.0), ("top", cx + 17.0, -eps), ("bottom", cx - 19.0, h + eps)):
        at("outside " + name, orc.cam_unproject(cam5, w, h, ix, iy))
    for name, ix, iy in (("left", eps, cy + 11.0), ("right", w - eps, cy - 13.0), ("top", cx + 17.0, eps), ("bottom", cx - 19.0, h - eps)):
        at("inside " + name, orc.cam_unproject(cam5, w, h, ix, iy))
    at("r < 0.001", (3e-4, -4e-4))                                      # r = 5e-4: the factor switch
    at("r < 0.01", (-3e-3, 4e-3))                                       # r = 5e-3: the derivative switch only
    return out


def add_edge_points(m, cam5, w, h, pose12):
    """-> (map with the edge points in front, as a plain dict; {name: point index}).  pose12: the pose the tracker projects with in
    frame 0 (the start pose: the motion model's velocity is zero)."""
    pts = [dict(q) for q in m["points"]]
    R, t = np.asarray(pose12[:9]).reshape(3, 3), np.asarray(pose12[9:])
    proj = []                                                           # where the real points project, for the neighbour
    for q in pts:
        kind, (_z, _r, im) = classify(cam5, w, h, pose12, q["pos"])
        proj.append(im if kind == "in image" else (np.inf, np.inf))
    proj = np.array(proj)
    index, edge = {}, []
    for name, c in edge_targets(cam5, w, h).items():
        pos = R.T @ (c - t)
        z = c[2] if abs(c[2]) > 0.01 else 1.0
        fx, fy, cx, cy = w * cam5[0], h * cam5[1], w * cam5[2] - 0.5, h * cam5[3] - 0.5
        approx = np.array([cx + fx * c[0] / z, cy + fy * c[1] / z])     # the pinhole position is near enough to pick a neighbour
        if c[2] > 0.01:
            kind, (_z, _r, im) = classify(cam5, w, h, pose12, pos)
            if im is not None:
                approx = im
        nb = int(np.argmin(((proj - approx) ** 2).sum(1)))
        q = dict(pts[nb]); q["pos"] = pos
        index[name] = len(edge)
        edge.append(q)
    # measurements as build_map gives a point in the keyframes that see it: the exact projection, so that an edge point the tracker finds
    # enters the bundle adjustment as well constrained as any other
    emeas = []
    for j, q in enumerate(edge):
        b = 12 * (1 << q["level"])
        for k, kf in enumerate(m["keyframes"]):
            kind, (_z, _r, im) = classify(cam5, w, h, np.asarray(kf["pose"], np.float64), q["pos"])
            if kind == "in image" and b <= im[0] < w - b and b <= im[1] < h - b:
                emeas.append((k, j, q["level"], float(im[0]), float(im[1]), 1, 0))
    # in front of the map: with the identity order of the potentially visible set, the chop at max_patches_per_frame drops the last points
    ne = len(edge)
    meas = [(kf, pt + ne, lv, rx, ry, sp, src) for (kf, pt, lv, rx, ry, sp, src) in m["meas"]]
    return {"keyframes": m["keyframes"], "points": edge + pts, "meas": meas + emeas}, index


def exit_of(name):
    """what classify() must say of the edge point `name`"""
    if name == "behind":
        return "behind"
    if name == "z below 0.001":
        return "z < 0.001"
    if name == "beyond largest radius":
        return "radius"
    if name.startswith("outside"):
        return name
    if name == "within largest radius":                                  # the image corner itself: projected, in or out by a rounding
        return "projected"
    return "in image"


@functools.lru_cache(maxsize=None)
def scene(name, seed, w=W, h=H, n_frames=N_FRAMES):
    """(feeder, map with edge points, frames, {edge name: point index}) rendered and mapped at the calibration `name`"""
    cam5 = CALIBRATIONS[name]
    f, m, frames = make_scene(w, h, seed=seed, n_frames=n_frames, cam=cam5)
    m2, index = add_edge_points(m, cam5, w, h, f.pose(-1))
    return f, m2, frames, index


def takes_exit(kind, name):
    want = exit_of(name)
    return kind in ("in image", "outside left", "outside right", "outside top", "outside bottom") if want == "projected" else kind == want


def frame0_maps(patches=(8, 11)):
    """{"name seed patch": [LM trials, point positions, keyframe poses]} after frame 0 (keyframe, map growth, bundle adjustment) in the
    oracle build this process has loaded, for every scene"""
    from helpers import make_oracle
    from visualslam_android_amd import capi
    out = {}
    for name in NAMES:
        for seed in SEEDS:
            f, m, frames, _ix = scene(name, seed)
            for patch in patches:
                o = make_oracle(capi.default_params(W, H, 1, patch_size=patch, grow_map=3, cam=CALIBRATIONS[name]), m, f.pose(-1))
                o.track_frame(frames[0])
                st = o.state()
                out["%s %d %d" % (name, seed, patch)] = [int(st.n_ba_trials), o.points()["pos"].ravel().tolist(), [list(o.keyframe_pose(k)) for k in range(st.n_keyframes)]]
                o.close()
    return out


@functools.lru_cache(maxsize=None)
def boot_scene(name):
    """(first frame, last frame, matches (n, 4) x y first, x y second) of the calibration's bootstrap scene: the oracle's own trails"""
    from visualslam_android_amd import capi, feeder
    cam5 = CALIBRATIONS[name]
    frames = feeder.Feeder(W, H, seed=BOOT_SEED, noise=2, cam=cam5).render(0, BOOT_FRAMES)
    o = orc.OracleSystem(orc.params_from_vslam(capi.default_params(W, H, 1, patch_size=8, grow_map=3, cam=cam5)))
    o.press_spacebar()
    for t in range(BOOT_FRAMES):
        o.track_frame(frames[t])
    matches = o.trails()
    o.close()
    return frames[0], frames[BOOT_FRAMES - 1], matches


def boot_oracle(name):
    """the oracle after InitFromStereo on the calibration's bootstrap scene -> (oracle, ok)"""
    from visualslam_android_amd import capi
    first, last, matches = boot_scene(name)
    o = orc.OracleSystem(orc.params_from_vslam(capi.default_params(W, H, 1, patch_size=8, grow_map=3, cam=CALIBRATIONS[name])))
    ok, _pose = o.init_from_stereo(first, last, matches)
    return o, ok


def boot_records():
    """{name: [matches, ok, stereo points, LM trials, the stereo points the second keyframe still measures]} in the oracle build this
    process has loaded"""
    out = {}
    for name in NAMES:
        o, ok = boot_oracle(name)
        mo = o.keyframe_meas(1)
        out[name] = [len(boot_scene(name)[2]), int(ok), int(o.init_info()["stereo_points"]), int(o.state().n_ba_trials), mo["pt"][mo["source"] == 3].tolist()]
        o.close()
    return out
