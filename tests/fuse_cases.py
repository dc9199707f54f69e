"""Random small inputs of point fusion for the CPU tests: the plain arrays tests/fuse_ref.py's core works on, with duplicates, chains,
conflicts, bad points, odd level bytes and NaN roots planted.  Roots are multiples of 1/4, so d2 == lim2 happens, not only nearly."""
import numpy as np

RADII = (0.5, 1.0, 1.25, 2.0)


def random_case(rng, nk, n, idle=True):
    """-> dict(valid, level, root, source, bad, n_meas_kfs, never_retry, radius, min_views)"""
    pt_level = rng.integers(0, 4, n)
    root = rng.integers(0, 40, (nk, n, 2)).astype(np.float64) * 16.0
    level = np.repeat(pt_level[None, :], nk, 0).astype(np.int64)
    valid = rng.random((nk, n)) < 0.65
    for i in range(1, n):
        u = rng.random()
        if u < 0.5:                                                  # a copy of a lower point, within or at or just beyond the radius
            j = int(rng.integers(i))
            step = 0.25 * (1 << int(pt_level[j]))
            root[:, i] = root[:, j] + rng.integers(-5, 6, (nk, 2)) * step * (rng.random() < 0.8)
            level[:, i] = level[:, j]
            if u < 0.12 and nk:                                      # ... with one keyframe elsewhere, or at another level
                k = int(rng.integers(nk))
                if rng.random() < 0.5:
                    root[k, i, 0] += 64.0
                else:
                    level[k, i] = (level[k, j] + 1) % 4
    odd = rng.random((nk, n))
    level[odd < 0.01] = -1
    level[(odd >= 0.01) & (odd < 0.02)] = 31
    root[rng.random((nk, n)) < 0.01, 0] = np.nan
    never = None
    if idle:
        never = [int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 64) if rng.random() < 0.5 else 0 for _ in range(n)]
        never = [v & ((1 << nk) - 1) for v in never]
    return dict(valid=valid, level=level, root=root, source=rng.integers(0, 5, (nk, n)).astype(np.int8), bad=rng.random(n) < 0.1,
                n_meas_kfs=rng.integers(2, 9, n).astype(np.int32), never_retry=never, radius=float(rng.choice(RADII)), min_views=int(rng.integers(1, 4)))


def blob_with(blob, valid=None, level=None, root=None, source=None, bad=None, n_meas_kfs=None, never_retry=None, **_):
    """the snapshot blob with the arrays given written into its measurement table, point records and never-retry sets (tests/retire_ref.py
    has the layout); every other byte, a cell's subpix and padding included, stays"""
    import retire_ref as rr
    h, s = rr.sections(blob)
    nk, n = h.n_kf, h.n_points
    meas = s[rr.KF_MEAS].reshape(nk, n, rr.MEAS_BYTES).copy()
    rest = s[rr.POINT_REST].reshape(n, rr.REST_BYTES).copy()
    if root is not None:
        meas[:, :, :16] = np.ascontiguousarray(root, np.float64).reshape(nk, n, 2).view(np.uint8).reshape(nk, n, 16)
    for off, a in ((16, valid), (17, level), (19, source)):
        if a is not None:
            meas[:, :, off] = np.asarray(a).astype(np.int8).view(np.uint8).reshape(nk, n)
    for off, a in ((rr.REST_BAD, bad), (rr.REST_N_MEAS_KFS, n_meas_kfs)):
        if a is not None:
            rest[:, off:off + 4] = np.asarray(a).astype(np.int32).view(np.uint8).reshape(n, 4)
    s[rr.KF_MEAS], s[rr.POINT_REST] = meas.reshape(-1), rest.reshape(-1)
    if never_retry is not None and h.parts & rr.PART_IDLE:
        m64 = (1 << 64) - 1
        s[rr.NEVER_RETRY] = np.array([[v & m64, v >> 64] for v in never_retry], np.uint64).reshape(-1).view(np.uint8)
    return rr.assemble(h, s)


# ---- the scene of the live GPU test ------------------------------------------------------------------------------------------------------
LIVE_SCENE = dict(seed=1234, n_frames=65)      # the scene tests/test_gpu_retire.py, test_gpu_transform.py and test_gpu_merge.py render: one cache entry
LIVE_RADII = (0.5, 1.0, 1.5, 2.0)              # the radii the live test chooses among
LIVE_MIN_VIEWS = 2
# deduplicated(), second pass: same-level points closer than this many level pixels on the surface count as one corner.  Why 3: the rule's
# largest radius is 2 level pixels, measured in whatever keyframe sees both points, where the footprint of a level pixel differs from the
# one in the point's source keyframe by the change of perspective along the scene's path (well under half); 3 is that radius and half as
# much again.  Why the pass is needed at all: two points made of one corner in two keyframes and measured in their own keyframe only share
# no keyframe, so no measurement shows them as duplicates until the live map-maker re-finds them.  Observed behind a merge: the copies
# (1301, 1221) of two such level-2 points, 0.42 level pixels apart in ten keyframes.  It removes 32 of the 827 points the first pass leaves.
NEAR_LEVEL_PIXELS = 3.0


def map_arrays(m):
    """the core's arrays of a map dict (feeder.build_map): valid, level, root, source from its measurement list; nobody bad, no never-retry set"""
    nk, n = len(m["keyframes"]), len(m["points"])
    c = dict(valid=np.zeros((nk, n), bool), level=np.zeros((nk, n), np.int64), root=np.zeros((nk, n, 2)), source=np.zeros((nk, n), np.int8),
             bad=np.zeros(n, bool), n_meas_kfs=np.zeros(n, np.int32), never_retry=None)
    for k, p, lv, rx, ry, _sp, src in m["meas"]:
        c["valid"][k, p], c["level"][k, p], c["source"][k, p] = True, lv, src
        c["root"][k, p] = (rx, ry)
    c["n_meas_kfs"] = c["valid"].sum(0).astype(np.int32)
    return c


def deduplicated(m, radius=max(LIVE_RADII), min_views=1):
    """The map dict without the points the model would drop, repeated until it drops none.  feeder.build_map makes a point of every
    thinned corner of every keyframe and measures it in the other keyframes at its exact projection, so a surface corner that several
    keyframes detect is several points measured within a pixel of each other: about 1500 of the 2472 points of the default scene are
    duplicates by the rule (at 1 level pixel, 2 views), whatever the seed or per_level.  A duplicate at a radius is one at every larger
    radius and at every smaller min_views, so the map made at the largest radius and one view holds none at any of LIVE_RADII and
    LIVE_MIN_VIEWS -- and none that one more coinciding measurement would make: two points that share a single keyframe, agree there
    and conflict nowhere are the same corner too, and the live map-maker adds that measurement.  -> (map, points removed)"""
    import fuse_ref as fr
    from tracker_cases import sub_map
    removed = 0
    while True:
        c = map_arrays(m)
        r = fr.fuse_core(c["valid"], c["level"], c["root"], c["bad"], None, c["n_meas_kfs"], c["source"], radius, min_views)
        if not r["pairs"]:
            break
        gone = {p for p, _ in r["pairs"]}
        removed += len(gone)
        m = sub_map(m, [i for i in range(len(m["points"])) if i not in gone])
    # ... and the duplicates no measurement shows yet: two points of one level made of one corner in two keyframes, each measured in its own
    # keyframe only, share no keyframe until the live map-maker re-finds them (after a merge: their copies, everywhere).  They lie within a
    # few level pixels of each other on the surface; a point's `right` is the world vector of one level pixel (MapPoint::v3PixelRight_W).
    pos = np.array([q["pos"] for q in m["points"]], np.float64).reshape(-1, 3)
    pix = np.array([np.linalg.norm(q["right"]) for q in m["points"]])
    lev = np.array([q["level"] for q in m["points"]])
    keep = []
    for i in range(len(pos)):
        k = np.array(keep, np.int64)
        near = len(k) and ((lev[k] == lev[i]) & (np.linalg.norm(pos[k] - pos[i], axis=1) < NEAR_LEVEL_PIXELS * np.maximum(pix[k], pix[i]))).any()
        if not near:
            keep.append(i)
    removed += len(pos) - len(keep)
    return sub_map(m, keep), removed
