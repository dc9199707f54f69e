"""Cases of the many-stream parity tests (test_gpu_many_streams.py): the launch plans that change with the stream count S and the
device's compute-unit count, restated here so that a test can ask for the S at which a plan takes a given form.

* pick() restates the strip-height choice of fe_launch_slide (csrc/frontend.hip): per launch (level 0; levels 1..3) the height R in
  {16, 24, .., 64} with the fewest row steps, ceil(workgroups / (4 n_cu)) * (R + 6), the smallest R among equals.
* replica() is the pattern by which K = 3 scenes are spread over S streams; neighbours never share a scene.
* fixed_streams() are the streams of a large system that are compared with the oracle directly.
Nothing here needs a GPU; test_many_stream_cases.py pins the restatement to the figures it gives for 256 compute units."""

NLEV = 4
HALO = 3
SL_THREADS = 256
SL_CAP = 1024
SL_RMAX = 64
HEIGHTS = tuple(range(16, SL_RMAX + 1, 8))
K = 3                                    # distinct scenes (frames) of a many-stream test


def bands_per_workgroup(wl):
    return SL_THREADS // ((wl + 15) >> 4)


def _pick(w, h, S, n_cu, l0, l1):
    slots = 4 * (n_cu if n_cu > 0 else 256)
    best, best_r = -1, 32
    for R in HEIGHTS:
        wgs, fits = 0, True
        for l in range(l0, l1 + 1):
            wl, hl = w >> l, h >> l
            bpw = bands_per_workgroup(wl)
            wgs += (S * ((hl + R - 1) // R) + bpw - 1) // bpw
            if SL_THREADS * 16 + (SL_THREADS // 64) * SL_CAP * 2 + bpw * R * ((wl + 63) >> 6) * 8 > 60000:
                fits = False
        if not fits and R > 16:
            continue
        cost = ((wgs + slots - 1) // slots) * (R + 2 * HALO)
        if best < 0 or cost < best:
            best, best_r = cost, R
    return best_r


def pick(w, h, S, n_cu):
    """-> (R of the level-0 launch, R of the levels-1..3 launch) of a strip-form frame w x h in a system of S streams"""
    return _pick(w, h, S, n_cu, 0, 0), _pick(w, h, S, n_cu, 1, NLEV - 1)


def smallest_streams(w, h, n_cu, launch, s_max=4096):
    """launch 0: the level-0 launch, 1: the levels-1..3 launch -> {R: the smallest S <= s_max at which the launch runs strips R high}"""
    out = {}
    for S in range(1, s_max + 1):
        out.setdefault(pick(w, h, S, n_cu)[launch], S)
    return out


def partial_last_strip(h, R):
    """per level: does the last strip of a frame h high end short of R rows"""
    return [(h >> l) % R[l] != 0 for l in range(NLEV)]


# ---- replication --------------------------------------------------------------------------------------------------------------------
def replica(s):
    """the scene of stream s.  Neighbours differ by 5, or by 5 + 2 = 7 where s + 1 opens a new 64-lane workgroup of the
    one-lane-per-stream kernels: neither is a multiple of K = 3, so no two neighbouring streams share a scene, and the scenes of the
    lanes of one workgroup differ from those of the same lanes of the next.  (5 s + s // 64 would not do: 63 and 64 differ by 6.)"""
    return (5 * s + 2 * (s // 64)) % K


def fixed_streams(S, n_cu):
    """streams of a large system that are held to the oracle directly: the edges of the 64-lane workgroups and of the 2 n_cu grid"""
    want = [0, 63, 64, 65, 127, 128, 2 * n_cu - 1, 2 * n_cu, 2 * n_cu + 1, S - 1]
    return sorted({s for s in want if 0 <= s < S})


def tracker_streams(n_cu):
    """stream count of the tracker / map-maker tests: past the 2 n_cu cap of the map-maker's grid by a workgroup of lanes and one"""
    return 2 * n_cu + 65


# ---- the front-end sweep: (w, h, launch, R); S = smallest_streams(w, h, n_cu, launch)[R] at run time --------------------------------
# 2080 wide: 130 strips of 16 columns, one band per workgroup on level 0 (bands per workgroup 1, 3, 7, 15 on the four levels) -- each
# height with about half the pixels a 640-wide frame needs.  640 wide: six bands per workgroup on level 0 (6, 12, 25, 51): a workgroup
# holds strips of several streams.
# Heights: 2080x256 has levels 256, 128, 64, 32 -- multiples of the level-0 heights 32 and 64 and of the 16 the levels launch then
# runs, so no strip is partial.  2080x250 and 640x250 have levels 250, 125, 62, 31 (250 = 10 mod 16): no multiple of any R, every level
# ends in a partial strip.  640x480 is the benchmark's shape; it alone reaches 40 on the levels launch below 2000 streams.
# A case sets the height of ONE launch; the other launch runs whatever pick() gives at that S (sweep_plan says which).
FE_SWEEP = [
    (2080, 250, 0, 24), (2080, 250, 0, 40), (2080, 250, 0, 48), (2080, 250, 0, 56),
    (2080, 256, 0, 32), (2080, 256, 0, 64),
    (640, 250, 0, 24),
    (2080, 250, 1, 24), (2080, 250, 1, 48), (2080, 250, 1, 64),
    (640, 480, 1, 40),
]
LEVEL0_HEIGHTS = (24, 32, 40, 48, 56, 64)                # what the sweep must cover on the level-0 launch
LEVELS_HEIGHTS = (24, 40, 48, 64)                        # and on the levels launch: 40 and 48 are what the two benchmark configurations run


def sweep_plan(n_cu):
    """-> [(w, h, S, (R of level 0, R of levels 1..3))] of FE_SWEEP on a device of n_cu compute units"""
    out = []
    for w, h, launch, R in FE_SWEEP:
        S = smallest_streams(w, h, n_cu, launch)[R]
        out.append((w, h, S, pick(w, h, S, n_cu)))
    return out


# ---- offsets past 2^31 and 2^32 bytes ------------------------------------------------------------------------------------------------
def keyframe_image_stride(w, h, level, max_keyframes):
    """bytes a stream owns of kf_img[level]: max_keyframes images of pitch (a multiple of 64) x height"""
    return max_keyframes * ((((w >> level) + 63) & ~63) * (h >> level))


def offset_streams(w, h, max_keyframes):
    """-> (S, streams): the smallest system whose last two streams start beyond 2^32 bytes in kf_img[0], and the streams that get a map:
    0, the stream that straddles each of 2^31 and 2^32, the first that starts beyond each, and the last"""
    stride = keyframe_image_stride(w, h, 0, max_keyframes)
    first31, first32 = -(-(1 << 31) // stride), -(-(1 << 32) // stride)
    S = first32 + 2
    return S, sorted({0, first31 - 1, first31, first32 - 1, first32, S - 1})


MEAS_BYTES = 24                          # sizeof(MeasDev): double root[2], four flag bytes, an int of padding


def measurement_table_stride(max_keyframes, max_points):
    """bytes a stream owns of kf_meas: one slot per keyframe x map point"""
    return max_keyframes * max_points * MEAS_BYTES


def measurement_offset_streams(max_keyframes, max_points):
    """as offset_streams, for kf_meas"""
    stride = measurement_table_stride(max_keyframes, max_points)
    first31, first32 = -(-(1 << 31) // stride), -(-(1 << 32) // stride)
    S = first32 + 2
    return S, sorted({0, first31 - 1, first31, first32 - 1, first32, S - 1})
