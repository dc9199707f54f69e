"""NumPy restatement of the PVS shuffle (csrc/pvs_perm.h) and of TrackMap's selection (jni/Tracker.cc:437-461, 493-527), written from their
specification and not by calling the library: tests/test_pvs_perm.py and tests/test_gpu_pvs_shuffle.py hold the host form, the device routine and
k_plan's plans against it.

    mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31   (mod 2^64)
    h   = mix(seed << 32 | (u32)frame)
    key = (u32)(mix(h ^ (L << 16 | i)) >> 32)      L = 0..3: avPVS[L], 4: the list of the remaining points; i = position in identity order
    shuffled list = identity-order list sorted ascending by key << 32 | i"""
import numpy as np

SORT_CAP = 4096
LIST_REST = 4
_U = np.uint64


def mix(z):
    """the 64-bit finaliser on a uint64 array (NumPy's unsigned arithmetic wraps modulo 2^64)"""
    z = np.asarray(z, _U)
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
    return z ^ (z >> _U(31))


def keys(seed, frame, lst, n):
    h = mix(np.array([(int(seed) << 32) | (int(frame) & 0xFFFFFFFF)], _U))[0]
    i = np.arange(n, dtype=_U)
    return (mix(h ^ ((_U(lst) << _U(16)) | i)) >> _U(32)).astype(np.uint32)


def permutation(seed, frame, lst, n, explicit_keys=None):
    """out[j] = the identity-order position that lands at j"""
    k = keys(seed, frame, lst, n) if explicit_keys is None else np.asarray(explicit_keys, np.uint32)
    assert len(k) == n
    comp = (k.astype(_U) << _U(32)) | np.arange(n, dtype=_U)
    return np.argsort(comp, kind="stable").astype(np.int32)


def shuffled(lst_entries, seed, frame, lst):
    a = np.asarray(lst_entries, np.int64)
    return a if seed == 0 or len(a) < 2 else a[permutation(seed, frame, lst, len(a))]


def iteration_set(level, coarse_min, coarse_max, max_patches, try_coarse, seed, frame):
    """level[i]: search level of map point i, -1 outside the PVS.  try_coarse: bTryCoarse after :425-432 (the velocity gate, the switch; a
    just-recovered frame doubles coarse_max before calling).  seed 0 = identity.  -> dict of the ordered index lists: coarse (:437-461),
    level3 (:502-508), other (:510-527), all = vIterationSet, and chopped (the :523 condition)."""
    level = np.asarray(level)
    pvs = [shuffled(np.flatnonzero(level == l), seed, frame, l) for l in range(4)]          # :369-392 in map order, :396-397
    coarse = np.zeros(0, np.int64)
    if try_coarse and len(pvs[3]) + len(pvs[2]) > coarse_min:                                # :437
        take = min(len(pvs[3]), coarse_max)                                                  # :442-449
        coarse, pvs[3] = pvs[3][:take], pvs[3][take:]
        if len(coarse) < coarse_max:                                                         # :452
            more = coarse_max - len(coarse)
            if len(pvs[2]) <= more:                                                          # :454-456 replaces the level-3 selection
                coarse, pvs[2] = pvs[2], pvs[2][:0]
            else:                                                                            # :457-460
                coarse, pvs[2] = np.r_[coarse, pvs[2][:more]], pvs[2][more:]
    level3 = pvs[3]                                                                          # :502-508
    rest = np.r_[pvs[2], pvs[1], pvs[0]]                                                     # :511-514
    n_fine = max(0, max_patches - (len(coarse) + len(level3)))                               # :520-522
    chopped = len(rest) > n_fine                                                             # :523
    if chopped:
        rest = shuffled(rest, seed, frame, LIST_REST)[:n_fine]                               # :525-526
    return {"coarse": coarse, "level3": level3, "other": rest, "all": np.r_[coarse, level3, rest].astype(np.int64), "chopped": chopped}
