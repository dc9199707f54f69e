"""The sizes and keyframe counts at which the SmallBlurryImage code (csrc/sbi_dev.h, sbi.hip, reloc.hip) takes another path, with the
synthetic frames and the oracle's answers for them.  tests/test_sbi_cases.py checks the table against the constants of the sources and
the oracle on the CPU; tests/test_gpu_sbi_sizes.py runs the kernels on it.

Frames are synthetic full-resolution images, no feeder and no map: a smooth texture (tests/test_oracle_sbi.py's smooth_image, at
eight times the wavelengths so that level 3 looks like it) plus noise.  A stream sees A, A again, then A turned by 0.03 rad and moved by
a few level-3 pixels with fresh noise; every stream has its own seed."""
import collections
import math
import os
import re

import numpy as np

import reloc_ref
from oracle import binding as orc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "visualslam_android_amd", "csrc")
LDS_NO_ATTRIBUTE = 48 * 1024            # above this sbi.hip and reloc.hip raise the kernel's dynamic-LDS limit before the launch


def constants():
    """the #defines the table depends on, read from the sources"""
    out = {}
    for fn, names in (("sbi_dev.h", ("SBI_THREADS", "SBI_CHUNK", "SBI_MAX_PIX", "SBI_REC")), ("reloc.hip", ("RELOC_KF_PER_ROUND",))):
        text = open(os.path.join(CSRC, fn)).read()
        for n in names:
            m = re.findall(r"^#define\s+%s\s+(\d+)\b" % n, text, re.M)
            assert len(m) == 1, (fn, n, m)
            out[n] = int(m[0])
    return out


Geom = collections.namedtuple("Geom", "w3 h3 W H N nch last floats pos rec lds")


def geometry(w, h, c):
    """what sbi_dev.h computes for a w x h frame: level 3, the small image, the chunks of the ESM sums, sbi_lds_bytes' terms"""
    w3, h3 = w >> 3, h >> 3
    W, H = w3 // 2, h3 // 2
    N = W * H
    nch = (N + c["SBI_CHUNK"] - 1) // c["SBI_CHUNK"]
    floats = (2 * N * 4 + 7) & ~7
    pos, rec = 2 * N * 8, 2 * c["SBI_CHUNK"] * c["SBI_REC"] * 8
    return Geom(w3, h3, W, H, N, nch, N - (nch - 1) * c["SBI_CHUNK"], floats, pos, rec, floats + max(pos, rec))


# a property of a size, named in a row's `hits`: (frame size, its geometry, the constants) -> bool
PROPERTIES = {
    "smallest legal frame": lambda w, h, g, c: (w, h) == (48, 48),
    "no interior pixel survives": lambda w, h, g, c: g.W < 4 or g.H < 4,               # every interior pixel has a neighbour in the warp's last column or row, which is never sampled
    "level 3 odd both ways": lambda w, h, g, c: g.w3 % 2 == 1 and g.h3 % 2 == 1,
    "level-3 pitch above its width": lambda w, h, g, c: (g.w3 + 63) // 64 * 64 > g.w3,
    "N below a chunk": lambda w, h, g, c: g.N < c["SBI_CHUNK"],
    "one chunk": lambda w, h, g, c: g.nch == 1,
    "exactly one full chunk": lambda w, h, g, c: g.N == c["SBI_CHUNK"],
    "full last chunk of several": lambda w, h, g, c: g.nch > 1 and g.last == c["SBI_CHUNK"],
    "partial last chunk of several": lambda w, h, g, c: g.nch > 1 and g.last < c["SBI_CHUNK"],
    "N below the threads": lambda w, h, g, c: g.N < c["SBI_THREADS"],
    "N equals the threads": lambda w, h, g, c: g.N == c["SBI_THREADS"],
    "N no multiple of the threads": lambda w, h, g, c: g.N > c["SBI_THREADS"] and g.N % c["SBI_THREADS"] != 0,
    "W, H and N odd": lambda w, h, g, c: g.W % 2 == 1 and g.H % 2 == 1 and g.N % 2 == 1,
    "records the larger": lambda w, h, g, c: g.rec > g.pos,
    "positions equal records": lambda w, h, g, c: g.pos == g.rec,
    "first size with positions the larger": lambda w, h, g, c: g.pos > g.rec and geometry(w, h - 16, c).pos <= g.rec,
    "last size without the attribute": lambda w, h, g, c: g.lds == LDS_NO_ATTRIBUTE,
    "first size with the attribute": lambda w, h, g, c: g.lds > LDS_NO_ATTRIBUTE and geometry(w, h - 16, c).lds <= LDS_NO_ATTRIBUTE,
    "the documented large shape": lambda w, h, g, c: (w, h) == (1280, 720) and g.lds > LDS_NO_ATTRIBUTE,
    "N equals SBI_MAX_PIX": lambda w, h, g, c: g.N == c["SBI_MAX_PIX"],
    "one column over SBI_MAX_PIX": lambda w, h, g, c: g.N > c["SBI_MAX_PIX"] and geometry(w - 16, h, c).N <= c["SBI_MAX_PIX"],
}

Row = collections.namedtuple("Row", "w h W H N nch last lds hits")

# frame size -> small image W x H, N, chunks of the ESM sums, pixels of the last one, dynamic LDS in bytes, and why the row is there
TABLE = [
    Row(48, 48, 3, 3, 9, 1, 9, 30792, ("smallest legal frame", "no interior pixel survives", "N below a chunk", "one chunk", "N below the threads", "records the larger")),
    Row(56, 72, 3, 4, 12, 1, 12, 30816, ("level 3 odd both ways", "no interior pixel survives", "N below a chunk")),
    Row(136, 120, 8, 7, 56, 1, 56, 31168, ("level 3 odd both ways", "N below a chunk", "one chunk", "N below the threads")),
    Row(256, 128, 16, 8, 128, 1, 128, 31744, ("exactly one full chunk", "one chunk", "N below the threads")),
    Row(264, 136, 16, 8, 128, 1, 128, 31744, ("exactly one full chunk", "level 3 odd both ways", "level-3 pitch above its width")),
    Row(256, 256, 16, 16, 256, 2, 128, 32768, ("N equals the threads", "full last chunk of several")),
    Row(496, 496, 31, 31, 961, 8, 65, 38408, ("W, H and N odd", "partial last chunk of several", "N no multiple of the threads")),
    Row(512, 480, 32, 30, 960, 8, 64, 38400, ("partial last chunk of several", "N no multiple of the threads")),
    Row(1024, 480, 64, 30, 1920, 15, 128, 46080, ("positions equal records", "full last chunk of several")),
    Row(1024, 496, 64, 31, 1984, 16, 64, 47616, ("first size with positions the larger",)),
    Row(1024, 512, 64, 32, 2048, 16, 128, 49152, ("last size without the attribute",)),
    Row(1024, 528, 64, 33, 2112, 17, 64, 50688, ("first size with the attribute", "partial last chunk of several")),
    Row(1280, 720, 80, 45, 3600, 29, 16, 86400, ("the documented large shape", "partial last chunk of several")),
    Row(1024, 1024, 64, 64, 4096, 32, 128, 98304, ("N equals SBI_MAX_PIX", "full last chunk of several")),
    Row(1040, 1024, 65, 64, 4160, 33, 64, 99840, ("one column over SBI_MAX_PIX",)),
]
REFUSED = [r for r in TABLE if "one column over SBI_MAX_PIX" in r.hits]
LEGAL = [r for r in TABLE if r not in REFUSED]
DEGENERATE = [r for r in LEGAL if "no interior pixel survives" in r.hits]
STREAMS = 3


def size_id(r):
    return "%dx%d" % (r.w, r.h)


# ---- frames ----------------------------------------------------------------------------------------------------------------------
def texture(seed):
    """-> f(x, y) in grey levels 40 .. 200 over full-resolution pixel coordinates: smooth_image's sum of sinusoids with the seed's own
    phases and wavelengths (within a fifth of smooth_image's)"""
    rng = np.random.default_rng(seed)
    ph, sc = rng.uniform(0.0, 2.0 * math.pi, 4), rng.uniform(0.8, 1.25, 3)

    def f(x, y):
        u, v = x / 8.0, y / 8.0
        return 120 + 50 * np.sin(u / (7.0 * sc[0]) + ph[0]) * np.cos(v / (5.0 * sc[1]) + ph[1]) + 30 * np.sin((u + 2 * v) / (11.0 * sc[2]) + ph[2])
    return f


def render(f, w, h, noise_seed, angle=0.0, shift=(0.0, 0.0)):
    """the texture seen by a frame turned by `angle` about its centre and moved by `shift` full-resolution pixels, plus unit noise"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy, c, s = w / 2.0, h / 2.0, math.cos(angle), math.sin(angle)
    xs = cx + c * (x - cx) - s * (y - cy) + shift[0]
    ys = cy + s * (x - cx) + c * (y - cy) + shift[1]
    img = f(xs, ys) + np.random.default_rng(noise_seed).normal(0.0, 1.0, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


WARP = dict(angle=0.03, shift=(20.0, -12.0))       # 2.5 and 1.5 level-3 pixels


def stream_frames(w, h, seed):
    """A, A again, A warped with fresh noise"""
    f = texture(seed)
    a = render(f, w, h, seed + 1)
    return [a, a, render(f, w, h, seed + 2, **WARP)]


def level3(gray):
    return orc.make_keyframe_lite(gray)[3][0]


_frames = {}


def frames_and_expected(r, cam, quirks=0):
    """the frames of the STREAMS streams of a row, [stream][frame], and what read_sbi must give after each: (small, template, rotation,
    score) of frame t against frame t - 1 (the first against itself).  Computed once per size."""
    key = (r.w, r.h, tuple(cam), quirks)
    if key not in _frames:
        fr, want = [], []
        for s in range(STREAMS):
            f = stream_frames(r.w, r.h, 1000 * r.w + r.h + 17 * s)
            l3 = [level3(x) for x in f]
            fr.append(f)
            want.append([orc.sbi_make(l3[t]) + orc.sbi_rotation(l3[t], l3[max(t - 1, 0)], cam, quirks) for t in range(3)])
        _frames[key] = (fr, want)
    return _frames[key]


# ---- the relocaliser's scoring ---------------------------------------------------------------------------------------------------
# name, frame size, keyframes in the map, max_keyframes (None: the default), keyframe pairs that share one image, the keyframe whose
# warped image is the frame, the best keyframe
RelocCase = collections.namedtuple("RelocCase", "name w h nk cap same src best")
RELOC_CASES = [
    RelocCase("one keyframe", 256, 128, 1, None, (), 0, 0),
    RelocCase("best in a second round of one", 320, 240, 5, None, (), 4, 4),
    RelocCase("tie at the minimum", 496, 496, 7, None, ((1, 5),), 1, 1),
    RelocCase("tie above the minimum", 496, 496, 7, None, ((2, 6),), 4, 4),
    RelocCase("map at max_keyframes", 264, 136, 5, 5, (), 4, 4),
    RelocCase("large LDS", 1024, 528, 6, None, (), 5, 5),
]
RELOC_BLURS = (2.0, 2.5)
RELOC_STREAMS = 2
_reloc = {}


def reloc_images(c):
    """-> [stream] of (keyframe images, the frame): every keyframe its own texture but for the pairs of c.same, which are one array; the
    frame is keyframe c.src's texture warped, with fresh noise"""
    if c.name not in _reloc:
        out = []
        for s in range(RELOC_STREAMS):
            base = 100000 * (s + 1) + 1000 * c.w + c.h
            seeds = [base + 10 * k for k in range(c.nk)]
            for a, b in c.same:
                seeds[b] = seeds[a]
            made = {}
            kfs = [made.setdefault(sd, render(texture(sd), c.w, c.h, sd + 1)) for sd in seeds]
            out.append((kfs, render(texture(seeds[c.src]), c.w, c.h, seeds[c.src] + 2, **WARP)))
        _reloc[c.name] = out
    return _reloc[c.name]


def reloc_expected(kfs, frame, blur, cam, quirks=0):
    """what k_kf_sbi and k_recover must give up to the pose: keyframe templates and gradient images, the frame's template, every ZMSSD,
    the best keyframe, ln of the adjustment and the ESM's final score"""
    kf_l3, cur_l3 = [level3(k) for k in kfs], level3(frame)
    tmpls = [orc.sbi_make(l3, blur)[1] for l3 in kf_l3]
    cur = orc.sbi_make(cur_l3, blur)[1]
    best, scores = reloc_ref.score_keyframes(cur, tmpls)
    ln, score = orc.sbi_rotation(cur_l3, kf_l3[best], cam, quirks, blur)
    return dict(kf_tmpl=tmpls, kf_jacs=[reloc_ref.make_jacs(t) for t in tmpls], cur=cur, zmssd=scores, best=best, ln=ln, score=score)
