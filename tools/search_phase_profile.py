"""Phase profile of k_searchN (diagnostic library from tools/build_baprof.sh): python tools/search_phase_profile.py [streams] [patch]
VSLAM_LIB names another diagnostic library, e.g. one built with VSLAM_PROF_DEFS="-DSEARCH_N=32 -DSEARCH_K=2" (the earlier trip sizes)."""
import os, sys, ctypes as C
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')); sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests'))
import numpy as np
from visualslam_android_amd import capi
capi.load_library(os.environ.get('VSLAM_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'visualslam_android_amd', 'libvslam_hip_baprof.so'))
from helpers import *
W, H = 640, 480
f, m, frames = make_scene(W, H, n_frames=6)
S = int(sys.argv[1]) if len(sys.argv) > 1 else 1
PATCH = int(sys.argv[2]) if len(sys.argv) > 2 else 8
g = capi.System(capi.default_params(W, H, S, patch_size=PATCH))
for s in range(S):
    g.load_map(s, m); g.set_pose(s, f.pose(-1))
lib = capi.load_library()
SLOTS = 64
out = (C.c_ulonglong * (2 * SLOTS))()
g.track_frame(np.stack([frames[0]] * S)); g.synchronize()        # the first frame makes every template: kept out of the sums
lib.vslam_debug_search_prof(out, 1)
NF = 4
for t in range(1, 1 + NF):
    g.track_frame(np.stack([frames[t]] * S))
g.synchronize()
lib.vslam_debug_search_prof(out, 1)
N, K = int(out[15]), int(out[SLOTS + 15])
names = ['entry loads', 'template (cached or refresh)', 'LUT', 'filter trips', 'ZMSSD trips', 'write-out']


def hist(v, labels):
    tot = max(1, sum(v))
    return ', '.join('%s: %.1f%%' % (l, 100.0 * x / tot) for l, x in zip(labels, v))


print('S %d, %dx%d patches, %d frames, corners per group and trip N = %d, candidates in flight K = %d; every seventh workgroup per XCD is stamped' % (S, PATCH, PATCH, NF, N, K))
for stage, label in ((0, 'coarse'), (1, 'fine')):
    o = [int(x) for x in out[stage * SLOTS:(stage + 1) * SLOTS]]
    waves, patches = o[6], o[11]
    if not waves:
        print('%s stage: no wavefront stamped' % label); continue
    tot = sum(o[0:6])
    print('%s stage: %d wavefronts, %d patches stamped, %.1f kcycles per wavefront' % (label, waves, patches, tot / 1e3 / waves))
    for i in range(6):
        print('  %-30s %8.2f kcyc/wavefront %5.1f%%' % (names[i], o[i] / 1e3 / waves, 100.0 * o[i] / tot))
    print('  wavefronts on the __any(refresh) path: %.1f%%' % (100.0 * o[7] / waves))
    print('  window corners per patch: mean %.1f; %s' % (o[13] / max(1, patches), hist(o[16:24], ['0', '1-16', '17-32', '33-48', '49-64', '65-96', '97-128', '>128'])))
    print('  filter trips per wavefront: mean %.2f; %s' % (o[8] / waves, hist(o[34:40], ['0', '1', '2', '3', '4', '5+'])))
    print('  survivors per patch: mean %.2f; %s' % (o[12] / max(1, patches), hist(o[24:33], ['0', '1', '2', '3', '4', '5-8', '9-12', '13-16', '>16'])))
    ppw = patches / waves
    print('  ZMSSD trips per wavefront: mean %.2f, against %.2f if each of its %.1f patches made only its own (ceil(survivors / K), mean over the patches); %s'
          % (o[9] / waves, o[10] / max(1, patches), ppw, hist(o[40:50], [str(i) for i in range(9)] + ['9+'])))
