#!/bin/bash
# Diagnostic build of libvslam_hip.so with clock64() phase stamps inside the persistent BA kernel (-DVSLAM_BA_PROF).
# Output: visualslam_android_amd/libvslam_hip_baprof.so (never the product library). Use with tests/tools: see DESIGN.md.
# VSLAM_PROF_DEFS adds compiler flags (e.g. "-DSEARCH_N=32 -DSEARCH_K=2", k_searchN's earlier trip sizes), VSLAM_PROF_OUT names another output file.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
mkdir -p $T/visualslam_android_amd && cp -r $ROOT/visualslam_android_amd/csrc $T/visualslam_android_amd/ && cp -r $ROOT/include $T/
rm -rf $T/visualslam_android_amd/csrc/_build
make -s -j4 -C $T/visualslam_android_amd/csrc HIPFLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -DVSLAM_BA_PROF $VSLAM_PROF_DEFS"
OUT=$ROOT/visualslam_android_amd/${VSLAM_PROF_OUT:-libvslam_hip_baprof.so}
cp $T/visualslam_android_amd/libvslam_hip.so $OUT
rm -rf $T
echo built $OUT
