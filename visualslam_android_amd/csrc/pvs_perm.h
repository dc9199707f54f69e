// The permutation that stands in for Tracker::TrackMap's random_shuffle of the potentially visible set (jni/Tracker.cc:396-397: every
// level's list before the coarse selection; :525: the list of all remaining points before it is cut to MaxPatchesPerFrame), stated once
// for the host and for gfx950 (like bootstrap_math.h's bm_rand).  The reference draws from libc rand(), which cannot be pinned; this
// permutation is the project's own, a pure function of (seed, frame, list, length):
//
//   mix(z)  z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
//           (the 64-bit finaliser of bm_rand, all modulo 2^64)
//   h       = mix(seed << 32 | (u32)frame)                frame: TrackerState::frame as k_motion leaves it (mnFrame after :100)
//   key(i)  = (u32)(mix(h ^ (L << 16 | i)) >> 32)         L: 0..3 = avPVS[L], 4 = the :525 list; i: position in the list's identity order
//   the shuffled list = the identity-order list sorted ascending by the composite key(i) << 32 | i
//
// 0 <= i < n <= PVS_SORT_CAP.  The composite is unique, so every correct sort gives the same list, and equal keys keep identity order.
// The stream's slot in the batch does not enter.  Seed 0 means "no shuffle" to every caller; the functions here do not special-case it.
//
// Host: pvs_permutation_host (std::sort).  Device: pvs_block_sort, a bitonic network over the workgroup's LDS buffer, which is what
// k_plan (track.hip) and the one-workgroup kernel behind vslam_pvs_permutation both call.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PVS_FN __host__ __device__ inline
#else
#define PVS_FN inline
#endif

#define PVS_SORT_CAP 4096           // longest list (= the map-point capacity of a stream): 32 KB of composites in LDS
#define PVS_LIST_REST 4             // L of the :525 list

PVS_FN uint64_t pvs_mix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
PVS_FN uint64_t pvs_frame_hash(unsigned seed, int frame) { return pvs_mix(((uint64_t)seed << 32) | (uint64_t)(uint32_t)frame); }
PVS_FN uint32_t pvs_key(uint64_t h, int list, int i) { return (uint32_t)(pvs_mix(h ^ (((uint64_t)list << 16) | (uint64_t)i)) >> 32); }
PVS_FN uint64_t pvs_composite(uint32_t key, int i) { return ((uint64_t)key << 32) | (uint64_t)(uint32_t)i; }
// length of the network that sorts n composites: the next power of two, at least one wavefront
PVS_FN int pvs_padded_length(int n) { int m = 64; while (m < n) m <<= 1; return m; }

#include <algorithm>
#include <vector>
// Host only.  out[j] = the identity-order position that lands at j.  keys (may be null) replaces the generated keys.
inline void pvs_permutation_host(unsigned seed, int frame, int list, int n, const unsigned* keys, int* out) {
  const uint64_t h = pvs_frame_hash(seed, frame);
  std::vector<uint64_t> c((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) c[i] = pvs_composite(keys ? (uint32_t)keys[i] : pvs_key(h, list, i), i);
  std::sort(c.begin(), c.end());
  for (int j = 0; j < n; j++) out[j] = (int)(uint32_t)c[j];
}

#if defined(__HIPCC__)
// buf[i] = composite of position i for i < n, the padding up to pvs_padded_length(n) above every composite.  All threads of the
// workgroup of T threads; no barrier inside (pvs_block_sort starts with one).
template <int T>
__device__ __forceinline__ void pvs_block_fill(uint64_t* buf, int n, uint64_t h, int list, const unsigned* keys) {
  const int M = pvs_padded_length(n);
  for (int i = threadIdx.x; i < M; i += T)
    buf[i] = i < n ? pvs_composite(keys ? (uint32_t)keys[i] : pvs_key(h, list, i), i) : ~0ull;
}

// Ascending bitonic sort of buf[0, M), M = pvs_padded_length(n), by the T threads of the workgroup (a multiple of 64); ends
// with a barrier.  A rank-by-counting scheme reads without conflicts (every lane the same word) but compares n^2 pairs, 65 k 64-bit
// compares per thread at 4096; the network compares M/2 log^2 M / 2.  Its sub-stages with a partner distance below one wavefront
// would put lanes l and l + 16 of a 32-lane group on one bank (a group reads 32 of 64 consecutive 8-byte words: two-way conflict
// on every ds_read_b64), so they never go through LDS: a lane holds element 64 b + lane of block b and meets its partner by a
// cross-lane exchange, all sub-stages of distance 32..1 of a stage back to back between one conflict-free load and store (32 lanes
// on 32 consecutive 8-byte words = the 64 banks once).  The sub-stages of distance >= 64 work in LDS: comparator c takes the
// words lo(c) and lo(c) + distance, consecutive lanes of a group on consecutive words again.  21 LDS sub-stages and 7 register
// passes at M = 4096 instead of 78 barriers.
template <int T>
__device__ __forceinline__ void pvs_block_sort(uint64_t* buf, int n) {
  static_assert(T % 64 == 0, "whole wavefronts: a wavefront's lanes hold one block of 64 consecutive elements");
  const int M = pvs_padded_length(n);
  __syncthreads();
  // stages k = 2..64 entirely in registers
  for (int e = threadIdx.x; e < M; e += T) {
    uint64_t v = buf[e];
    for (int k = 2; k <= 64; k <<= 1)
      for (int j = k >> 1; j >= 1; j >>= 1) {
        const uint64_t p = __shfl_xor(v, j);
        const bool keep_min = ((e & j) == 0) == ((e & k) == 0);
        v = keep_min ? (p < v ? p : v) : (p > v ? p : v);
      }
    buf[e] = v;
  }
  __syncthreads();
  for (int k = 128; k <= M; k <<= 1) {
    for (int j = k >> 1; j >= 64; j >>= 1) {
      for (int c = threadIdx.x; c < (M >> 1); c += T) {
        const int lo = ((c & ~(j - 1)) << 1) | (c & (j - 1)), hi = lo + j;
        const uint64_t a = buf[lo], b = buf[hi];
        if ((a > b) == ((lo & k) == 0)) { buf[lo] = b; buf[hi] = a; }
      }
      __syncthreads();
    }
    for (int e = threadIdx.x; e < M; e += T) {
      uint64_t v = buf[e];
      for (int j = 32; j >= 1; j >>= 1) {
        const uint64_t p = __shfl_xor(v, j);
        const bool keep_min = ((e & j) == 0) == ((e & k) == 0);
        v = keep_min ? (p < v ? p : v) : (p > v ? p : v);
      }
      buf[e] = v;
    }
    __syncthreads();
  }
}
#endif
