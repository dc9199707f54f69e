// Frame front-end on gfx950: KeyFrame::MakeKeyFrame_Lite (jni/KeyFrame.cc:5-51) and fast_nonmax
// (jni/vision/cvfast.cpp:9243-9400) for all streams of a system at once.
//
// Kernels (byte/integer work, one pass over each level image; VALU-issue bound):
//   k_fast_slide<PYR>  the form used whenever the level widths are multiples of 4 and the input is 16-B aligned: a lane owns
//                 a strip 16 pixels wide, walks down it with a sliding window of seven rows in registers (no LDS staging),
//                 runs a branch-free quick reject on every pixel, two pixels per instruction (fast_reject_dev.h), compacts the ~2 % survivors per wavefront and runs the
//                 16-pixel run-of-10 test on them; level 0 also writes its share of levels 1..3 from the same registers.
//   k_pyr_fast0 / k_fast_lvl   the general path (any width / alignment): one workgroup per 16-row band staged in LDS,
//                 pyramid from LDS, quick reject + compacted full test per 4 rows, corner-mask words in LDS.
//   k_compact     per (band of rows, level, stream) one wavefront: it adds the row counts above its band, scans the popcounts
//                 of its mask words (raster order) and every lane expands its words at its scanned offset -> bit-exact
//                 raster-ordered corner list and row LUT (jni/KeyFrame.cc:43-49) without ordered atomics or barriers.
//   k_score / k_nonmax   compute_fast_score_old + nonmax_suppression, one lane per corner.
//   k_candidates / k_thin_candidates   MakeKeyFrame_Rest's Shi-Tomasi candidates (jni/KeyFrame.cc:66-95) and
//                 MapMaker::ThinCandidates (jni/MapMaker.cc:393-422), ordered block compaction.
#include "vslam_internal.h"
#include "fast_reject_dev.h"
#include <stdlib.h>
#include <stdio.h>

#define BAND 16          // level-0 rows per workgroup (multiple of 8: three halvings stay inside a band)
#define HALO 3           // FAST ring radius (cvfast.cpp:6094-6111)
#define FE_THREADS 256

struct FeArgs {
  const uint8_t* in; size_t in_sstride; int in_pitch;
  uint8_t* lvl[NLEV]; size_t lvl_sstride[NLEV]; int lvl_pitch[NLEV];
  int w[NLEV], h[NLEV], nchunk[NLEV], thr[NLEV], cap[NLEV];
  unsigned long long* cmask[NLEV];
  int* rowcnt[NLEV];
  int* rowlut[NLEV];
  uint32_t* corners[NLEV];
  int* ncorners;
  int* overflow;
  int band_first[NLEV];   // k_fast_lvl: first blockIdx.x of each level
  const int* list;        // subset step: launch ordinal -> stream whose slots (input and products) the ordinal works on; null: the identity
};
// the stream of launch ordinal i (uniform per workgroup in the band kernels and k_compact)
DEVFN int fe_stream_of(const FeArgs& a, int i) { return a.list ? a.list[i] : i; }

__device__ __forceinline__ bool ring_run10(unsigned m16) {
  unsigned m = m16 | (m16 << 16);
  unsigned r2 = m & (m >> 1);
  unsigned r4 = r2 & (r2 >> 2);
  unsigned r8 = r4 & (r4 >> 4);
  unsigned r10 = r8 & (r2 >> 8);
  return (r10 & 0xFFFFu) != 0;
}

// FAST-10 segment test (cvfast.cpp:6088-9241; equivalence with the decision tree is pinned in
// tests/golden/fast10_tree_pin.json), split in two so the expensive part runs on densely packed lanes:
//   quick reject: an arc of 10 contiguous ring pixels contains at least one pixel of every opposite pair, so a corner
//                 needs (p0 or p8) AND (p4 or p12) outside [c-t, c+t]; rejects most pixels (fast_band phase A, and
//                 fast10_quick below for one pixel);
//   fast10_full : the 16-pixel brighter/darker masks and the run-of-10 test.
__device__ __forceinline__ bool fast10_quick(const uint8_t* p, int lp, int t) {
  const int c = p[0], cb = c + t, c_b = c - t;
  const int p0 = p[3 * lp], p8 = p[-3 * lp];
  if (!(p0 > cb || p0 < c_b || p8 > cb || p8 < c_b)) return false;
  const int p4 = p[3], p12 = p[-3];
  return p4 > cb || p4 < c_b || p12 > cb || p12 < c_b;
}
__device__ __forceinline__ bool fast10_full(const uint8_t* p, int lp, int t) {
  const int c = p[0], cb = c + t, c_b = c - t;
  unsigned mb = 0, md = 0;
#define RINGPIX(k, dx, dy) { const int v = p[(dx) + (dy) * lp]; mb |= (unsigned)(v > cb) << (k); md |= (unsigned)(v < c_b) << (k); }
  RINGPIX(0, 0, 3) RINGPIX(1, 1, 3) RINGPIX(2, 2, 2) RINGPIX(3, 3, 1) RINGPIX(4, 3, 0) RINGPIX(5, 3, -1)
  RINGPIX(6, 2, -2) RINGPIX(7, 1, -3) RINGPIX(8, 0, -3) RINGPIX(9, -1, -3) RINGPIX(10, -2, -2)
  RINGPIX(11, -3, -1) RINGPIX(12, -3, 0) RINGPIX(13, -3, 1) RINGPIX(14, -2, 2) RINGPIX(15, -1, 3)
#undef RINGPIX
  return ring_run10(mb) || ring_run10(md);
}

// Stage rows [gy0, gy0+nrows) of an image into LDS (row pitch lp, 16-B aligned). Rows outside the image are skipped.
__device__ __forceinline__ void stage_rows(uint8_t* tile, int lp, const uint8_t* img, int pitch, int w, int h,
                                           int gy0, int nrows) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
  for (int r = wave; r < nrows; r += nwave) {
    const int gy = gy0 + r;
    if (gy < 0 || gy >= h) continue;
    const uint8_t* src = img + (size_t)gy * pitch;
    uint8_t* dst = tile + r * lp;
    int done = 0;
    if ((((uintptr_t)src) & 15) == 0) {
      const int nvec = w >> 4;
      for (int v = lane; v < nvec; v += 64) ((uint4*)dst)[v] = ((const uint4*)src)[v];
      done = nvec << 4;
    }
    for (int i = done + lane; i < w; i += 64) dst[i] = src[i];
  }
}

// FAST over nrows image rows starting at y0; tile row 0 holds image row y0 - HALO.
// Per group of FB_ROWS rows: (A) every pixel runs the quick reject, survivors are appended (wave-aggregated) to an LDS
// candidate list; (B) the full test runs over the dense list and sets bits of the band's corner mask in LDS.
// Finally the mask words and the row counts go to global memory with coalesced stores.
#define FB_ROWS 4
__device__ __forceinline__ void fast_band(const uint8_t* tile, int lp, int y0, int nrows, int w, int h, int thr,
                                          int nchunk, unsigned long long* cmask /* [h][nchunk] */,
                                          int* rowcnt /* [h] */, unsigned long long* mask_lds, unsigned short* cand, int* ncand) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwave = blockDim.x >> 6;
  for (int i = threadIdx.x; i < nrows * nchunk; i += blockDim.x) mask_lds[i] = 0ull;
  for (int r0 = 0; r0 < nrows; r0 += FB_ROWS) {
    if (threadIdx.x == 0) *ncand = 0;
    __syncthreads();
    const int gr = min(FB_ROWS, nrows - r0);
    // (A) quick reject, four pixels per lane: one aligned dword of centres, the dwords 3 rows above / below, and the
    //     pixels 3 to the left / right assembled from the neighbouring aligned dwords (v_alignbyte).  The compiler reads
    //     the bytes straight out of the registers (SDWA), so the LDS sees 5 dword reads per 4 pixels instead of 20 byte reads.
    const int nq = (w + 3) >> 2;                                     // dwords per row
#ifndef VSLAM_FE_SKIP_QUICK
    for (int it = wave * 64 + lane; it - lane < gr * nq; it += nwave * 64) {
      const int r = r0 + it / nq, q = it - (it / nq) * nq;
      const int y = y0 + r, x0 = q << 2;
      unsigned pass = 0;
      if (it < gr * nq && y >= HALO && y < h - HALO) {               // cvfast.cpp:6113-6117
        const uint8_t* row = tile + (r + HALO) * lp + x0;
        const unsigned cw = *(const unsigned*)row, lw = *(const unsigned*)(row - 4), rw = *(const unsigned*)(row + 4);
        const unsigned uw = *(const unsigned*)(row + 3 * lp), dw = *(const unsigned*)(row - 3 * lp);
        const unsigned p12w = __builtin_amdgcn_alignbyte(cw, lw, 1);   // pixels x-3 .. x
        const unsigned p4w = __builtin_amdgcn_alignbyte(rw, cw, 3);    // pixels x+3 .. x+6
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int x = x0 + j;
          const int c = (cw >> (8 * j)) & 255u, cb = c + thr, c_b = c - thr;
          const int p0 = (uw >> (8 * j)) & 255u, p8 = (dw >> (8 * j)) & 255u;
          const int p4 = (p4w >> (8 * j)) & 255u, p12 = (p12w >> (8 * j)) & 255u;
          const bool ok = (p0 > cb || p0 < c_b || p8 > cb || p8 < c_b) && (p4 > cb || p4 < c_b || p12 > cb || p12 < c_b);
          if (ok && x >= HALO && x < w - HALO) pass |= 1u << j;
        }
      }
      unsigned long long bm[4];
      int tot = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) { bm[j] = __ballot((pass >> j) & 1u); tot += __popcll(bm[j]); }
      if (tot) {
        int base = 0;
        if (lane == 0) base = atomicAdd(ncand, tot);
        base = __shfl(base, 0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if ((pass >> j) & 1u) cand[base + __popcll(bm[j] & ((1ull << lane) - 1ull))] = (unsigned short)((r << 12) | (x0 + j));
          base += __popcll(bm[j]);
        }
      }
    }
#endif
    __syncthreads();
    const int n = *ncand;
#ifndef VSLAM_FE_SKIP_FULL
    for (int i = threadIdx.x; i < n; i += blockDim.x) {               // (B) full segment test on packed lanes
      const int r = cand[i] >> 12, x = cand[i] & 4095;
      if (fast10_full(tile + (r + HALO) * lp + x, lp, thr)) atomicOr(&mask_lds[r * nchunk + (x >> 6)], 1ull << (x & 63));
    }
#endif
    __syncthreads();
  }
  for (int i = threadIdx.x; i < nrows * nchunk; i += blockDim.x) cmask[(size_t)y0 * nchunk + i] = mask_lds[i];
  if ((int)threadIdx.x < nrows) {
    int c = 0;
    for (int k = 0; k < nchunk; k++) c += __popcll(mask_lds[threadIdx.x * nchunk + k]);
    rowcnt[y0 + threadIdx.x] = c;
  }
}

// 2x2 box mean of nrows_out output rows: src rows (2j, 2j+1) of an LDS tile -> LDS tile + global.
__device__ __forceinline__ void halve_rows(const uint8_t* src, int slp, uint8_t* dst, int dlp, int wout, int nrows_out,
                                           uint8_t* gdst, int gpitch) {
  const int q = wout >> 2;
  for (int it = threadIdx.x; it < nrows_out * q; it += blockDim.x) {
    const int j = it / q, xq = it - j * q;
    const uint2 a = *(const uint2*)(src + (2 * j) * slp + 8 * xq);
    const uint2 b = *(const uint2*)(src + (2 * j + 1) * slp + 8 * xq);
    uint32_t o = 0;
#define HQ(k, wa, wb, sh) { const unsigned s = ((wa >> sh) & 255u) + ((wa >> (sh + 8)) & 255u) + ((wb >> sh) & 255u) + ((wb >> (sh + 8)) & 255u) + 2u; o |= (s >> 2) << (8 * k); }
    HQ(0, a.x, b.x, 0) HQ(1, a.x, b.x, 16) HQ(2, a.y, b.y, 0) HQ(3, a.y, b.y, 16)
#undef HQ
    if (dst) *(uint32_t*)(dst + j * dlp + 4 * xq) = o;
    *(uint32_t*)(gdst + (size_t)j * gpitch + 4 * xq) = o;
  }
  const int rem = wout - (q << 2);
  for (int it = threadIdx.x; it < nrows_out * rem; it += blockDim.x) {
    const int j = it / rem, x = (q << 2) + (it - j * rem);
    const uint8_t* r0 = src + (2 * j) * slp + 2 * x;
    const uint8_t* r1 = r0 + slp;
    const uint8_t o = (uint8_t)((r0[0] + r0[1] + r1[0] + r1[1] + 2) >> 2);
    if (dst) dst[j * dlp + x] = o;
    gdst[(size_t)j * gpitch + x] = o;
  }
}

__global__ __launch_bounds__(FE_THREADS) void k_pyr_fast0(FeArgs a, int lp0, int lp1, int lp2) {
  extern __shared__ __align__(16) uint8_t lds[];
  uint8_t* t0 = lds;                               // (BAND + 2*HALO) rows of level 0
  uint8_t* t1 = t0 + (BAND + 2 * HALO) * lp0;      // BAND/2 rows of level 1
  uint8_t* t2 = t1 + (BAND / 2) * lp1;             // BAND/4 rows of level 2
  unsigned long long* mask_lds = (unsigned long long*)(((uintptr_t)(t2 + (BAND / 4) * lp2) + 15) & ~(uintptr_t)15);
  unsigned short* cand = (unsigned short*)(mask_lds + BAND * a.nchunk[0]);
  int* ncand = (int*)(cand + FB_ROWS * lp0);
  const int b = blockIdx.x, s = fe_stream_of(a, blockIdx.y);
  const uint8_t* in = a.in + (size_t)s * a.in_sstride;
  const int y0 = b * BAND;
  stage_rows(t0, lp0, in, a.in_pitch, a.w[0], a.h[0], y0 - HALO, BAND + 2 * HALO);
  __syncthreads();
  // pyramid rows owned by this band (jni/KeyFrame.cc:19-23; 2:1 area filter)
  int n1 = min(BAND / 2, a.h[1] - y0 / 2); n1 = max(n1, 0);
  halve_rows(t0 + HALO * lp0, lp0, t1, lp1, a.w[1], n1, a.lvl[1] + (size_t)s * a.lvl_sstride[1] + (size_t)(y0 / 2) * a.lvl_pitch[1], a.lvl_pitch[1]);
  __syncthreads();
  int n2 = min(BAND / 4, a.h[2] - y0 / 4); n2 = max(n2, 0);
  halve_rows(t1, lp1, t2, lp2, a.w[2], n2, a.lvl[2] + (size_t)s * a.lvl_sstride[2] + (size_t)(y0 / 4) * a.lvl_pitch[2], a.lvl_pitch[2]);
  __syncthreads();
  int n3 = min(BAND / 8, a.h[3] - y0 / 8); n3 = max(n3, 0);
  halve_rows(t2, lp2, nullptr, 0, a.w[3], n3, a.lvl[3] + (size_t)s * a.lvl_sstride[3] + (size_t)(y0 / 8) * a.lvl_pitch[3], a.lvl_pitch[3]);
  // FAST-10 on the level-0 rows of the band
  const int nrows = min(BAND, a.h[0] - y0);
  fast_band(t0, lp0, y0, nrows, a.w[0], a.h[0], a.thr[0], a.nchunk[0],
            a.cmask[0] + (size_t)s * a.h[0] * a.nchunk[0], a.rowcnt[0] + (size_t)s * a.h[0], mask_lds, cand, ncand);
}

__global__ __launch_bounds__(FE_THREADS) void k_fast_lvl(FeArgs a) {
  extern __shared__ __align__(16) uint8_t lds[];
  int l = 1;
  if ((int)blockIdx.x >= a.band_first[2]) l = 2;
  if ((int)blockIdx.x >= a.band_first[3]) l = 3;
  const int b = blockIdx.x - a.band_first[l], s = fe_stream_of(a, blockIdx.y);
  const int lp = (a.w[l] + 15) & ~15;
  uint8_t* t = lds;
  unsigned long long* mask_lds = (unsigned long long*)(((uintptr_t)(t + (BAND + 2 * HALO) * lp) + 15) & ~(uintptr_t)15);
  unsigned short* cand = (unsigned short*)(mask_lds + BAND * a.nchunk[l]);
  int* ncand = (int*)(cand + FB_ROWS * lp);
  const int y0 = b * BAND;
  stage_rows(t, lp, a.lvl[l] + (size_t)s * a.lvl_sstride[l], a.lvl_pitch[l], a.w[l], a.h[l], y0 - HALO, BAND + 2 * HALO);
  __syncthreads();
  const int nrows = min(BAND, a.h[l] - y0);
  fast_band(t, lp, y0, nrows, a.w[l], a.h[l], a.thr[l], a.nchunk[l],
            a.cmask[l] + (size_t)s * a.h[l] * a.nchunk[l], a.rowcnt[l] + (size_t)s * a.h[l], mask_lds, cand, ncand);
}

// ---------------------------------------------------------------------------------------------------------------
// The same FAST-10 sweep WITHOUT staging the image in LDS (the form used whenever the level widths are multiples of 4 and
// the input is 16-B aligned; the band kernels above stay as the general path).  One lane owns a strip 16 pixels wide and
// SL_R rows tall and walks down it: one 16-B global load per row, a sliding window of seven rows in registers -- the centre
// row's neighbours 3 to the left / right come from the neighbouring lanes' registers (wave shuffles; the two edge lanes of a
// wavefront load one extra dword), the pixels 3 above / below are the window's first and last row -- so the quick reject
// reads nothing but registers (it was LDS-issue bound).  Level 0 also produces its share of levels
// 1..3 from the same registers (2x2 sums by v_perm + v_sad_u8) with lane-contiguous stores.
// Quick reject (cvfast.cpp:6088-9241 as a filter): ten contiguous ring pixels contain two ADJACENT compass pixels
// (0, 4, 8, 12), so a corner has such a pair both brighter than c + t or both darker than c - t.  ~2 % of the pixels of the
// feeder's frames pass (0.4 % are corners).  Every eight rows a wavefront compacts its survivors (prefix sum of the lanes'
// bit counts) into its own LDS list and runs the full 16-pixel run-of-10 test on them with dense lanes, the ring read back
// through L1/L2, 12 bytes per ring row; corners are OR-ed into the workgroup's mask words in LDS, which leave with coalesced
// stores together with the row counts.  A workgroup owns 256 / (w / 16) whole strips-rows ("bands") of consecutive frames.
#define SL_RMAX 64         // most rows of a strip; the height R (a multiple of 8: the three halvings stay inside a strip) is chosen per launch
#define SL_THREADS 256
#define SL_CAP 1024        // entries of a wavefront's candidate list (one row of a wavefront: 64 lanes x 16 pixels)
#define SL_RING 8          // row steps per round of the strip loop = named register sets of the window: its seven rows plus the one in flight
#define SL_AHEAD (SL_RING - 7)

struct SlArgs {
  int w16[NLEV], nb[NLEV], bpw[NLEV], wg_first[NLEV + 1];   // strips per row, bands per frame, bands per workgroup, first workgroup of a level
  int R[NLEV];                                              // rows of a strip
  int S;
};

// sum of the 2x2 block (wa byte k, k+1; wb byte k, k+1) + 2, >> 2, for k = 0 and k = 2 -> two output pixels in bits 0..15
DEVFN unsigned sl_half2(unsigned wa, unsigned wb) {
  const unsigned q0 = __builtin_amdgcn_perm(wb, wa, 0x05040100u), q1 = __builtin_amdgcn_perm(wb, wa, 0x07060302u);
  return (__builtin_amdgcn_sad_u8(q0, 0u, 2u) >> 2) | ((__builtin_amdgcn_sad_u8(q1, 0u, 2u) >> 2) << 8);
}
DEVFN unsigned sl_half4(unsigned a0, unsigned a1, unsigned b0, unsigned b1) { return sl_half2(a0, b0) | (sl_half2(a1, b1) << 16); }

// full segment test of pixel (x, y) of an image read through the caches: per ring row ONE 12-byte load that covers x - 3 .. x + 3.
// It starts at the aligned dword xb that holds x - 3, or one dword earlier where xb + 12 would pass the end of the row (x - 3 then
// lies in the row's last two dwords and the ring ends inside them), so nothing beyond the row's w pixels is ever read.  One address
// per row instead of two leaves the registers, beside the strip's window, to have all seven loads in flight together.
struct __attribute__((packed, aligned(4))) SlRow3 { unsigned x, y, z; };
DEVFN bool sl_full_test(const uint8_t* img, int pitch, int w, int x, int y, int thr) {
  const int xb = (x - 3) & ~3, o = (x - 3) & 3;
  const int xl = min(xb, w - 12);                                    // w >= 16
  const bool late = xl != xb;                                        // x - 3 is in the load's second dword
  unsigned A[7], B[7], v0[7], v1[7], v2[7];
  const uint8_t* r = img + (size_t)(y - 3) * pitch + xl;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const SlRow3 v = *(const SlRow3*)r;
    v0[k] = v.x; v1[k] = v.y; v2[k] = v.z;
    r += pitch;
  }
  // All 21 dwords are live here, so the loads are issued together and cost one round trip.  Left to itself the scheduler, short of
  // registers beside the strip's window, waits for the first rows before it asks for the last.
  asm volatile("" : "+v"(v0[0]), "+v"(v0[1]), "+v"(v0[2]), "+v"(v0[3]), "+v"(v0[4]), "+v"(v0[5]), "+v"(v0[6]),
                    "+v"(v1[0]), "+v"(v1[1]), "+v"(v1[2]), "+v"(v1[3]), "+v"(v1[4]), "+v"(v1[5]), "+v"(v1[6]));
  asm volatile("" : "+v"(v2[0]), "+v"(v2[1]), "+v"(v2[2]), "+v"(v2[3]), "+v"(v2[4]), "+v"(v2[5]), "+v"(v2[6]));
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const unsigned lo = late ? v1[k] : v0[k], mid = late ? v2[k] : v1[k];
    A[k] = __builtin_amdgcn_alignbyte(mid, lo, o);                   // pixels x-3 .. x
    B[k] = __builtin_amdgcn_alignbyte(v2[k], mid, o);                // pixels x+1 .. x+4 (x+4 is not on the ring: when late, o < 2 and it is a byte of mid or any byte)
  }
  const int c = (A[3] >> 24) & 255u, cb = c + thr, c_b = c - thr;
  unsigned mb = 0, md = 0;                                          // ring pixel k -> bit k: the sign bits of cb - v / v - c_b are shifted in, k = 15 first
#define SLPIX(k, dx, dy) { const int v = (int)(((dx) <= 0 ? (A[(dy) + 3] >> (8 * ((dx) + 3))) : (B[(dy) + 3] >> (8 * ((dx) - 1)))) & 255u); mb = __builtin_amdgcn_alignbit(mb, (unsigned)(cb - v), 31); md = __builtin_amdgcn_alignbit(md, (unsigned)(v - c_b), 31); }
  SLPIX(15, -1, 3) SLPIX(14, -2, 2) SLPIX(13, -3, 1) SLPIX(12, -3, 0) SLPIX(11, -3, -1) SLPIX(10, -2, -2)
  SLPIX(9, -1, -3) SLPIX(8, 0, -3) SLPIX(7, 1, -3) SLPIX(6, 2, -2) SLPIX(5, 3, -1) SLPIX(4, 3, 0)
  SLPIX(3, 3, 1) SLPIX(2, 2, 2) SLPIX(1, 1, 3) SLPIX(0, 0, 3)
#undef SLPIX
  return ring_run10(mb) || ring_run10(md);
}

template <bool PYR>
__global__ __launch_bounds__(SL_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_fast_slide(FeArgs a, SlArgs q) {
  extern __shared__ __align__(16) uint8_t lds[];
  int l = 0;
  if (!PYR) { l = 1; if ((int)blockIdx.x >= q.wg_first[2]) l = 2; if ((int)blockIdx.x >= q.wg_first[3]) l = 3; }
  const int wg = (int)blockIdx.x - (PYR ? 0 : q.wg_first[l]);
  const int w = a.w[l], h = a.h[l], nchunk = a.nchunk[l], thr = a.thr[l];
  const int W16 = q.w16[l], nb = q.nb[l], bpw = q.bpw[l], SL_R = q.R[l], SL_NSTEP = SL_R + 2 * HALO;
  const uint8_t* img = PYR ? a.in : a.lvl[l];
  const size_t sstride = PYR ? a.in_sstride : a.lvl_sstride[l];
  const int pitch = PYR ? a.in_pitch : a.lvl_pitch[l];
  int4* tb = (int4*)lds;                                             // per thread: stream, first row, first column, band of the workgroup
  unsigned short* lists = (unsigned short*)(tb + SL_THREADS);
  unsigned long long* mask = (unsigned long long*)(lists + (SL_THREADS / 64) * SL_CAP);   // [bpw][R][nchunk]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned short* list = lists + wave * SL_CAP;
  const int bl = tid / W16, cg = tid - bl * W16;
  const long gband = (long)wg * bpw + bl;
  const bool active = bl < bpw && gband < (long)q.S * nb;
  const int ord = active ? (int)(gband / nb) : 0, b = active ? (int)(gband - (long)ord * nb) : 0;
  const int s = active ? fe_stream_of(a, ord) : 0;
  const int yb = b * SL_R, x0 = cg * 16;
  tb[tid] = make_int4(s, yb, x0, active ? bl : -1);
  for (int i = tid; i < bpw * SL_R * nchunk; i += SL_THREADS) mask[i] = 0ull;
  __syncthreads();
  const uint8_t* base = img + (size_t)s * sstride + x0;
  unsigned xvalid = 0;                                               // columns of the strip FAST runs on (cvfast.cpp:6113-6117)
  for (int j = 0; j < 16; j++) if (x0 + j >= HALO && x0 + j < w - HALO) xvalid |= 1u << j;
  if (!active) xvalid = 0;
  const bool eL = active && lane == 0 && cg > 0, eR = active && lane == 63 && cg < W16 - 1;

  // Row step i of the strip (image row yb - 3 + i) straight into the window slot it is read from.  The address is clamped into the
  // image: a row outside it is never consumed (the pyramid and the quick reject test their own row against h below), so no register
  // is cleared.  r[0] / r[5] are loaded by the edge lanes of a wavefront only; the other lanes take theirs from their neighbours.
  auto load_row = [&](int i, unsigned (&r)[6]) {
    const int y = min(max(yb - HALO + i, 0), h - 1);
    const uint8_t* p = base + (size_t)y * pitch;
    const uint4 v = *(const uint4*)p;
    r[1] = v.x; r[2] = v.y; r[3] = v.z; r[4] = v.w;
    if (eL) r[0] = *(const unsigned*)(p - 4);
    if (eR) r[5] = *(const unsigned*)(p + 16);
  };
  // The window and the prefetch are one ring of SL_RING named register sets: seven rows of window and one row in flight.  Row step i
  // lives in slot i % 8 from its load to its last use as row y - 3, and the loop is unrolled by 8, so the ring closes and no row is
  // ever copied; a strip is a multiple of 8 rows, so which pyramid rows a step closes is known when it is compiled.
  // (Two rows in flight, a ring of 9, bought nothing: the row is waited for at the end of the step that asked for it either way, and
  // its six registers more left the full test too few to have its loads in flight together.)
  // Per slot: [0] left neighbour dword, [1..4] own, [5] right neighbour.
  unsigned W[SL_RING][6];
#pragma unroll
  for (int u = 0; u < SL_RING; u++) W[u][0] = W[u][5] = 0;           // [1..4] are loaded before they are read
#pragma unroll
  for (int k = 0; k < SL_AHEAD; k++) load_row(k, W[k]);
  unsigned l1p[2] = {0, 0}, l2p = 0;                                 // pyramid pieces waiting for their second row

  for (int i0 = 0; i0 < SL_NSTEP; i0 += SL_RING) {
    unsigned pw[(SL_RING + 1) / 2];                                  // quick-reject survivors of this round: 16 bits per row
#pragma unroll
    for (int k = 0; k < (SL_RING + 1) / 2; k++) pw[k] = 0;
#pragma unroll
    for (int u = 0; u < SL_RING; u++) {
      const int i = i0 + u;
      if (i >= SL_NSTEP) continue;
      load_row(i + SL_AHEAD, W[(u + SL_AHEAD) % SL_RING]);
      const unsigned nl = __shfl_up(W[u][4], 1), nr = __shfl_down(W[u][1], 1);
      if (lane != 0) W[u][0] = nl;
      if (lane != 63) W[u][5] = nr;
      if (PYR) {                                                     // jni/KeyFrame.cc:19-23 (2:1 area filter)
        const int rb = i - HALO, y = yb + rb;                        // row of the band
        if (active && rb >= 0 && rb < SL_R && y < h && (rb & 1)) {
          const int up = (u + SL_RING - 1) % SL_RING;
          const unsigned o0 = sl_half4(W[up][1], W[up][2], W[u][1], W[u][2]), o1 = sl_half4(W[up][3], W[up][4], W[u][3], W[u][4]);
          if ((y >> 1) < a.h[1]) *(uint2*)(a.lvl[1] + (size_t)s * a.lvl_sstride[1] + (size_t)(y >> 1) * a.lvl_pitch[1] + cg * 8) = make_uint2(o0, o1);
          if ((rb & 3) == 3) {
            const unsigned o2 = sl_half4(l1p[0], l1p[1], o0, o1);
            if ((y >> 2) < a.h[2]) *(unsigned*)(a.lvl[2] + (size_t)s * a.lvl_sstride[2] + (size_t)(y >> 2) * a.lvl_pitch[2] + cg * 4) = o2;
            if ((rb & 7) == 7) {
              int s3 = s;                                            // opaque: the level-3 slot's address is worked out here, once in eight rows, not kept in two registers all along
              asm volatile("" : "+v"(s3));
              if ((y >> 3) < a.h[3]) *(unsigned short*)(a.lvl[3] + (size_t)s3 * a.lvl_sstride[3] + (size_t)(y >> 3) * a.lvl_pitch[3] + cg * 2) = (unsigned short)sl_half2(l2p, o2);
            } else l2p = o2;
          } else { l1p[0] = o0; l1p[1] = o1; }
        }
      }
      // quick reject on the centre row (row step i - 3): band row rel = i - 6.  Row y + 3 is slot u, row y - 3 row step i - 6.
      const int rel = i - 2 * HALO, yc = yb + rel;
      if (rel >= 0 && yc >= HALO && yc < h - HALO) {                  // uniform but for yc (per band)
        const int sc = (u + SL_RING - 3) % SL_RING, sd = (u + SL_RING - 6) % SL_RING;
        const unsigned pass = fast_reject16(W[sc], W[u], W[sd], thr) & xvalid;   // two pixels per instruction, fast_reject_dev.h
        pw[u >> 1] |= pass << (16 * (u & 1));
      }
    }
    // ---- the round's survivors: compact per wavefront, full test on dense lanes ----
    const int relg = i0 - 2 * HALO;                                  // band row of the round's slot 0
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < (SL_RING + 1) / 2; k++) cnt += __popc(pw[k]);
    const int tot = wave_sum(cnt);
#ifdef VSLAM_SL_SKIP_FLUSH
    if (tot != 123456) continue;
#endif
    if (tot == 0) continue;
    const int nsub = tot <= SL_CAP ? 1 : SL_RING;                    // a round that overflows the list goes row by row
    for (int sub = 0; sub < nsub; sub++) {
      unsigned m4[(SL_RING + 1) / 2];
      int c4 = 0;
#pragma unroll
      for (int k = 0; k < (SL_RING + 1) / 2; k++) {
        m4[k] = nsub == 1 ? pw[k] : ((sub >> 1) == k ? (pw[k] & (0xFFFFu << (16 * (sub & 1)))) : 0u);
        c4 += __popc(m4[k]);
      }
      int inc = c4;
      for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
      const int n = __shfl(inc, 63);
      int pos = inc - c4;
#pragma unroll
      for (int k = 0; k < (SL_RING + 1) / 2; k++) {
        unsigned m = m4[k];
        while (m) {
          const int bit = __ffs((int)m) - 1;
          list[pos++] = (unsigned short)((lane << 8) | (k * 32 + bit));   // lane, row of the round, column
          m &= m - 1;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (int k = lane; k < n; k += 64) {
        const int e = list[k];
        const int4 t = tb[wave * 64 + (e >> 8)];
        const int rr = relg + ((e >> 4) & 15), x = t.z + (e & 15), y = t.y + rr;
#ifdef VSLAM_SL_SKIP_FULL
        if (x == 7 && y == 7)
#else
        if (sl_full_test(img + (size_t)t.x * sstride, pitch, w, x, y, thr))
#endif
          atomicOr(&mask[((size_t)t.w * SL_R + rr) * nchunk + (x >> 6)], 1ull << (x & 63));
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  // masks and row counts of the workgroup's bands
  const int per = SL_R * nchunk;
  for (int i = tid; i < bpw * per; i += SL_THREADS) {
    const int bb = i / per, rem = i - bb * per, row = rem / nchunk, c = rem - row * nchunk;
    const int4 t = tb[bb * W16];
    if (t.w >= 0 && t.y + row < h) a.cmask[l][((size_t)t.x * h + t.y + row) * nchunk + c] = mask[i];
  }
  for (int i = tid; i < bpw * SL_R; i += SL_THREADS) {
    const int bb = i / SL_R, row = i - bb * SL_R;
    const int4 t = tb[bb * W16];
    if (t.w < 0 || t.y + row >= h) continue;
    int c = 0;
    for (int k = 0; k < nchunk; k++) c += __popcll(mask[(size_t)i * nchunk + k]);
    a.rowcnt[l][(size_t)t.x * h + t.y + row] = c;
  }
}

// Raster-ordered corner lists + row LUT from the corner bit-masks, one WAVEFRONT per (band of rows, level, stream) and no barrier: the
// wavefront adds the row counts above its band (its list offset = lut of its first row; the loads are issued together, four per lane
// and trip), scans the popcounts of its band's mask words (word index = row * nchunk + chunk, i.e. raster order; a lane owns one to
// four consecutive words) and every lane expands its words at its scanned offset -> the list is bit-exactly the reference's push_back
// order (cvfast.cpp:9237-9238) with no ordered atomics; lut[y] is the offset of the first word of row y (jni/KeyFrame.cc:43-49).
// The grid's x counts the bands the four levels really have (CpArgs::first), four to a workgroup whose wavefronts never meet.
// (A workgroup of four wavefronts per band of level-0 height spent 63 % of its cycles waiting at its four barriers, and three quarters
// of the workgroups of levels 1..3 returned at once; one workgroup per (level, stream) walking the whole level was slower still.)
#define COMPACT_THREADS 256
#define COMPACT_WORDS 256   // most mask words of a band: four per lane
struct CpArgs {
  int first[NLEV + 1];      // first band of each level in the grid's x order, [NLEV] = all bands
  int rows[NLEV];           // rows per band: COMPACT_WORDS / nchunk, so 4 (4096 pixels wide, 64 words a row) to 256
};
static CpArgs fe_compact_args(const FeArgs& a) {
  CpArgs c;
  c.first[0] = 0;
  for (int l = 0; l < NLEV; l++) {
    c.rows[l] = COMPACT_WORDS / a.nchunk[l];                        // nchunk <= 64: vslam_create accepts no level wider than 4096
    c.first[l + 1] = c.first[l] + (a.h[l] + c.rows[l] - 1) / c.rows[l];
  }
  return c;
}
static dim3 fe_compact_grid(const CpArgs& c, int S) { return dim3((c.first[NLEV] + COMPACT_THREADS / 64 - 1) / (COMPACT_THREADS / 64), S); }

__global__ __launch_bounds__(COMPACT_THREADS) void k_compact(FeArgs a, CpArgs q) {
  const int lane = threadIdx.x & 63;
  const int gb = (int)blockIdx.x * (COMPACT_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (gb >= q.first[NLEV]) return;
  int l = 0;
  if (gb >= q.first[1]) l = 1;
  if (gb >= q.first[2]) l = 2;
  if (gb >= q.first[3]) l = 3;
  const int s = fe_stream_of(a, blockIdx.y);
  const int h = a.h[l], nchunk = a.nchunk[l], cap = a.cap[l];
  const int y0 = (gb - q.first[l]) * q.rows[l];
  const int nrows = min(q.rows[l], h - y0);
  const int* rc = a.rowcnt[l] + (size_t)s * h;
  const int nw = nrows * nchunk;
  const unsigned long long* cm = a.cmask[l] + ((size_t)s * h + y0) * nchunk;
  uint32_t* out = a.corners[l] + (size_t)s * cap;
  int* lut = a.rowlut[l] + (size_t)s * (h + 1);
  int above = 0;
  for (int y = lane; y < y0; y += 256) {                            // the row counts above the band, four loads in flight per lane
    const int r0 = rc[y], r1 = y + 64 < y0 ? rc[y + 64] : 0, r2 = y + 128 < y0 ? rc[y + 128] : 0, r3 = y + 192 < y0 ? rc[y + 192] : 0;
    above += (r0 + r1) + (r2 + r3);
  }
  const int per = (nw + 63) >> 6;                                    // 1..4 consecutive words per lane
  const int lo = min(lane * per, nw), hi = min(lo + per, nw);
  unsigned long long m[COMPACT_WORDS / 64];
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < COMPACT_WORDS / 64; k++) {
    m[k] = lo + k < hi ? cm[lo + k] : 0ull;
    cnt += __popcll(m[k]);
  }
  const int first = wave_sum(above);
  int inc = cnt;
  for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(inc, d); if (lane >= d) inc += v; }
  int pos = first + inc - cnt;
  const int total = first + __shfl(inc, 63);
  int y = y0 + lo / nchunk, c = lo - (lo / nchunk) * nchunk;         // row and chunk of the lane's first word
#pragma unroll
  for (int k = 0; k < COMPACT_WORDS / 64; k++) {
    if (lo + k >= hi) break;
    if (c == nchunk) { c = 0; y++; }
    if (c == 0) lut[y] = min(pos, cap);
    unsigned long long mm = m[k];
    while (mm) {
      const int bit = __ffsll((long long)mm) - 1;
      if (pos < cap) out[pos] = (uint32_t)((c << 6) + bit) | ((uint32_t)y << 16);
      pos++;
      mm &= mm - 1;
    }
    c++;
  }
  if (lane == 0 && y0 + nrows == h) {                                // the last band of the level closes the list
    lut[h] = min(total, cap);
    a.ncorners[s * NLEV + l] = min(total, cap);
    if (total > cap) *a.overflow = 1;
  }
}

// Subset step from device memory: image i of the caller's buffer into the owned level-0 slot of stream list[i], all n images in one
// launch (n two-dimensional copies would cost the host more than the front end costs the device).  One workgroup per band of
// GATHER_ROWS rows of one image; 16 B per lane when the source allows it, bytes otherwise (any base address, pitch and stride).
#define GATHER_ROWS 16
__global__ __launch_bounds__(FE_THREADS) void k_gather_level0(const uint8_t* in, size_t in_sstride, int in_pitch, uint8_t* out, size_t out_sstride,
                                                             int out_pitch /* multiple of 64, slots 16-B aligned */, int w, int h, const int* list) {
  const int i = blockIdx.y, s = list[i];
  const int y0 = blockIdx.x * GATHER_ROWS, nrows = min(GATHER_ROWS, h - y0);
  const uint8_t* src = in + (size_t)i * in_sstride + (size_t)y0 * in_pitch;
  uint8_t* dst = out + (size_t)s * out_sstride + (size_t)y0 * out_pitch;
  int done = 0;
  if ((((uintptr_t)src) & 15) == 0 && (in_pitch & 15) == 0) {
    const int nvec = w >> 4;
    for (int t = threadIdx.x; t < nrows * nvec; t += FE_THREADS) {
      const int r = t / nvec, v = t - r * nvec;
      ((uint4*)(dst + (size_t)r * out_pitch))[v] = ((const uint4*)(src + (size_t)r * in_pitch))[v];
    }
    done = nvec << 4;
  }
  const int rem = w - done;
  for (int t = threadIdx.x; t < nrows * rem; t += FE_THREADS) {
    const int r = t / rem, x = done + (t - r * rem);
    dst[(size_t)r * out_pitch + x] = src[(size_t)r * in_pitch + x];
  }
}

// ---- MakeKeyFrame_Rest: FAST score + non-max (jni/KeyFrame.cc:53-63) ---------------------------------------------
struct NmArgs {
  const uint8_t* img[NLEV]; size_t img_sstride[NLEV]; int img_pitch[NLEV];
  int h[NLEV], cap[NLEV];
  const uint32_t* corners[NLEV]; const int* rowlut[NLEV]; const int* ncorners;
  int* scores[NLEV]; uint32_t* maxcorners[NLEV]; int* nmax;
  int barrier, quirk;
  const TrackerState* gate;   // non-null: only the streams whose tracker asked for a keyframe (kf_pending)
  const unsigned char* held;  // the frame's subset mask (null: a full step): a held stream has no front-end products
};

// compute_fast_score_old (cvfast.cpp:9337-9393): one lane per corner.
__global__ __launch_bounds__(FE_THREADS) void k_score(NmArgs a) {
  const int l = blockIdx.y, s = blockIdx.z;
  if (!trk_in_step(a.held, s) || (a.gate && !a.gate[s].kf_pending)) return;
  const int n = a.ncorners[s * NLEV + l];
  for (int i = blockIdx.x * FE_THREADS + threadIdx.x; i < n; i += gridDim.x * FE_THREADS) {
  const uint32_t cxy = a.corners[l][(size_t)s * a.cap[l] + i];
  const int x = cxy & 0xFFFF, y = cxy >> 16, lp = a.img_pitch[l];
  const uint8_t* p = a.img[l] + (size_t)s * a.img_sstride[l] + (size_t)y * lp + x;
  const int cb = p[0] + a.barrier, c_b = p[0] - a.barrier;
  int sp = 0, sn = 0;
#define SC(dx, dy) { const int v = p[(dx) + (dy) * lp]; if (v > cb) sp += v - cb; else if (v < c_b) sn += c_b - v; }
  SC(0, 3) SC(1, 3) SC(2, 2) SC(3, 1) SC(3, 0) SC(3, -1) SC(2, -2) SC(1, -3)
  SC(0, -3) SC(-1, -3) SC(-2, -2) SC(-3, -1) SC(-3, 0) SC(-3, 1) SC(-2, 2) SC(-1, 3)
#undef SC
  a.scores[l][(size_t)s * a.cap[l] + i] = sp > sn ? sp : sn;
  }
}

// nonmax_suppression (cvfast.cpp:9243-9335): a corner survives unless a corner among its 8 neighbours
// has a strictly greater score; rows above/below are found through the row LUT.  One workgroup per
// (stream, level) keeps the output in raster order with a block scan of the keep flags.
__global__ __launch_bounds__(FE_THREADS) void k_nonmax(NmArgs a) {
  __shared__ int wsum[8];
  __shared__ int carry;
  const int l = blockIdx.x, s = blockIdx.y;
  if (!trk_in_step(a.held, s) || (a.gate && !a.gate[s].kf_pending)) return;
  const int n = a.ncorners[s * NLEV + l], cap = a.cap[l], h = a.h[l];
  const uint32_t* cs = a.corners[l] + (size_t)s * cap;
  const int* sc = a.scores[l] + (size_t)s * cap;
  const int* lut = a.rowlut[l] + (size_t)s * (h + 1);
  uint32_t* out = a.maxcorners[l] + (size_t)s * cap;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i0 = 0; i0 < n; i0 += FE_THREADS) {
    const int i = i0 + threadIdx.x;
    int keep = 0;
    uint32_t me = 0;
    if (i < n) {
      me = cs[i];
      const int x = me & 0xFFFF, y = me >> 16, score = sc[i];
      keep = 1;
      if (i > 0) {                                                     // check left  :9276-9279
        const uint32_t c = cs[i - 1];
        if ((int)(c & 0xFFFF) == x - 1 && (int)(c >> 16) == y && sc[i - 1] > score) keep = 0;
      }
      if (keep && i < n - 1) {                                         // check right :9281-9285
        const uint32_t c = cs[i + 1];
        if (a.quirk) {  // reference tests corners[i-1](1) == pos(1); i == 0 reads out of bounds there -> no match
          if (i > 0 && (int)(c & 0xFFFF) == x + 1 && (int)(cs[i - 1] >> 16) == y && sc[i + 1] > score) keep = 0;
        } else {
          if ((int)(c & 0xFFFF) == x + 1 && (int)(c >> 16) == y && sc[i + 1] > score) keep = 0;
        }
      }
      if (keep && y > 0) {                                             // check above :9287-9306
        for (int j = lut[y - 1]; j < lut[y]; j++) {
          const int xx = cs[j] & 0xFFFF;
          if (xx > x + 1) break;
          if (xx >= x - 1 && sc[j] > score) { keep = 0; break; }
        }
      }
      if (keep && y + 1 < h) {                                         // check below :9308-9326
        for (int j = lut[y + 1]; j < lut[y + 2 > h ? h : y + 2]; j++) {
          const int xx = cs[j] & 0xFFFF;
          if (xx > x + 1) break;
          if (xx >= x - 1 && sc[j] > score) { keep = 0; break; }
        }
      }
    }
    int inc = keep;
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(inc, d); if (lane >= d) inc += v; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = carry;
    for (int w = 0; w < wave; w++) base += wsum[w];
    if (keep) out[base + inc - 1] = me;
    __syncthreads();
    if (threadIdx.x == FE_THREADS - 1) carry = base + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) a.nmax[s * NLEV + l] = carry;
}

// KeyFrame::MakeKeyFrame_Rest candidate loop (jni/KeyFrame.cc:66-95): maximal corners inside the 10-px border whose
// Shi-Tomasi score (FindShiTomasiScoreAtPoint, jni/vision/ImageHandler.cpp:124-155, half-window 3) exceeds the minimum,
// in raster order.  One workgroup per (level, stream); one lane per maximal corner; block scan keeps the order.
// The three gradient sums are integers (exact in fp64 in any order), the rest follows the reference expression.
struct CandArgs {
  const uint8_t* img[NLEV]; size_t img_sstride[NLEV]; int img_pitch[NLEV];
  int w[NLEV], h[NLEV], cap[NLEV];
  const uint32_t* maxcorners[NLEV]; const int* nmax;
  uint32_t* cand[NLEV]; double* cand_score[NLEV]; int* ncand;
  double min_score; int border;
  const TrackerState* gate;
  const unsigned char* held;
};

__device__ __forceinline__ double shi_tomasi7(const uint8_t* img, int pitch, int px, int py) {
  int sxx = 0, syy = 0, sxy = 0;
  for (int cy = py - 3; cy <= py + 3; cy++) {
    const uint8_t* r = img + (size_t)cy * pitch;
#pragma unroll
    for (int cx = -3; cx <= 3; cx++) {
      const int dx = (int)r[px + cx + 1] - (int)r[px + cx - 1];
      const int dy = (int)r[px + cx + pitch] - (int)r[px + cx - pitch];
      sxx += dx * dx; syy += dy * dy; sxy += dx * dy;
    }
  }
  const int nPixels = 49;
  const double dXX = (double)sxx / (2.0 * nPixels), dYY = (double)syy / (2.0 * nPixels), dXY = (double)sxy / (2.0 * nPixels);
  return 0.5 * (dXX + dYY - sqrt((dXX + dYY) * (dXX + dYY) - 4 * (dXX * dYY - dXY * dXY)));
}

// ordered append of the lanes with keep != 0 (block-wide, raster order preserved); returns the new carry
__device__ __forceinline__ int block_ordered_slot(int keep, int* wsum, int* carry, int& slot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = keep;
  for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(inc, d); if (lane >= d) inc += v; }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = *carry;
  for (int w = 0; w < wave; w++) base += wsum[w];
  slot = base + inc - 1;
  __syncthreads();
  if (threadIdx.x == FE_THREADS - 1) *carry = base + inc;
  __syncthreads();
  return 0;
}

__global__ __launch_bounds__(FE_THREADS) void k_candidates(CandArgs a) {
  __shared__ int wsum[FE_THREADS / 64];
  __shared__ int carry;
  const int l = blockIdx.x, s = blockIdx.y;
  if (!trk_in_step(a.held, s) || (a.gate && !a.gate[s].kf_pending)) return;
  const int n = a.nmax[s * NLEV + l], cap = a.cap[l];
  const uint32_t* mc = a.maxcorners[l] + (size_t)s * cap;
  const uint8_t* img = a.img[l] + (size_t)s * a.img_sstride[l];
  uint32_t* out = a.cand[l] + (size_t)s * cap;
  double* outs = a.cand_score[l] + (size_t)s * cap;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += FE_THREADS) {
    const int i = i0 + threadIdx.x;
    int keep = 0; uint32_t me = 0; double st = 0.0;
    if (i < n) {
      me = mc[i];
      const int x = me & 0xFFFF, y = me >> 16;
      if (x >= a.border && y >= a.border && x < a.w[l] - a.border && y < a.h[l] - a.border) {   // :72-73
        st = shi_tomasi7(img, a.img_pitch[l], x, y);
        keep = st > a.min_score;                                                                // :81
      }
    }
    int slot;
    block_ordered_slot(keep, wsum, &carry, slot);
    if (keep) { out[slot] = me; outs[slot] = st; }
  }
  __syncthreads();
  if (threadIdx.x == 0) a.ncand[s * NLEV + l] = carry;
}

// MapMaker::ThinCandidates (jni/MapMaker.cc:393-422) on every level: a candidate survives when no measurement of the
// keyframe at the same level or one level up lies within 10 level-pixels (rounded(), :381-386).  One workgroup per
// (level, stream); the busy positions are staged in LDS; the surviving list is compacted in place, order kept.
#define THIN_BUSY_CAP 4096
struct ThinArgs {
  uint32_t* cand[NLEV]; double* cand_score[NLEV]; int* ncand; int cap[NLEV];
  const MeasDev* meas; size_t meas_sstride;   // measurement row of the keyframe per stream
  int new_kf;       // 1: gated on kf_pending and against the keyframe slot k_add_keyframe has just filled (slot n_kf)
  int only_level;   // >= 0: this level only
  size_t kf_row;    // max_points (elements per keyframe row) when new_kf
  const unsigned char* held;   // the frame's subset mask (null: a full step)
};

__global__ __launch_bounds__(FE_THREADS) void k_thin_candidates(ThinArgs a, const TrackerState* st) {
  __shared__ int busy[THIN_BUSY_CAP * 2];
  __shared__ int nbusy;
  __shared__ int wsum[FE_THREADS / 64];
  __shared__ int carry;
  const int l = a.only_level >= 0 ? a.only_level : blockIdx.x, s = blockIdx.y;
  if (!trk_in_step(a.held, s) || (a.new_kf && !st[s].kf_pending)) return;
  const MeasDev* ms = a.meas + (size_t)s * a.meas_sstride + (a.new_kf ? (size_t)st[s].n_kf * a.kf_row : 0);
  const int np = st[s].n_points;
  if (threadIdx.x == 0) { nbusy = 0; carry = 0; }
  __syncthreads();
  const int scale = 1 << l;
  for (int i = threadIdx.x; i < np; i += FE_THREADS) {
    const MeasDev m = ms[i];
    if (!m.valid || !(m.level == l || m.level == l + 1)) continue;
    const double vx = m.root[0] / scale, vy = m.root[1] / scale;
    const int k = atomicAdd(&nbusy, 1);
    if (k < THIN_BUSY_CAP) { busy[2 * k] = (int)(vx > 0.0 ? vx + 0.5 : vx - 0.5); busy[2 * k + 1] = (int)(vy > 0.0 ? vy + 0.5 : vy - 0.5); }
  }
  __syncthreads();
  const int nb = nbusy < THIN_BUSY_CAP ? nbusy : THIN_BUSY_CAP;
  const int n = a.ncand[s * NLEV + l];
  uint32_t* cp = a.cand[l] + (size_t)s * a.cap[l];
  double* cs = a.cand_score[l] + (size_t)s * a.cap[l];
  for (int i0 = 0; i0 < n; i0 += FE_THREADS) {
    const int i = i0 + threadIdx.x;
    int keep = 0; uint32_t me = 0; double sc = 0.0;
    if (i < n) {
      me = cp[i]; sc = cs[i];
      const int cx = me & 0xFFFF, cy = me >> 16;
      keep = 1;
      for (int j = 0; j < nb; j++) {
        const int dx = busy[2 * j] - cx, dy = busy[2 * j + 1] - cy;
        if (dx * dx + dy * dy < 100) { keep = 0; break; }
      }
    }
    int slot;
    block_ordered_slot(keep, wsum, &carry, slot);          // barriers inside: every read of this chunk precedes its writes
    if (keep) { cp[slot] = me; cs[slot] = sc; }            // slot <= i: in-place compaction never overtakes the reads
  }
  __syncthreads();
  if (threadIdx.x == 0) a.ncand[s * NLEV + l] = carry;
}

// ---- host side ------------------------------------------------------------------------------------------------
static void fill_fe_args(vslam_system* sys, FeArgs& a) {
  for (int l = 0; l < NLEV; l++) {
    a.lvl[l] = sys->d_lvl[l];
    a.lvl_sstride[l] = (size_t)sys->geom[l].pitch * sys->geom[l].h;
    a.lvl_pitch[l] = sys->geom[l].pitch;
    a.w[l] = sys->geom[l].w; a.h[l] = sys->geom[l].h; a.nchunk[l] = sys->geom[l].nchunk;
    a.thr[l] = sys->geom[l].thr; a.cap[l] = sys->geom[l].cap;
    a.cmask[l] = sys->fr.cmask[l]; a.rowcnt[l] = sys->fr.rowcnt[l]; a.rowlut[l] = sys->fr.rowlut[l];
    a.corners[l] = sys->fr.corners[l];
  }
  a.ncorners = sys->fr.ncorners;
  a.overflow = sys->fr.overflow;
  a.list = nullptr;
}

// the strip form applies when every level is a multiple of 4 wide and at most 4096, and the level-0 input can be read 16 B at a time
static bool fe_slide_ok(const vslam_system* sys, const FeArgs& a) {
  static const bool off = getenv("VSLAM_FE_BANDS") != nullptr;        // diagnostic: force the band kernels
  if (off) return false;
  for (int l = 0; l < NLEV; l++) if ((a.w[l] & 3) || a.w[l] < 16 || a.w[l] > 4096 || a.h[l] < 7) return false;
  return (((uintptr_t)a.in) & 15) == 0 && (a.in_pitch & 15) == 0 && (a.in_sstride & 15) == 0 && a.in_pitch >= ((a.w[0] + 15) & ~15);
}
static void fe_launch_slide(vslam_system* sys, FeArgs& a, hipStream_t fs, int S) {
  SlArgs q;
  q.S = S;
  int nwg[NLEV];
  size_t lds[NLEV];
  const long slots = 4L * (sys->n_cu > 0 ? sys->n_cu : 256);          // workgroups the device holds at once (four per CU)
  for (int l = 0; l < NLEV; l++) { q.w16[l] = (a.w[l] + 15) >> 4; q.bpw[l] = SL_THREADS / q.w16[l]; }
  // strip height per launch (level 0; levels 1..3): the one that costs the fewest row steps, rounds of resident workgroups x (R + halo)
  auto pick = [&](int l0, int l1) {
    long best = -1; int bestR = 32;
    for (int R = 16; R <= SL_RMAX; R += 8) {
      long wgs = 0;
      bool fits = true;                                                // 64 KB of dynamic LDS
      for (int l = l0; l <= l1; l++) {
        wgs += ((long)S * ((a.h[l] + R - 1) / R) + q.bpw[l] - 1) / q.bpw[l];
        if ((size_t)SL_THREADS * 16 + (size_t)(SL_THREADS / 64) * SL_CAP * 2 + (size_t)q.bpw[l] * R * a.nchunk[l] * 8 > 60000) fits = false;
      }
      if (!fits && R > 16) continue;
      const long cost = ((wgs + slots - 1) / slots) * (R + 2 * HALO);
      if (best < 0 || cost < best) { best = cost; bestR = R; }
    }
    for (int l = l0; l <= l1; l++) q.R[l] = bestR;
  };
  pick(0, 0);
  pick(1, NLEV - 1);
  for (int l = 0; l < NLEV; l++) {
    q.nb[l] = (a.h[l] + q.R[l] - 1) / q.R[l];
    nwg[l] = (int)(((long)S * q.nb[l] + q.bpw[l] - 1) / q.bpw[l]);
    lds[l] = (size_t)SL_THREADS * 16 + (size_t)(SL_THREADS / 64) * SL_CAP * 2 + (size_t)q.bpw[l] * q.R[l] * a.nchunk[l] * 8;
  }
  static const bool dbg = getenv("VSLAM_FE_DEBUG") != nullptr;
  if (dbg) fprintf(stderr, "fe slide: S %d n_cu %d R %d %d %d %d nb %d %d %d %d wgs %d %d %d %d lds %zu %zu %zu %zu\n", S, sys->n_cu, q.R[0], q.R[1], q.R[2], q.R[3],
                   q.nb[0], q.nb[1], q.nb[2], q.nb[3], nwg[0], nwg[1], nwg[2], nwg[3], lds[0], lds[1], lds[2], lds[3]);
  q.wg_first[0] = 0; q.wg_first[1] = 0;
  for (int l = 1; l < NLEV; l++) q.wg_first[l + 1] = q.wg_first[l] + nwg[l];
  size_t lds123 = lds[1]; if (lds[2] > lds123) lds123 = lds[2]; if (lds[3] > lds123) lds123 = lds[3];
  prof_mark(sys, PROF_PYR_FAST0);
  hipLaunchKernelGGL(k_fast_slide<true>, dim3(nwg[0]), dim3(SL_THREADS), lds[0], fs, a, q);
  prof_mark(sys, PROF_FAST_LVL);
  hipLaunchKernelGGL(k_fast_slide<false>, dim3(q.wg_first[NLEV]), dim3(SL_THREADS), lds123, fs, a, q);
}

// The band form, k_pyr_fast0 then k_fast_lvl for S streams: the only statement of their dynamic LDS sizes, which follow the tile of
// k_pyr_fast0 / k_fast_lvl and the layout of fast_band.  marks: the per-frame path's profile marks 0 and 1 (a keyframe upload records none).
// A band is staged at its full width, about 37 B per padded level-0 pixel of width: 64 KiB, the most a kernel gets without asking, is passed
// a little above 1,760 pixels (k_fast_lvl: level-1 widths from 2,033), so wider bands raise the kernel's limit first; 4096 pixels, the widest
// vslam_create accepts, take 151,584 B of the CU's 160 KiB.
#define FE_LDS_MAX (160 * 1024)
static int fe_band_lds(const void* kernel, size_t lds) {
  if (lds > FE_LDS_MAX) { vslam_set_error("front end: a band of %zu B does not fit the %d B of LDS", lds, FE_LDS_MAX); return VSLAM_E_INVALID; }
  if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return VSLAM_OK;
}
static int fe_launch_bands(vslam_system* sys, FeArgs& a, hipStream_t stream, int S, bool marks) {
  const LevelGeom* g = sys->geom;
  const int lp0 = (g[0].w + 15) & ~15, lp1 = (g[1].w + 15) & ~15, lp2 = (g[2].w + 15) & ~15;
  const size_t lds0 = (size_t)(BAND + 2 * HALO) * lp0 + (BAND / 2) * lp1 + (BAND / 4) * lp2 + 16 + (size_t)BAND * g[0].nchunk * 8 + (size_t)FB_ROWS * lp0 * 2 + 16;
  const size_t lds1 = (size_t)(BAND + 2 * HALO) * lp1 + 16 + (size_t)BAND * g[1].nchunk * 8 + (size_t)FB_ROWS * lp1 * 2 + 16;
  int r = fe_band_lds((const void*)k_pyr_fast0, lds0);
  if (!r) r = fe_band_lds((const void*)k_fast_lvl, lds1);
  if (r) return r;
  if (marks) prof_mark(sys, PROF_PYR_FAST0);
  hipLaunchKernelGGL(k_pyr_fast0, dim3((g[0].h + BAND - 1) / BAND, S), dim3(FE_THREADS), lds0, stream, a, lp0, lp1, lp2);
  int nb = 0;
  a.band_first[0] = 0;
  for (int l = 1; l < NLEV; l++) { a.band_first[l] = nb; nb += (g[l].h + BAND - 1) / BAND; }
  if (marks) prof_mark(sys, PROF_FAST_LVL);
  hipLaunchKernelGGL(k_fast_lvl, dim3(nb, S), dim3(FE_THREADS), lds1, stream, a);
  return VSLAM_OK;
}

// A subset step's arguments (vslam_make_keyframe_lite_subset), checked before anything moves: the list, and on systems with the map
// bootstrap the one stream state that cannot be held.  A stream whose trails are running reads the previous frame's level 0 and corner
// list out of the other front-end buffer in place (k_trail_advance), so its frames must be consecutive steps: this is the one place
// where a subset step waits for the device, to read the stages.
static int fe_check_subset(vslam_system* sys, const uint8_t* gray, const int* streams, int n, std::vector<unsigned char>& in_step) {
  if (n < 0 || n > sys->S || (n > 0 && (!streams || !gray))) { vslam_set_error("make_keyframe_lite_subset: bad arguments (n %d of %d streams)", n, sys->S); return VSLAM_E_INVALID; }
  if (sys->frame_open) { vslam_set_error("make_keyframe_lite_subset: the previous frame was not finished (vslam_finish_frame)"); return VSLAM_E_STATE; }
  in_step.assign((size_t)sys->S, 0);
  for (int i = 0; i < n; i++) {
    const int s = streams[i];
    if (s < 0 || s >= sys->S) { vslam_set_error("make_keyframe_lite_subset: stream %d outside the batch of %d", s, sys->S); return VSLAM_E_INVALID; }
    if (in_step[s]) { vslam_set_error("make_keyframe_lite_subset: stream %d listed twice", s); return VSLAM_E_INVALID; }
    in_step[s] = 1;
  }
  if (sys->p.bootstrap && n < sys->S) {
    std::vector<TrackerState> st((size_t)sys->S);
    VCHK(host_get(sys->stream, st.data(), sys->map.st, (size_t)sys->S));
    for (int s = 0; s < sys->S; s++)
      if (!in_step[s] && st[s].init_stage == 1) { vslam_set_error("make_keyframe_lite_subset: stream %d has trails running and cannot be held", s); return VSLAM_E_STATE; }
  }
  return VSLAM_OK;
}

int fe_stream_in_step(vslam_system* sys, int stream, const char* who) {
  if (sys->step_subset && !sys->step_in[(size_t)stream]) { vslam_set_error("%s: stream %d was held in this step, it has no front-end products", who, stream); return VSLAM_E_STATE; }
  return VSLAM_OK;
}

// n < 0: the full step, image s for stream s.  n >= 0: a subset step, image i for streams[i]; every image is copied into its stream's
// owned level-0 slot (from the host or from device memory alike), so the kernels find input and products of an ordinal in the same
// stream's slots and the tracker finds level 0 where it finds it after a host-input full step.
int fe_make_keyframe_lite(vslam_system* sys, const uint8_t* gray, size_t row_stride, size_t stream_stride,
                          int on_device, const int* streams, int n) {
  const LevelGeom* g = sys->geom;
  const bool subset = n >= 0;
  if ((!gray && !(subset && n == 0)) || (gray && (int)row_stride < g[0].w)) { vslam_set_error("make_keyframe_lite: bad image arguments"); return VSLAM_E_INVALID; }
  std::vector<unsigned char> in_step;
  if (subset) { const int r = fe_check_subset(sys, gray, streams, n, in_step); if (r) return r; }
  const int nb = sys->fr_idx ^ 1;
  if (subset && sys->step_stage_used[nb]) HIPCHK(hipEventSynchronize(sys->ev_step_stage[nb]));   // the upload of two steps ago has left the block
  // next front-end buffer; it may be rebuilt once the tracking that last read it (two frames ago) has finished
  const int b = nb;
  sys->fr_idx = b;
  sys->fr = sys->frbuf[b];
  for (int l = 0; l < NLEV; l++) sys->d_lvl[l] = sys->d_lvl_buf[b][l];
  hipStream_t fs = sys->fe_stream;
  HIPCHK(hipStreamWaitEvent(fs, sys->ev_track_done[b], 0));
  // map bootstrap: the trail tracker of the frame in flight (k_trail_advance, boot.hip) still reads THIS buffer as its previous
  // frame (image, corners, row LUT) -- the buffer is free only when that frame has finished too
  if (sys->p.bootstrap) HIPCHK(hipStreamWaitEvent(fs, sys->ev_track_done[b ^ 1], 0));
  FeArgs a;
  fill_fe_args(sys, a);
  const int S = subset ? n : sys->S;                                  // streams the front end works on
  if (subset) {
    const size_t Sz = (size_t)sys->S;
    int* hl = (int*)sys->step_stage[b];
    unsigned char* hm = sys->step_stage[b] + Sz * sizeof(int);
    for (int i = 0; i < sys->S; i++) { hl[i] = i < n ? streams[i] : 0; hm[i] = in_step[(size_t)i] ? 0 : 1; }
    HIPCHK(hipMemcpyAsync(sys->fr.step_list, sys->step_stage[b], Sz * sizeof(int) + Sz, hipMemcpyHostToDevice, fs));
    HIPCHK(hipEventRecord(sys->ev_step_stage[b], fs));
    sys->step_stage_used[b] = true;
    sys->step_in.swap(in_step);
    a.list = sys->fr.step_list;
    sys->fe_held = sys->fr.held; sys->map.held = sys->fr.held;
  } else {
    if (sys->step_subset) sys->step_in.assign((size_t)sys->S, 1);
    sys->fe_held = nullptr; sys->map.held = nullptr;
  }
  sys->step_subset = subset;
  if (on_device && !subset) {
    a.in = gray; a.in_sstride = stream_stride; a.in_pitch = (int)row_stride;
  } else {
    // host input: copy into the owned level-0 image (TrackFrame copies its input too, jni/KeyFrame.cc:12)
    for (int i = 0; i < S && !on_device; i++) {
      const int s = subset ? streams[i] : i;
      HIPCHK(hipMemcpy2DAsync(sys->d_lvl[0] + (size_t)s * a.lvl_sstride[0], g[0].pitch, gray + (size_t)i * stream_stride,
                              row_stride, g[0].w, g[0].h, hipMemcpyHostToDevice, fs));
    }
    if (on_device && S > 0)                                          // a subset step from device memory: the same, in one launch
      hipLaunchKernelGGL(k_gather_level0, dim3((g[0].h + GATHER_ROWS - 1) / GATHER_ROWS, S), dim3(FE_THREADS), 0, fs, gray, stream_stride, (int)row_stride,
                         sys->d_lvl[0], a.lvl_sstride[0], g[0].pitch, g[0].w, g[0].h, (const int*)sys->fr.step_list);
    a.in = sys->d_lvl[0]; a.in_sstride = a.lvl_sstride[0]; a.in_pitch = g[0].pitch;
  }
  sys->fr.img[0] = a.in; sys->fr.img_sstride[0] = a.in_sstride; sys->fr.img_pitch[0] = a.in_pitch;
  for (int l = 1; l < NLEV; l++) { sys->fr.img[l] = a.lvl[l]; sys->fr.img_sstride[l] = a.lvl_sstride[l]; sys->fr.img_pitch[l] = a.lvl_pitch[l]; }
  sys->frbuf[b] = sys->fr;

  if (S > 0) {                                                        // (an empty subset step launches nothing here)
    if (fe_slide_ok(sys, a)) fe_launch_slide(sys, a, fs, S);
    else { const int r = fe_launch_bands(sys, a, fs, S, true); if (r) return r; }
  }
  prof_mark(sys, PROF_COMPACT);
  if (S > 0) {
    const CpArgs cp = fe_compact_args(a);
    hipLaunchKernelGGL(k_compact, fe_compact_grid(cp, S), dim3(COMPACT_THREADS), 0, fs, a, cp);
  }
  if (sys->p.use_sbi) {                                           // jni/Tracker.cc:86-97, 104-105
    const FrameDev& last = sys->have_sbi ? sys->frbuf[b ^ 1] : sys->fr;
    int r = VSLAM_OK;
    if (subset) {
      // a stream whose first frame comes in a subset step, after other streams' frames: its "last frame" is the frame itself
      for (int i = 0; i < n && sys->have_sbi; i++)
        if (!sys->sbi_seen[(size_t)streams[i]]) { HIPCHK(hipMemsetAsync(sys->sbi_restart + streams[i], 1, 1, fs)); sys->sbi_restart_pending = true; }
      for (int i = 0; i < n; i++) sys->sbi_seen[(size_t)streams[i]] = 1;
      if (S > 0) r = fe_sbi(sys, last, a.list, S);
      if (!r && sys->have_sbi && S < sys->S) r = fe_sbi_carry(sys, last);   // the held streams keep their last frame's products in the current buffer
    } else {
      if (!sys->sbi_all_seen) { sys->sbi_seen.assign((size_t)sys->S, 1); sys->sbi_all_seen = true; }
      r = fe_sbi(sys, last, nullptr, S);
    }
    if (r) return r;
    // streams reset since their last frame: a full step serves every flag; a subset step only its own streams' (k_sbi_restart), so the
    // flags of held streams may remain and the launch is repeated until a full step
    if (sys->sbi_restart_pending && S > 0) { r = fe_sbi_restart(sys); if (r) return r; if (!subset) sys->sbi_restart_pending = false; }
    if (S > 0) sys->have_sbi = true;
  }
  prof_mark(sys, PROF_FE_END);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(sys->ev_fe_done[b], fs));
  HIPCHK(hipStreamWaitEvent(sys->stream, sys->ev_fe_done[b], 0));   // everything on the main stream sees the new frame
  sys->have_frame = true;
  return VSLAM_OK;
}

static int fe_nonmax_impl(vslam_system* sys, bool gated) {
  if (!sys->have_frame) { vslam_set_error("fast_nonmax: no current frame"); return VSLAM_E_STATE; }
  NmArgs a;
  int maxcap = 0;
  for (int l = 0; l < NLEV; l++) {
    a.img[l] = sys->fr.img[l]; a.img_sstride[l] = sys->fr.img_sstride[l]; a.img_pitch[l] = sys->fr.img_pitch[l];
    a.h[l] = sys->geom[l].h; a.cap[l] = sys->geom[l].cap;
    a.corners[l] = sys->fr.corners[l]; a.rowlut[l] = sys->fr.rowlut[l];
    a.scores[l] = sys->fr.scores[l]; a.maxcorners[l] = sys->fr.maxcorners[l];
    if (a.cap[l] > maxcap) maxcap = a.cap[l];
  }
  a.ncorners = sys->fr.ncorners; a.nmax = sys->fr.nmax;
  a.barrier = sys->p.nonmax_barrier;
  a.quirk = (sys->p.quirks & VSLAM_Q_NONMAX_RIGHT_NEIGHBOUR) ? 1 : 0;
  a.gate = gated ? sys->map.st : nullptr;
  a.held = sys->fe_held;
  (void)maxcap;
  hipLaunchKernelGGL(k_score, dim3(16, NLEV, sys->S), dim3(FE_THREADS), 0, sys->stream, a);
  hipLaunchKernelGGL(k_nonmax, dim3(NLEV, sys->S), dim3(FE_THREADS), 0, sys->stream, a);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

int fe_fast_nonmax(vslam_system* sys) { return fe_nonmax_impl(sys, false); }

// KeyFrame::MakeKeyFrame_Rest (jni/KeyFrame.cc:53-95) for the current frame of every stream: fast_nonmax + candidates.
static int fe_rest_impl(vslam_system* sys, double min_score, bool gated) {
  int r = fe_nonmax_impl(sys, gated);
  if (r) return r;
  CandArgs a;
  for (int l = 0; l < NLEV; l++) {
    a.img[l] = sys->fr.img[l]; a.img_sstride[l] = sys->fr.img_sstride[l]; a.img_pitch[l] = sys->fr.img_pitch[l];
    a.w[l] = sys->geom[l].w; a.h[l] = sys->geom[l].h; a.cap[l] = sys->geom[l].cap;
    a.maxcorners[l] = sys->fr.maxcorners[l];
    a.cand[l] = sys->cand[l]; a.cand_score[l] = sys->cand_score[l];
  }
  a.nmax = sys->fr.nmax; a.ncand = sys->ncand;
  a.min_score = min_score; a.border = 10;                            // gvdCandidateMinSTScore / border, jni/KeyFrame.cc:57,65
  a.gate = gated ? sys->map.st : nullptr;
  a.held = sys->fe_held;
  hipLaunchKernelGGL(k_candidates, dim3(NLEV, sys->S), dim3(FE_THREADS), 0, sys->stream, a);
  HIPCHK(hipGetLastError());
  sys->have_candidates = true;
  return VSLAM_OK;
}
int fe_make_keyframe_rest(vslam_system* sys, double min_score) { return fe_rest_impl(sys, min_score, false); }
int fe_keyframe_rest_gated(vslam_system* sys) { return fe_rest_impl(sys, 70.0, true); }   // gvdCandidateMinSTScore, jni/KeyFrame.cc:57

int fe_thin_candidates(vslam_system* sys, int keyframe) {
  if (!sys->have_candidates) { vslam_set_error("thin_candidates: call vslam_make_keyframe_rest first"); return VSLAM_E_STATE; }
  if (keyframe >= sys->p.max_keyframes) { vslam_set_error("thin_candidates: bad keyframe"); return VSLAM_E_INVALID; }
  ThinArgs a;
  for (int l = 0; l < NLEV; l++) { a.cand[l] = sys->cand[l]; a.cand_score[l] = sys->cand_score[l]; a.cap[l] = sys->geom[l].cap; }
  a.ncand = sys->ncand;
  const size_t P = sys->p.max_points, K = sys->p.max_keyframes;
  a.new_kf = 0; a.only_level = -1; a.kf_row = 0; a.held = sys->fe_held;
  if (keyframe < 0) { a.meas = sys->map.cur_meas; a.meas_sstride = P; }           // the tracker's measurements of this frame
  else { a.meas = sys->map.kf_meas + (size_t)keyframe * P; a.meas_sstride = K * P; }
  hipLaunchKernelGGL(k_thin_candidates, dim3(NLEV, sys->S), dim3(FE_THREADS), 0, sys->stream, a, sys->map.st);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

// MapMaker::ThinCandidates(new keyframe, level) inside AddSomeMapPoints (jni/MapMaker.cc:432): against the measurement row of
// the slot k_add_keyframe has just filled, which also holds the points the earlier levels of this keyframe have added.
int fe_thin_new_keyframe(vslam_system* sys, int level) {
  ThinArgs a;
  for (int l = 0; l < NLEV; l++) { a.cand[l] = sys->cand[l]; a.cand_score[l] = sys->cand_score[l]; a.cap[l] = sys->geom[l].cap; }
  a.ncand = sys->ncand;
  const size_t P = sys->p.max_points, K = sys->p.max_keyframes;
  a.meas = sys->map.kf_meas; a.meas_sstride = K * P; a.new_kf = 1; a.only_level = level; a.kf_row = P; a.held = sys->fe_held;
  hipLaunchKernelGGL(k_thin_candidates, dim3(1, sys->S), dim3(FE_THREADS), 0, sys->stream, a, sys->map.st);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

// Level::vCorners of a stored keyframe (map upload with grow_map): the front-end kernels on a one-stream view whose level
// images are the keyframe's own storage; the mask / list scratch is the front-end buffer that is not the current frame's.
// Enqueued on the main stream and not waited for: the caller keeps the front-end stream off the scratch -- add_keyframes by the
// wait of its upload batch, vslam_restore_stream by ordering the front-end stream behind the restore.
__global__ void k_store_kf_corners(const uint32_t* c0, const uint32_t* c1, const uint32_t* c2, const uint32_t* c3, const int* ncorners,
                                   uint32_t* d0, uint32_t* d1, uint32_t* d2, uint32_t* d3, int* dn, int k0, int k1, int k2, int k3) {
  const int l = blockIdx.x;
  const uint32_t* src = l == 0 ? c0 : (l == 1 ? c1 : (l == 2 ? c2 : c3));
  uint32_t* dst = l == 0 ? d0 : (l == 1 ? d1 : (l == 2 ? d2 : d3));
  const int kc = l == 0 ? k0 : (l == 1 ? k1 : (l == 2 ? k2 : k3));
  const int n = ncorners[l] < kc ? ncorners[l] : kc;
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x == 0) dn[l] = n;
}

int fe_keyframe_corners(vslam_system* sys, int s, int kf) {
  const LevelGeom* g = sys->geom;
  const FrameDev& scr = sys->frbuf[sys->fr_idx ^ 1];
  const size_t K = sys->p.max_keyframes;
  FeArgs a;
  for (int l = 0; l < NLEV; l++) {
    uint8_t* img = sys->map.kf_img[l] + ((size_t)s * K + kf) * (size_t)g[l].pitch * g[l].h;
    a.lvl[l] = img; a.lvl_sstride[l] = 0; a.lvl_pitch[l] = g[l].pitch;
    a.w[l] = g[l].w; a.h[l] = g[l].h; a.nchunk[l] = g[l].nchunk; a.thr[l] = g[l].thr; a.cap[l] = g[l].cap;
    a.cmask[l] = scr.cmask[l]; a.rowcnt[l] = scr.rowcnt[l]; a.rowlut[l] = scr.rowlut[l]; a.corners[l] = scr.corners[l];
  }
  a.ncorners = scr.ncorners; a.overflow = scr.overflow; a.list = nullptr;
  a.in = a.lvl[0]; a.in_sstride = 0; a.in_pitch = g[0].pitch;
  { const int r = fe_launch_bands(sys, a, sys->stream, 1, false); if (r) return r; }
  const CpArgs cp = fe_compact_args(a);
  hipLaunchKernelGGL(k_compact, fe_compact_grid(cp, 1), dim3(COMPACT_THREADS), 0, sys->stream, a, cp);
  uint32_t* d[NLEV];
  for (int l = 0; l < NLEV; l++) d[l] = sys->map.kf_corners[l] + ((size_t)s * K + kf) * sys->tp.kcap[l];
  hipLaunchKernelGGL(k_store_kf_corners, dim3(NLEV), dim3(256), 0, sys->stream, scr.corners[0], scr.corners[1], scr.corners[2], scr.corners[3], scr.ncorners,
                     d[0], d[1], d[2], d[3], sys->map.kf_ncorners + ((size_t)s * K + kf) * NLEV, sys->tp.kcap[0], sys->tp.kcap[1], sys->tp.kcap[2], sys->tp.kcap[3]);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}
