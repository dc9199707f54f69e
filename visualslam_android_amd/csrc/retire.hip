// Keyframe retirement: one keyframe of a stream leaves its map, on the device and in place, so that a map at capacity can take the
// next keyframe (vslam_params.keyframe_retire) or a caller can thin a map between frames (vslam_retire_keyframes).  The reference has no
// such operation: its Map grows on the heap (jni/Map.h:21-34) and nothing ever leaves vpKeyFrames.  Like max_points and the snapshots
// this is the build's own.
//
// Retired keyframe r of nk, np points.  A point is dropped when bad || src_kf == r: the template of a point sourced in r can no longer
// be made (the patch finders read kf_img[src_kf]), and a bad point only holds a slot.  Everything indexed by keyframe loses row r and
// the later rows move down one; everything indexed by point is compacted through remap[i] (the new index, -1 for a dropped point);
// keyframes keep their order of creation and points their relative order.  A survivor changes in two fields only: src_kf > r is
// decremented, n_meas_kfs is decremented where row r measured the point.  What a read-back can reach above the new counts is zero
// afterwards (the tail a compaction leaves, the vacated last keyframe row), as reset.hip keeps it.
//
// Three launches, each stream by its own workgroups:
//   k_retire_plan     one workgroup per stream.  The gate; the policy (the keyframe farthest from pose_final, KeyFrameLinearDist, lowest
//                     index on ties); remap by ballot and prefix (k_ba_assemble's pattern); the survivors' two fields and their
//                     never-retry bits, at their OLD index, before anything moves (row r is read here: "was it valid" needs no copy);
//                     the failure queue and iter_list filtered in place; RelocInfo::best; fixedness; the record; the new counts.
//                     The OLD counts go into the plan record: the two kernels below read r, nk, np from there, never from TrackerState,
//                     so publishing n_kf and n_points here cannot mislead them.
//   k_retire_columns  one workgroup per (stream, row): a row is a per-point array or one keyframe's row of kf_meas.  It walks the row in
//                     ascending tiles: a tile is loaded into registers, a barrier, then its survivors are stored.  remap[i] <= i, so a
//                     tile's stores end at or before the tile's own end, which has been read; the next tile's loads start there.  Rows are
//                     independent.  Words of 8 bytes (4 for the two int arrays), consecutive lanes on consecutive words.
//   k_retire_shift    a launch of its own, after the compaction: a workgroup that pulled row k + 1 into row k while its neighbour
//                     compacts row k + 1 would race.  Each lane owns fixed byte offsets inside a slot and runs
//                     slot[k][off] = slot[k + 1][off] for k = r .. nk - 2: its own program order is the whole ordering argument, no lane
//                     reads what another writes.  Loads are issued four slots ahead of their stores.  16-byte words where base and slot
//                     stride allow (the pyramids always: the pitch is a multiple of 64), else 8, 4 or single bytes.
// Scratch: remap is [S][max_points] ints, held by the system's DevOwner from creation with keyframe_retire != 0 or from the first
// explicit call; a default system allocates nothing here.
#include "vslam_internal.h"
#include <string.h>

#define RETIRE_THREADS 256
#define RETIRE_WAVES (RETIRE_THREADS / 64)
#define RETIRE_MAX_KF 128        // = BA_MAX_KF (ba_alloc refuses more keyframes)
#define RETIRE_TILE_WORDS 8      // words a lane holds of one tile
#define RETIRE_SHIFT_BLOCKS 32   // workgroups per stream: level 0 of 640 x 480 is 2.3 16-byte words per lane and slot
#define RETIRE_SHIFT_AHEAD 4     // slots whose loads are in flight before the first of their stores (shift_as states them one by one)

// plan record: what the moving kernels need, the old counts among it
enum RetirePlan : int { RP_R = 0 /* -1: nothing to do */, RP_NK, RP_NP, RP_NP_NEW, RP_NCORN /* [NLEV] longest corner list above r */, RETIRE_PLAN_N = RP_NCORN + NLEV };
#define RETIRE_NOT_LISTED (-2)   // request of a stream the explicit call does not name; -1: by policy

static_assert(sizeof(MapPointDev) % 8 == 0 && sizeof(TrackData) % 8 == 0 && TMPL_PITCH % 8 == 0 && sizeof(MeasDev) == 24, "the compaction moves 8-byte words");

struct RetireArgs { int* remap; int* plan; int* info; const int* req; RelocInfo* reloc; };

// rank of this lane's element among the block's `in` elements, and their number (k_ba_assemble's ballot and prefix)
DEVFN int block_rank(bool in, int* ired, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bm = __ballot(in);
  __syncthreads();
  if (lane == 0) ired[wave] = __popcll(bm);
  __syncthreads();
  int off = 0, all = 0;
  for (int w = 0; w < RETIRE_WAVES; w++) { if (w < wave) off += ired[w]; all += ired[w]; }
  total = all;
  return off + __popcll(bm & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(RETIRE_THREADS) void k_retire_plan(MapDev m, TrackParams tp, RetireArgs a) {
  const int s = blockIdx.x;
  TrackerState* st = &m.st[s];
  int* plan = a.plan + (size_t)s * RETIRE_PLAN_N;
  const int K = tp.max_keyframes, P = tp.max_points;
  const int nk = st->n_kf, np = st->n_points;
  __shared__ int ired[RETIRE_WAVES];
  __shared__ int cnt[8 + NLEV];     // dropped as sourced in r, dropped as bad, survivors below newq_head, left the coarse / level-3 segment; [8 + l]: corners
  __shared__ double dist[RETIRE_MAX_KF];
  __shared__ int sh_r;
  // ---- gate (the same in every lane) ----
  bool go = st->map_good && nk >= 3 && nk <= K && nk <= RETIRE_MAX_KF && np >= 0 && np <= P && st->init_stage != 1 && !(tp.ba_delay > 0 && st->ba_countdown > 0);
  int r = -1;
  if (a.req) { r = a.req[s]; go = go && r >= -1 && r < nk; }
  else {
    const bool asked = trk_kf_pending(m.held, s, st) && nk >= K;
    if (asked && !go && threadIdx.x == 0) st->kf_pending = 0;       // no slot is freed, so no keyframe: k_add_keyframe would write slot K, past the stream's tables
    go = go && asked;
  }
  if (!go) { if (threadIdx.x == 0) plan[RP_R] = -1; return; }
  const Pose* kfp = m.kf_pose + (size_t)s * K;
  if (r < 0) {                                                       // policy: the farthest camera centre, lowest index on ties
    if (threadIdx.x < nk) dist[threadIdx.x] = kf_linear_dist(kfp[threadIdx.x], st->pose_final);
    __syncthreads();
    if (threadIdx.x == 0) { int best = 0; for (int k = 1; k < nk; k++) if (dist[k] > dist[best]) best = k; sh_r = best; }
    __syncthreads();
    r = sh_r;
  }
  if (threadIdx.x < 8 + NLEV) cnt[threadIdx.x] = 0;
  __syncthreads();
  // ---- remap; the survivors' own fields at their old index ----
  int* remap = a.remap + (size_t)s * P;
  MapPointDev* pts = m.pts + (size_t)s * P;
  const MeasDev* row_r = m.kf_meas + ((size_t)s * K + r) * P;
  unsigned long long* nr = m.never_retry ? m.never_retry + (size_t)s * P * 2 : nullptr;
  const int head = st->newq_head;
  int base = 0, c_src = 0, c_bad = 0, c_below = 0;
  for (int i0 = 0; i0 < np; i0 += RETIRE_THREADS) {
    const int i = i0 + threadIdx.x;
    bool keep = false;
    int src = 0;
    if (i < np) {
      src = pts[i].src_kf;
      const bool bad = pts[i].bad != 0;
      keep = src != r && !bad;
      if (src == r) c_src++; else if (bad) c_bad++;
    }
    int total;
    const int id = base + block_rank(keep, ired, total);
    if (i < np) remap[i] = keep ? id : -1;
    if (keep) {
      if (src > r) pts[i].src_kf = src - 1;
      if (row_r[i].valid) pts[i].n_meas_kfs--;
      if (nr) {                                                      // bit r leaves the set, the bits above it move down one across both words
        const unsigned long long w0 = nr[2 * (size_t)i], w1 = nr[2 * (size_t)i + 1];
        if (r < 64) {
          const unsigned long long low = (1ull << r) - 1ull;
          nr[2 * (size_t)i] = (w0 & low) | ((w0 >> 1) & ~low) | (w1 << 63);
          nr[2 * (size_t)i + 1] = w1 >> 1;
        } else {
          const unsigned long long low = (1ull << (r - 64)) - 1ull;
          nr[2 * (size_t)i + 1] = (w1 & low) | ((w1 >> 1) & ~low);
        }
      }
      if (i < head) c_below++;
    }
    base += total;
  }
  const int np_new = base;
  atomicAdd(&cnt[0], c_src); atomicAdd(&cnt[1], c_bad); atomicAdd(&cnt[2], c_below);
  __syncthreads();                                                   // remap is complete and visible to the workgroup
  // ---- failure queue: entries of keyframe r or of a dropped point go, the rest are renumbered; compacted in place, tile by tile
  // (a tile is in registers before the barrier inside block_rank, its stores land at or below its own start) ----
  int fq_kept = 0, fq_stored = 0;
  if (m.fq) {
    int2* fq = m.fq + (size_t)s * tp.fq_cap;
    fq_stored = st->fq_n < 0 ? 0 : (st->fq_n < tp.fq_cap ? st->fq_n : tp.fq_cap);
    for (int e0 = 0; e0 < fq_stored; e0 += RETIRE_THREADS) {
      const int e = e0 + threadIdx.x;
      int2 v = make_int2(0, 0);
      bool keep = false;
      if (e < fq_stored) {
        v = fq[e];
        keep = v.x != r && v.y >= 0 && v.y < np && remap[v.y] >= 0;
        if (keep) { if (v.x > r) v.x--; v.y = remap[v.y]; }
      }
      int total;
      const int id = fq_kept + block_rank(keep, ired, total);
      if (keep) fq[id] = v;
      fq_kept += total;
    }
  }
  // ---- iter_list: dropped points leave, order kept; what left the coarse and the level-3 segment is counted ----
  int* il = m.iter_list + (size_t)s * P;
  const int n_it = st->n_iter < 0 ? 0 : (st->n_iter < P ? st->n_iter : P);
  const int seg_c = st->n_coarse < 0 ? 0 : (st->n_coarse < n_it ? st->n_coarse : n_it);
  const int seg_l = seg_c + (st->n_l3 < 0 ? 0 : (st->n_l3 < n_it - seg_c ? st->n_l3 : n_it - seg_c));
  int it_kept = 0, d_c = 0, d_l = 0;
  for (int e0 = 0; e0 < n_it; e0 += RETIRE_THREADS) {
    const int e = e0 + threadIdx.x;
    int v = -1;
    bool keep = false;
    if (e < n_it) {
      v = il[e];
      keep = v >= 0 && v < np && remap[v] >= 0;
      if (keep) v = remap[v]; else if (e < seg_c) d_c++; else if (e < seg_l) d_l++;
    }
    int total;
    const int id = it_kept + block_rank(keep, ired, total);
    if (keep) il[id] = v;
    it_kept += total;
  }
  atomicAdd(&cnt[3], d_c); atomicAdd(&cnt[4], d_l);
  // ---- the longest stored corner list above r, per level: what the shift has to move of a slot ----
  if (m.kf_ncorners) {
    const int k = r + 1 + (int)threadIdx.x / NLEV, l = threadIdx.x % NLEV;
    for (int kk = k; kk < nk; kk += RETIRE_THREADS / NLEV) {
      int n = m.kf_ncorners[((size_t)s * K + kk) * NLEV + l];
      n = n < 0 ? 0 : (n < tp.kcap[l] ? n : tp.kcap[l]);
      atomicMax(&cnt[8 + l], n);
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (a.reloc) { RelocInfo* ri = a.reloc + s; if (ri->best == r) ri->best = -1; else if (ri->best > r) ri->best--; }
  {                                                                  // the gauge: a map whose only fixed keyframe leaves fixes its oldest survivor
    int* kff = m.kf_fixed + (size_t)s * K;
    if (kff[r]) {
      bool any = false;
      for (int k = 0; k < nk; k++) if (k != r && kff[k]) any = true;
      if (!any) kff[r == 0 ? 1 : 0] = 1;                            // (at its old index: the shift moves it)
    }
  }
  int* o = a.info + 6 * (size_t)s;
  o[0]++; o[1] = r; o[2] = cnt[0]; o[3] = cnt[1]; o[4] = fq_stored - fq_kept; o[5] = st->frame;
  plan[RP_R] = r; plan[RP_NK] = nk; plan[RP_NP] = np; plan[RP_NP_NEW] = np_new;
  for (int l = 0; l < NLEV; l++) plan[RP_NCORN + l] = cnt[8 + l];
  st->n_kf = nk - 1; st->n_points = np_new; st->newq_head = cnt[2];
  if (m.fq) st->fq_n = fq_kept;
  st->n_iter -= n_it - it_kept; st->n_coarse -= cnt[3]; st->n_l3 -= cnt[4];
}

// one row of per-point elements of `wpe` words each, compacted in place through remap; the tail the compaction leaves is zeroed
template <class W>
DEVFN void compact_row(W* base, int wpe, const int* remap, int np_old, int np_new) {
  const int ept = RETIRE_THREADS * RETIRE_TILE_WORDS / wpe;          // elements of a tile (wpe <= 21)
  for (int e0 = 0; e0 < np_old; e0 += ept) {
    const int ne = np_old - e0 < ept ? np_old - e0 : ept, nw = ne * wpe;
    W v[RETIRE_TILE_WORDS];
    long dst[RETIRE_TILE_WORDS];
    W* src = base + (size_t)e0 * wpe;
#pragma unroll
    for (int q = 0; q < RETIRE_TILE_WORDS; q++) {
      const int j = q * RETIRE_THREADS + threadIdx.x;
      dst[q] = -1;
      if (j < nw) {
        const int e = j / wpe, w = j - e * wpe;
        v[q] = src[j];
        const int d = remap[e0 + e];
        if (d >= 0) dst[q] = (long)d * wpe + w;
      }
    }
    __syncthreads();                                                 // the tile is in registers: its stores may land anywhere up to its end
#pragma unroll
    for (int q = 0; q < RETIRE_TILE_WORDS; q++) if (dst[q] >= 0) base[dst[q]] = v[q];
  }
  const W zero{};
  for (long j = (long)np_new * wpe + threadIdx.x; j < (long)np_old * wpe; j += RETIRE_THREADS) base[j] = zero;
}

enum RetireRow : int { RR_PTS = 0, RR_TD, RR_TMPL, RR_CUR_MEAS, RR_NEVER_RETRY, RR_PT_FLAGS, RR_PT_LEVEL, RR_KF_MEAS /* + keyframe */ };

// blockIdx.x = row, blockIdx.y = stream
__global__ __launch_bounds__(RETIRE_THREADS) void k_retire_columns(MapDev m, TrackParams tp, RetireArgs a) {
  const int s = blockIdx.y, row = blockIdx.x;
  const int* plan = a.plan + (size_t)s * RETIRE_PLAN_N;
  if (plan[RP_R] < 0) return;
  const int nk = plan[RP_NK], np = plan[RP_NP], np_new = plan[RP_NP_NEW];
  const size_t P = tp.max_points, K = tp.max_keyframes;
  const int* remap = a.remap + (size_t)s * P;
  typedef unsigned long long W8;
  switch (row) {
    case RR_PTS: compact_row((W8*)(m.pts + (size_t)s * P), (int)(sizeof(MapPointDev) / 8), remap, np, np_new); break;
    case RR_TD: compact_row((W8*)(m.td + (size_t)s * P), (int)(sizeof(TrackData) / 8), remap, np, np_new); break;
    case RR_TMPL: compact_row((W8*)(m.tmpl + (size_t)s * P * TMPL_PITCH), TMPL_PITCH / 8, remap, np, np_new); break;
    case RR_CUR_MEAS: compact_row((W8*)(m.cur_meas + (size_t)s * P), (int)(sizeof(MeasDev) / 8), remap, np, np_new); break;
    case RR_NEVER_RETRY: if (m.never_retry) compact_row((W8*)(m.never_retry + (size_t)s * P * 2), 2, remap, np, np_new); break;
    case RR_PT_FLAGS: compact_row((unsigned*)(m.pt_flags + (size_t)s * P), 1, remap, np, np_new); break;
    case RR_PT_LEVEL: compact_row((unsigned*)(m.pt_level + (size_t)s * P), 1, remap, np, np_new); break;
    default: {
      const int k = row - RR_KF_MEAS;                                // row r is compacted too: its tail has to be zero when the shift fills it
      if (k < nk) compact_row((W8*)(m.kf_meas + ((size_t)s * K + k) * P), (int)(sizeof(MeasDev) / 8), remap, np, np_new);
    }
  }
}

// slot[k][o] = slot[k + 1][o] for k = r .. nk - 2, every lane on its own words o of V; then the vacated last slot is zeroed where asked
template <class V>
DEVFN void shift_as(uint8_t* base, size_t stride, size_t n_words, int r, int nk, bool zero_last, size_t tid, size_t nth) {
  for (size_t o = tid; o < n_words; o += nth) {
    uint8_t* p = base + (size_t)r * stride + o * sizeof(V);
    int k = r;
    for (; k + RETIRE_SHIFT_AHEAD <= nk - 1; k += RETIRE_SHIFT_AHEAD) {
      const V v0 = *(const V*)(p + stride), v1 = *(const V*)(p + 2 * stride), v2 = *(const V*)(p + 3 * stride), v3 = *(const V*)(p + 4 * stride);
      *(V*)p = v0; *(V*)(p + stride) = v1; *(V*)(p + 2 * stride) = v2; *(V*)(p + 3 * stride) = v3;
      p += (size_t)RETIRE_SHIFT_AHEAD * stride;
    }
    for (; k < nk - 1; k++) { const V v = *(const V*)(p + stride); *(V*)p = v; p += stride; }
    if (zero_last) *(V*)p = V{};
  }
}
// ... in the widest words base and stride allow, the bytes behind the last whole word singly
DEVFN void shift_slots(void* base_, size_t stride, size_t bytes, int r, int nk, bool zero_last, size_t tid, size_t nth) {
  uint8_t* base = (uint8_t*)base_;
  const uintptr_t al = (uintptr_t)base | (uintptr_t)stride;
  size_t done = 0;
  if ((al & 15) == 0) { shift_as<uint4>(base, stride, bytes / 16, r, nk, zero_last, tid, nth); done = bytes & ~(size_t)15; }
  else if ((al & 7) == 0) { shift_as<uint2>(base, stride, bytes / 8, r, nk, zero_last, tid, nth); done = bytes & ~(size_t)7; }
  else if ((al & 3) == 0) { shift_as<uint32_t>(base, stride, bytes / 4, r, nk, zero_last, tid, nth); done = bytes & ~(size_t)3; }
  if (done < bytes) shift_as<uint8_t>(base + done, stride, bytes - done, r, nk, zero_last, tid, nth);
}

struct RetireShiftArgs { size_t img_stride[NLEV]; size_t small_pixels; };

// blockIdx.y = stream; its RETIRE_SHIFT_BLOCKS workgroups share every array (as k_reset_clear's do)
__global__ __launch_bounds__(RETIRE_THREADS) void k_retire_shift(MapDev m, TrackParams tp, RetireArgs a, RelocDev reloc, RetireShiftArgs g) {
  const int s = blockIdx.y;
  const int* plan = a.plan + (size_t)s * RETIRE_PLAN_N;
  const int r = plan[RP_R];
  if (r < 0) return;
  const int nk = plan[RP_NK], np_new = plan[RP_NP_NEW];
  const size_t P = tp.max_points, K = tp.max_keyframes;
  const size_t tid = (size_t)blockIdx.x * RETIRE_THREADS + threadIdx.x, nth = (size_t)gridDim.x * RETIRE_THREADS;
  for (int l = 0; l < NLEV; l++) shift_slots(m.kf_img[l] + (size_t)s * K * g.img_stride[l], g.img_stride[l], g.img_stride[l], r, nk, false, tid, nth);
  shift_slots(m.kf_meas + (size_t)s * K * P, P * sizeof(MeasDev), (size_t)np_new * sizeof(MeasDev), r, nk, true, tid, nth);
  shift_slots(m.kf_pose + (size_t)s * K, sizeof(Pose), sizeof(Pose), r, nk, true, tid, nth);
  shift_slots(m.kf_fixed + (size_t)s * K, sizeof(int), sizeof(int), r, nk, true, tid, nth);
  shift_slots(m.kf_depth + (size_t)s * K * 2, 2 * sizeof(double), 2 * sizeof(double), r, nk, true, tid, nth);
  if (m.kf_ncorners) {
    for (int l = 0; l < NLEV; l++)
      shift_slots(m.kf_corners[l] + (size_t)s * K * tp.kcap[l], (size_t)tp.kcap[l] * sizeof(uint32_t), (size_t)plan[RP_NCORN + l] * sizeof(uint32_t), r, nk, false, tid, nth);
    shift_slots(m.kf_ncorners + (size_t)s * K * NLEV, NLEV * sizeof(int), NLEV * sizeof(int), r, nk, true, tid, nth);
  }
  if (reloc.kf_tmpl) {
    const size_t N = g.small_pixels;
    shift_slots(reloc.kf_tmpl + (size_t)s * K * N, N * sizeof(float), N * sizeof(float), r, nk, false, tid, nth);
    shift_slots(reloc.kf_jacs + (size_t)s * K * N * 2, N * 2 * sizeof(float), N * 2 * sizeof(float), r, nk, false, tid, nth);
    shift_slots(reloc.scores + (size_t)s * K, sizeof(double), sizeof(double), r, nk, false, tid, nth);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
int retire_alloc(vslam_system* sys) {
  if (sys->retire_remap) return VSLAM_OK;
  DevOwner& own = sys->own;
  const size_t S = (size_t)sys->S;
  VCHK(own.alloc(&sys->retire_plan, S * RETIRE_PLAN_N, sys->stream));
  VCHK(own.alloc(&sys->retire_req, S, sys->stream));
  VCHK(own.alloc(&sys->retire_info, S * 6, sys->stream));
  { void* pin = nullptr; VCHK(own.pinned(&pin, S * sizeof(int))); sys->retire_req_stage = (int*)pin; }
  for (int k = 0; k < 2; k++) VCHK(own.event(&sys->ev_retire_t[k], true));
  VCHK(own.alloc(&sys->retire_remap, S * (size_t)sys->p.max_points, sys->stream));   // last: the sign that the scratch is whole
  return VSLAM_OK;
}

// the three launches for every stream the plan kernel's gate lets through: the request array's streams, or (req == null) the full streams
// whose tracker has asked for a keyframe in this step
static int retire_launch(vslam_system* sys, const int* req) {
  RetireArgs a = {sys->retire_remap, sys->retire_plan, sys->retire_info, req, sys->reloc.info};
  RetireShiftArgs g;
  for (int l = 0; l < NLEV; l++) g.img_stride[l] = (size_t)sys->geom[l].pitch * sys->geom[l].h;
  g.small_pixels = (size_t)(sys->geom[3].w / 2) * (sys->geom[3].h / 2);
  hipLaunchKernelGGL(k_retire_plan, dim3(sys->S), dim3(RETIRE_THREADS), 0, sys->stream, sys->map, sys->tp, a);
  hipLaunchKernelGGL(k_retire_columns, dim3(RR_KF_MEAS + sys->p.max_keyframes, sys->S), dim3(RETIRE_THREADS), 0, sys->stream, sys->map, sys->tp, a);
  hipLaunchKernelGGL(k_retire_shift, dim3(RETIRE_SHIFT_BLOCKS, sys->S), dim3(RETIRE_THREADS), 0, sys->stream, sys->map, sys->tp, a, sys->reloc, g);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

int retire_on_keyframe(vslam_system* sys) {
  if (!sys->tp.keyframe_retire) return VSLAM_OK;
  return retire_launch(sys, nullptr);
}

extern "C" int vslam_retire_keyframes(vslam_system* sys, const int* streams, const int* keyframes, int n) {
  if (!sys || n < 0 || (n > 0 && (!streams || !keyframes))) { vslam_set_error("retire_keyframes: bad argument"); return VSLAM_E_INVALID; }
  if (sys->frame_open) { vslam_set_error("retire_keyframes: a frame is open (vslam_finish_frame first)"); return VSLAM_E_STATE; }
  std::vector<unsigned char> seen((size_t)sys->S, 0);
  for (int i = 0; i < n; i++) {
    if (streams[i] < 0 || streams[i] >= sys->S) { vslam_set_error("retire_keyframes: stream %d of %d (entry %d); nothing was retired", streams[i], sys->S, i); return VSLAM_E_INVALID; }
    if (seen[(size_t)streams[i]]) { vslam_set_error("retire_keyframes: stream %d is listed twice; nothing was retired", streams[i]); return VSLAM_E_INVALID; }
    seen[(size_t)streams[i]] = 1;
  }
  if (n == 0) return VSLAM_OK;
  VCHK(retire_alloc(sys));
  // One wait: the request goes up and the listed streams' states come down in one batch; everything is decided before anything is
  // launched.  (The wait also means the previous call's copy out of the pinned request has long finished.)
  int* req = sys->retire_req_stage;
  for (int s = 0; s < sys->S; s++) req[s] = RETIRE_NOT_LISTED;
  for (int i = 0; i < n; i++) req[streams[i]] = keyframes[i] < 0 ? -1 : keyframes[i];
  std::vector<TrackerState> st((size_t)n);
  {
    HostCopy c(sys->stream);
    VCHK(c.put(sys->retire_req, req, (size_t)sys->S));
    for (int i = 0; i < n; i++) VCHK(c.get(&st[(size_t)i], sys->map.st + streams[i]));
    VCHK(c.wait());
  }
  for (int i = 0; i < n; i++) {
    const TrackerState& t = st[(size_t)i];
    const char* why = !t.map_good ? "has no good map" : t.n_kf < 3 ? "has fewer than 3 keyframes (a map keeps at least two)" : t.init_stage == 1 ? "has its trails running"
                    : (sys->tp.ba_delay > 0 && t.ba_countdown > 0) ? "has an adjustment pending" : nullptr;
    if (why) { vslam_set_error("retire_keyframes: stream %d %s; nothing was retired", streams[i], why); return VSLAM_E_STATE; }
    if (keyframes[i] >= t.n_kf) { vslam_set_error("retire_keyframes: keyframe %d of %d (stream %d); nothing was retired", keyframes[i], t.n_kf, streams[i]); return VSLAM_E_INVALID; }
    if (t.n_kf > sys->p.max_keyframes || t.n_points < 0 || t.n_points > sys->p.max_points) { vslam_set_error("retire_keyframes: stream %d holds counts beyond the system's capacities", streams[i]); return VSLAM_E_STATE; }
  }
  HIPCHK(hipEventRecord(sys->ev_retire_t[0], sys->stream));
  VCHK(retire_launch(sys, sys->retire_req));
  VCHK(overlay_forget_listed(sys, sys->retire_req, RETIRE_NOT_LISTED));   // the listed streams draw no discs until TrackMap has run again
  HIPCHK(hipEventRecord(sys->ev_retire_t[1], sys->stream));
  sys->retire_calls++;
  return VSLAM_OK;
}

extern "C" int vslam_get_retire_info(vslam_system* sys, int stream, int out[6]) {
  if (!sys || stream < 0 || stream >= sys->S || !out) { vslam_set_error("get_retire_info: bad argument"); return VSLAM_E_INVALID; }
  if (!sys->retire_info) { for (int k = 0; k < 6; k++) out[k] = 0; return VSLAM_OK; }   // nothing has ever been retired here
  return host_get(sys->stream, out, sys->retire_info + 6 * (size_t)stream, 6);
}

extern "C" int vslam_get_retire_timing(vslam_system* sys, double* ms) {
  if (!sys || !ms) { vslam_set_error("get_retire_timing: bad argument"); return VSLAM_E_INVALID; }
  if (sys->retire_calls == 0) { vslam_set_error("get_retire_timing: no vslam_retire_keyframes call that retired yet"); return VSLAM_E_STATE; }
  HIPCHK(hipEventSynchronize(sys->ev_retire_t[1]));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, sys->ev_retire_t[0], sys->ev_retire_t[1]));
  *ms = t;
  return VSLAM_OK;
}
