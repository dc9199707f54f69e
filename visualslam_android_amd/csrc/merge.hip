// Map merge: the map of one stream of a live batch is appended to the map of another, on the device and in place, for any number of
// pairs in one call between two frames (vslam_merge_maps).  Two cameras that mapped two parts of a site, or a stream that was reset and
// bootstrapped again beside the snapshot of its old map, become one map that the destination's tracker and map-maker work on.  The
// reference has no such operation: its Map is a single heap object (jni/Map.h:21-34).  Like retirement and max_points this is the
// build's own, and opt-in by being called: a system that never calls it allocates nothing here and launches nothing.  The C++ mirror
// (include/vslam/ptam.h) gains nothing: its MapMaker is one stream.
//
// What it is not.  Points that both maps hold of one surface feature are two points afterwards; vslam_fuse_points (fuse.hip) makes them
// one once they have been measured at the same corners.  No registration: bringing both
// maps into one frame and one scale first is the caller's job (vslam_fit_similarity + vslam_transform_maps), and nothing here can check
// it.  The two parts become one adjustable map through what exists: keyframes added afterwards measure points of both parts, and
// TrackerState::newq_head stays where it was, so every appended point is in mqNewQueue and, with idle jobs, ReFindNewlyMade looks for
// it in the destination's keyframes.
//
// Destination d (nk_d keyframes, np_d points), source s (nk_s, np_s); the index rules are csrc/merge_dev.h.  s is only read and keeps
// every bit.  Nothing of d below its old counts changes except the scalars named last.
//   pts[np_d + p]                s's MapPointDev with src_kf + nk_d (bad points come along: a later retirement reclaims them)
//   td, tmpl [np_d + p]          s's, bit for bit: the cached template, last_warp, tsum and tsumsq stay consistent, the template's source
//                                image comes along below
//   pt_flags[np_d + p]           s's & (TDF_TMPL_BAD | TDF_HAVE_LAST);  pt_level[np_d + p] = -1 (not in d's PVS, as the map upload leaves it)
//   cur_meas[np_d + p]           zero
//   kf_meas[nk_d + k][np_d + p]  s's kf_meas[k][p]; the cross blocks (d's rows x new columns, new rows x d's columns) are WRITTEN zero.
//                                Reset and retirement keep the table zero above the counts, so they are zero already but for one case:
//                                the slot at n_kf may hold the row of a keyframe that never joined the map (reset.hip clears it for
//                                that reason).  Writing 24 bytes per cell of the two blocks costs little beside the images and makes
//                                the result independent of the invariant; the invariant holds afterwards either way.
//   kf_pose, kf_depth, kf_img[0..3], kf_corners[0..3] + kf_ncorners, RelocDev::kf_tmpl, kf_jacs   slot nk_d + k = s's slot k, whole slots
//   kf_fixed[nk_d + k] = 0       d's fixed keyframe stays the only gauge of BundleAdjustAll; two would pin the parts against each other
//   RelocDev::scores[nk_d + k] = 0   the keyframe was not in d's last attempt; RelocInfo is untouched, so `best` stays valid
//   never_retry[np_d + p]        s's set masked to nk_s bits, shifted up by nk_d (d's own sets stay: the new keyframes may be tried)
//   failure queue                s's stored entries renumbered behind d's stored ones; fq_n = stored_d + stored_s
//   TrackerState                 n_kf, n_points: the sums; ba_converged_recent = ba_converged_full = 0 as AddKeyFrameFromTopOfQueue sets
//                                them (ba.hip, k_add_keyframe); newq_head and every other byte stay
//   untouched                    iter_list and the per-frame lists, the last frame's SmallBlurryImage, trails, the transform and retire
//                                records, the overlay's record (d's indices did not move and the appended points carry no FOUND bit)
//
// Two launches.  The host reads the 2n states in the one batch that uploads the request and refuses there; the counts are known only
// after that wait, and a second upload would be a second wait (the host-copy rule).  So only (d, s) go up, and
//   k_merge_plan   one lane per pair completes the plan record from the two states on the device -- the states the host has judged:
//                  nothing runs on the stream in between -- and repeats the capacity check as a guard for the movers' bounds;
//   k_merge        blockIdx.y = pair, blockIdx.x = job: a block of 256 source points across the per-point arrays; a row of d's
//                  measurement table; a share of the keyframe slots; the queue with the commit.  The movers read counts from the plan
//                  only, never from TrackerState, so the one lane that publishes n_kf and n_points in the same launch cannot mislead
//                  them (the hazard retire.hip names does not arise, and no third launch is needed).
// Ordering: s is only read; d is written only at indices at or above its old counts, plus the scalars; within a pair every lane
// writes words that no lane reads (the sources are s's, or constants); streams are distinct across pairs.  Nothing orders the launch
// internally, and nothing has to.
// Source slots [0, nk_s) are contiguous, so each per-keyframe array is one copy of nk_s x slot bytes: 16-byte words where both
// addresses allow (the pyramids always: the pitch is a multiple of 64), else 8, 4 or single bytes (measurement rows at odd
// max_points or odd np_d, relocaliser images at odd (w/16)(h/16), corner lists); consecutive lanes on consecutive words, four loads in
// flight per lane, stated as four scalars (an array cost retirement 80 bytes of scratch per lane).
#include "vslam_internal.h"
#include "merge_dev.h"
#include <string.h>

#define MERGE_THREADS 256
#define MERGE_SLOT_BLOCKS 32     // workgroups per pair that share the keyframe slots: four keyframes of 640 x 480 are 12.6 16-byte words per lane

// plan record of a pair: the request (the host uploads MP_D and MP_S), then what k_merge_plan reads from the states
enum MergePlan : int { MP_D = 0, MP_S, MP_GO, MP_NK_D, MP_NP_D, MP_NK_S, MP_NP_S, MP_STORED_D, MP_STORED_S, MP_FRAME, MERGE_PLAN_N = 12 };

static_assert(MERGE_KEEP_FLAGS == (TDF_TMPL_BAD | TDF_HAVE_LAST), "merge_dev.h states the flags an appended point keeps");
static_assert(sizeof(MapPointDev) == 104 && offsetof(MapPointDev, src_kf) == 72 && sizeof(TrackData) % 8 == 0 && TMPL_PITCH % 8 == 0 && sizeof(MeasDev) == 24,
              "the per-point movers copy 8-byte words; src_kf is the low half of word 9 of 13");

struct MergeArgs { int* plan; int* info; size_t img_stride[NLEV]; size_t small_pixels; int point_blocks; };

__global__ void k_merge_plan(MapDev m, TrackParams tp, int* plan_all, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int* plan = plan_all + (size_t)i * MERGE_PLAN_N;
  const TrackerState* d = &m.st[plan[MP_D]];
  const TrackerState* s = &m.st[plan[MP_S]];
  const int nk_d = d->n_kf, np_d = d->n_points, nk_s = s->n_kf, np_s = s->n_points;
  plan[MP_NK_D] = nk_d; plan[MP_NP_D] = np_d; plan[MP_NK_S] = nk_s; plan[MP_NP_S] = np_s;
  plan[MP_STORED_D] = m.fq ? merge_queue_stored(d->fq_n, tp.fq_cap) : 0;
  plan[MP_STORED_S] = m.fq ? merge_queue_stored(s->fq_n, tp.fq_cap) : 0;
  plan[MP_FRAME] = d->frame;
  plan[MP_GO] = nk_d >= 0 && nk_s >= 0 && np_d >= 0 && np_s >= 0 && nk_d + nk_s <= tp.max_keyframes && nk_d + nk_s <= MERGE_SET_BITS && np_d + np_s <= tp.max_points;
}

// n bytes, d and s aligned alike to V: consecutive lanes on consecutive words, four loads in flight before their stores
template <class V>
DEVFN void copy_as(uint8_t* d, const uint8_t* s, size_t n_words, size_t tid, size_t nth) {
  V* dv = (V*)d; const V* sv = (const V*)s;
  size_t i = tid;
  for (; i + 3 * nth < n_words; i += 4 * nth) {
    const V v0 = sv[i], v1 = sv[i + nth], v2 = sv[i + 2 * nth], v3 = sv[i + 3 * nth];
    dv[i] = v0; dv[i + nth] = v1; dv[i + 2 * nth] = v2; dv[i + 3 * nth] = v3;
  }
  for (; i < n_words; i += nth) dv[i] = sv[i];
}
// ... in the widest words both addresses allow, the bytes behind the last whole word singly
DEVFN void copy_bytes(void* d_, const void* s_, size_t bytes, size_t tid, size_t nth) {
  uint8_t* d = (uint8_t*)d_; const uint8_t* s = (const uint8_t*)s_;
  const uintptr_t al = (uintptr_t)d | (uintptr_t)s;
  size_t done = 0;
  if ((al & 15) == 0) { copy_as<uint4>(d, s, bytes / 16, tid, nth); done = bytes & ~(size_t)15; }
  else if ((al & 7) == 0) { copy_as<uint2>(d, s, bytes / 8, tid, nth); done = bytes & ~(size_t)7; }
  else if ((al & 3) == 0) { copy_as<uint32_t>(d, s, bytes / 4, tid, nth); done = bytes & ~(size_t)3; }
  if (done < bytes) copy_as<uint8_t>(d + done, s + done, bytes - done, tid, nth);
}
// n 8-byte words of zero
DEVFN void zero_words(void* d, size_t n_words, size_t tid, size_t nth) {
  unsigned long long* q = (unsigned long long*)d;
  for (size_t i = tid; i < n_words; i += nth) q[i] = 0ull;
}

// source points [p0, p0 + cnt) across the per-point arrays, by one workgroup
DEVFN void merge_points(const MapDev& m, size_t P, int d, int s, int nk_d, int np_d, int nk_s, int p0, int cnt) {
  typedef unsigned long long W8;
  const size_t so = (size_t)s * P + p0, dO = (size_t)d * P + merge_point(p0, np_d);
  const int t = threadIdx.x;
  {                                                                  // MapPointDev: word 9 of 13 holds src_kf in its low half
    const int wpe = (int)(sizeof(MapPointDev) / 8);
    const W8* sp = (const W8*)(m.pts + so); W8* dp = (W8*)(m.pts + dO);
    for (int j = t; j < cnt * wpe; j += MERGE_THREADS) {
      W8 v = sp[j];
      if (j % wpe == 9) v = (v & 0xffffffff00000000ull) | (W8)(unsigned)merge_keyframe((int)(unsigned)v, nk_d);
      dp[j] = v;
    }
  }
  copy_as<W8>((uint8_t*)(m.td + dO), (const uint8_t*)(m.td + so), (size_t)cnt * (sizeof(TrackData) / 8), t, MERGE_THREADS);
  copy_as<W8>(m.tmpl + dO * TMPL_PITCH, m.tmpl + so * TMPL_PITCH, (size_t)cnt * (TMPL_PITCH / 8), t, MERGE_THREADS);
  zero_words(m.cur_meas + dO, (size_t)cnt * (sizeof(MeasDev) / 8), t, MERGE_THREADS);
  if (t < cnt) {
    m.pt_flags[dO + t] = merge_flags(m.pt_flags[so + t]);
    m.pt_level[dO + t] = -1;
    if (m.never_retry) {
      uint64_t o0, o1;
      merge_never_retry(m.never_retry[2 * (so + t)], m.never_retry[2 * (so + t) + 1], nk_s, nk_d, &o0, &o1);
      m.never_retry[2 * (dO + t)] = o0; m.never_retry[2 * (dO + t) + 1] = o1;
    }
  }
}

// blockIdx.y = pair; blockIdx.x = job: [0, point_blocks) blocks of points, then max_keyframes measurement rows of d, then
// MERGE_SLOT_BLOCKS shares of the keyframe slots, then the queue and the commit
__global__ __launch_bounds__(MERGE_THREADS) void k_merge(MapDev m, TrackParams tp, RelocDev reloc, MergeArgs a) {
  const int* plan = a.plan + (size_t)blockIdx.y * MERGE_PLAN_N;
  if (!plan[MP_GO]) return;
  const int d = plan[MP_D], s = plan[MP_S], nk_d = plan[MP_NK_D], np_d = plan[MP_NP_D], nk_s = plan[MP_NK_S], np_s = plan[MP_NP_S];
  const size_t P = tp.max_points, K = tp.max_keyframes;
  int job = blockIdx.x;
  if (job < a.point_blocks) {
    const int p0 = job * MERGE_THREADS;
    if (p0 < np_s) merge_points(m, P, d, s, nk_d, np_d, nk_s, p0, np_s - p0 < MERGE_THREADS ? np_s - p0 : MERGE_THREADS);
    return;
  }
  job -= a.point_blocks;
  if (job < (int)K) {                                                // row `job` of d's table
    MeasDev* row = m.kf_meas + ((size_t)d * K + job) * P;
    if (job < nk_d) zero_words(row + np_d, (size_t)np_s * (sizeof(MeasDev) / 8), threadIdx.x, MERGE_THREADS);
    else if (job < nk_d + nk_s) {
      zero_words(row, (size_t)np_d * (sizeof(MeasDev) / 8), threadIdx.x, MERGE_THREADS);
      copy_bytes(m.kf_meas + ((size_t)d * K) * P + merge_meas_cell(job - nk_d, 0, nk_d, np_d, (int)P), m.kf_meas + ((size_t)s * K + (job - nk_d)) * P,
                 (size_t)np_s * sizeof(MeasDev), threadIdx.x, MERGE_THREADS);
    }
    return;
  }
  job -= (int)K;
  if (job < MERGE_SLOT_BLOCKS) {                                     // source slots [0, nk_s) -> d's slots [nk_d, nk_d + nk_s), each array one span
    const size_t tid = (size_t)job * MERGE_THREADS + threadIdx.x, nth = (size_t)MERGE_SLOT_BLOCKS * MERGE_THREADS;
    const size_t ds = (size_t)d * K + nk_d, ss = (size_t)s * K, n = (size_t)nk_s;
    for (int l = 0; l < NLEV; l++) copy_bytes(m.kf_img[l] + ds * a.img_stride[l], m.kf_img[l] + ss * a.img_stride[l], n * a.img_stride[l], tid, nth);
    copy_bytes(m.kf_pose + ds, m.kf_pose + ss, n * sizeof(Pose), tid, nth);
    copy_bytes(m.kf_depth + ds * 2, m.kf_depth + ss * 2, n * 2 * sizeof(double), tid, nth);
    for (size_t k = tid; k < n; k += nth) m.kf_fixed[ds + k] = 0;
    if (m.kf_ncorners) {
      for (int l = 0; l < NLEV; l++) copy_bytes(m.kf_corners[l] + ds * tp.kcap[l], m.kf_corners[l] + ss * tp.kcap[l], n * tp.kcap[l] * sizeof(uint32_t), tid, nth);
      copy_bytes(m.kf_ncorners + ds * NLEV, m.kf_ncorners + ss * NLEV, n * NLEV * sizeof(int), tid, nth);
    }
    if (reloc.kf_tmpl) {
      const size_t N = a.small_pixels;
      copy_bytes(reloc.kf_tmpl + ds * N, reloc.kf_tmpl + ss * N, n * N * sizeof(float), tid, nth);
      copy_bytes(reloc.kf_jacs + ds * N * 2, reloc.kf_jacs + ss * N * 2, n * N * 2 * sizeof(float), tid, nth);
      for (size_t k = tid; k < n; k += nth) reloc.scores[ds + k] = 0.0;
    }
    return;
  }
  // ---- the failure queue, the record and the commit ----
  const int stored_d = plan[MP_STORED_D], stored_s = plan[MP_STORED_S];
  int appended = 0;
  if (m.fq) {
    const int2* qs = m.fq + (size_t)s * tp.fq_cap; int2* qd = m.fq + (size_t)d * tp.fq_cap;
    for (int j = threadIdx.x; j < stored_s; j += MERGE_THREADS) {
      const int q = merge_queue_slot(stored_d, j, tp.fq_cap);
      if (q < 0) break;
      const int2 e = qs[j];
      int2 o;
      merge_queue_entry(e.x, e.y, nk_d, np_d, &o.x, &o.y);
      qd[q] = o;
    }
    appended = stored_s < tp.fq_cap - stored_d ? stored_s : tp.fq_cap - stored_d;
  }
  if (threadIdx.x != 0) return;
  TrackerState* st = &m.st[d];
  st->n_kf = nk_d + nk_s; st->n_points = np_d + np_s;
  st->ba_converged_recent = 0; st->ba_converged_full = 0;
  if (m.fq) st->fq_n = stored_d + stored_s;
  int* o = a.info + 6 * (size_t)d;
  o[0]++; o[1] = s; o[2] = nk_s; o[3] = np_s; o[4] = appended; o[5] = plan[MP_FRAME];
}

// ---- host side ------------------------------------------------------------------------------------------------------
static int merge_alloc(vslam_system* sys) {
  if (sys->merge_plan) return VSLAM_OK;
  DevOwner& own = sys->own;
  const size_t S = (size_t)sys->S;
  VCHK(own.alloc(&sys->merge_info, S * 6, sys->stream));
  { void* pin = nullptr; VCHK(own.pinned(&pin, S * MERGE_PLAN_N * sizeof(int))); sys->merge_plan_stage = (int*)pin; }
  for (int k = 0; k < 2; k++) VCHK(own.event(&sys->ev_merge_t[k], true));
  VCHK(own.alloc(&sys->merge_plan, S * MERGE_PLAN_N, sys->stream));   // last: the sign that the scratch is whole
  return VSLAM_OK;
}

extern "C" int vslam_merge_maps(vslam_system* sys, const int* dst, const int* src, int n) {
  if (!sys || n < 0 || (n > 0 && (!dst || !src))) { vslam_set_error("merge_maps: bad argument"); return VSLAM_E_INVALID; }
  std::vector<unsigned char> seen((size_t)sys->S, 0);
  for (int i = 0; i < n; i++) {
    const int pair[2] = {dst[i], src[i]};
    for (int q = 0; q < 2; q++) {
      if (pair[q] < 0 || pair[q] >= sys->S) { vslam_set_error("merge_maps: stream %d of %d (pair %d); nothing was merged", pair[q], sys->S, i); return VSLAM_E_INVALID; }
      if (seen[(size_t)pair[q]]) {
        vslam_set_error(dst[i] == src[i] ? "merge_maps: pair %d appends stream %d to itself; nothing was merged" : "merge_maps: pair %d names stream %d a second time; nothing was merged", i, pair[q]);
        return VSLAM_E_INVALID;
      }
      seen[(size_t)pair[q]] = 1;
    }
  }
  if (n == 0) return VSLAM_OK;
  if (sys->frame_open) { vslam_set_error("merge_maps: a frame is open (vslam_finish_frame first); nothing was merged"); return VSLAM_E_STATE; }
  VCHK(merge_alloc(sys));
  // One wait: the request goes up and the 2n states come down in one batch; everything is decided before anything is launched.  (The
  // wait also means the previous call's copy out of the pinned request has long finished.)
  int* req = sys->merge_plan_stage;
  memset(req, 0, (size_t)n * MERGE_PLAN_N * sizeof(int));
  for (int i = 0; i < n; i++) { req[(size_t)i * MERGE_PLAN_N + MP_D] = dst[i]; req[(size_t)i * MERGE_PLAN_N + MP_S] = src[i]; }
  std::vector<TrackerState> st((size_t)2 * n);
  {
    HostCopy c(sys->stream);
    VCHK(c.put(sys->merge_plan, req, (size_t)n * MERGE_PLAN_N));
    for (int i = 0; i < n; i++) { VCHK(c.get(&st[(size_t)2 * i], sys->map.st + dst[i])); VCHK(c.get(&st[(size_t)2 * i + 1], sys->map.st + src[i])); }
    VCHK(c.wait());
  }
  const int K = sys->p.max_keyframes, P = sys->p.max_points;
  for (int i = 0; i < 2 * n; i++) {
    const TrackerState& t = st[(size_t)i];
    const int s = i & 1 ? src[i / 2] : dst[i / 2];
    const char* why = !t.map_good ? "has no good map" : t.init_stage == 1 ? "has its trails running"
                    : (sys->tp.ba_delay > 0 && t.ba_countdown > 0) ? "has an adjustment pending" : nullptr;
    if (why) { vslam_set_error("merge_maps: stream %d (pair %d) %s; nothing was merged", s, i / 2, why); return VSLAM_E_STATE; }
    if (t.n_kf < 0 || t.n_kf > K || t.n_points < 0 || t.n_points > P) { vslam_set_error("merge_maps: stream %d holds counts beyond the system's capacities", s); return VSLAM_E_STATE; }
  }
  for (int i = 0; i < n; i++) {
    const TrackerState& d = st[(size_t)2 * i], & s = st[(size_t)2 * i + 1];
    if (d.n_kf + s.n_kf > K || d.n_kf + s.n_kf > MERGE_SET_BITS) {
      vslam_set_error("merge_maps: pair %d (%d <- %d): %d + %d keyframes, the capacity is %d (vslam_retire_keyframes makes room); nothing was merged",
                      i, dst[i], src[i], d.n_kf, s.n_kf, K < MERGE_SET_BITS ? K : MERGE_SET_BITS);
      return VSLAM_E_CAPACITY;
    }
    if (d.n_points + s.n_points > P) {
      vslam_set_error("merge_maps: pair %d (%d <- %d): %d + %d points, the capacity is %d (vslam_retire_keyframes makes room); nothing was merged",
                      i, dst[i], src[i], d.n_points, s.n_points, P);
      return VSLAM_E_CAPACITY;
    }
  }
  MergeArgs a;
  a.plan = sys->merge_plan; a.info = sys->merge_info;
  for (int l = 0; l < NLEV; l++) a.img_stride[l] = (size_t)sys->geom[l].pitch * sys->geom[l].h;
  a.small_pixels = (size_t)(sys->geom[3].w / 2) * (sys->geom[3].h / 2);
  a.point_blocks = (P + MERGE_THREADS - 1) / MERGE_THREADS;
  HIPCHK(hipEventRecord(sys->ev_merge_t[0], sys->stream));
  hipLaunchKernelGGL(k_merge_plan, dim3((n + 63) / 64), dim3(64), 0, sys->stream, sys->map, sys->tp, sys->merge_plan, n);
  hipLaunchKernelGGL(k_merge, dim3(a.point_blocks + K + MERGE_SLOT_BLOCKS + 1, n), dim3(MERGE_THREADS), 0, sys->stream, sys->map, sys->tp, sys->reloc, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(sys->ev_merge_t[1], sys->stream));
  sys->merge_calls++;
  return VSLAM_OK;
}

extern "C" int vslam_get_merge_info(vslam_system* sys, int stream, int out[6]) {
  if (!sys || stream < 0 || stream >= sys->S || !out) { vslam_set_error("get_merge_info: bad argument"); return VSLAM_E_INVALID; }
  if (!sys->merge_info) { for (int k = 0; k < 6; k++) out[k] = 0; return VSLAM_OK; }   // nothing has ever been merged here
  return host_get(sys->stream, out, sys->merge_info + 6 * (size_t)stream, 6);
}

extern "C" int vslam_get_merge_timing(vslam_system* sys, double* ms) {
  if (!sys || !ms) { vslam_set_error("get_merge_timing: bad argument"); return VSLAM_E_INVALID; }
  if (sys->merge_calls == 0) { vslam_set_error("get_merge_timing: no vslam_merge_maps call that merged yet"); return VSLAM_E_STATE; }
  HIPCHK(hipEventSynchronize(sys->ev_merge_t[1]));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, sys->ev_merge_t[0], sys->ev_merge_t[1]));
  *ms = t;
  return VSLAM_OK;
}
