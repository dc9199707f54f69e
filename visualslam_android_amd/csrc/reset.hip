// Per-stream reset: Tracker::Reset (jni/Tracker.cc:45-70) -> MapMaker::RequestReset / Reset (jni/MapMaker.cc:60-74, 127-136) -> Map::Reset
// (jni/Map.cc:8-14) for any subset of the streams of a live batch.  Afterwards a stream is a stream of a newly created system: every
// read-back and every frame tracked on it after a new map give the bits a new system gives; the other streams are not touched.
//
// What a new system holds zeroed and a later reader may read before anything rewrites it is cleared here, and nothing else:
//   TrackerState                  whole, = tracker_reset_state() (the one statement of Tracker::Reset's and MapMaker::Reset's members; the
//                                 boot seed 1 and the PVS shuffle seed of vslam_params with them)
//   kf_meas [< n_kf][< n_points]  a keyframe the tracker adds writes its row only up to the points of that moment, a point the host
//                                 uploads later relies on zeros above it (24 bytes per cell: only the part that was used)
//   cur_meas [< n_points]         vslam_add_keyframe before the stream's first tracked frame copies it
//   never_retry [< n_points]      bits are only ever set (idle jobs)
//   TrackData, templates, pt_flags, pt_level [< n_points]   vslam_get_templates reads any point below max_points
//   kf_pose, kf_fixed, kf_depth, kf_ncorners [all]          vslam_get_keyframe_pose / _corners read any keyframe below max_keyframes
//   RelocInfo                     attempts, successes, the last attempt (vslam_get_reloc_info, vslam_read_reloc_attempt's guard)
//   the pool record               ba.hip, ba_reset_streams
//   the retire record             vslam_get_retire_info (retire.hip), where the system holds one
//   the merge record              vslam_get_merge_info (merge.hip), where the system holds one
//   the fuse record               vslam_get_fuse_info and vslam_get_fuse_pairs (fuse.hip), where the system holds one
//   the overlay's record          -1, TrackMap has not run (overlay.hip), where the system holds one
//   the transform record          vslam_get_transform_info (transform.hip), kept on the host: no transforms, the identity
// Not cleared, because every reader is bounded by a count that is now zero and the writer that raises the count fills what it exposes:
// MapPointDev (n_points; append_point / vslam_map_add_points), the failure queue (fq_n), keyframe images, corner lists and
// SmallBlurryImages (n_kf; k_add_keyframe, k_copy_kf_corners, k_kf_sbi and their upload forms), the relocaliser's scores and frame
// template (attempts), the trails and the homography matches (n_trails; k_trail_start), the per-frame lists of the tracker.
#include "vslam_internal.h"
#include <string.h>

#define RESET_THREADS 256
#define RESET_BLOCKS 32          // workgroups per stream: a full table (128 keyframes x 4096 points, 12.6 MB) is 1536 stores per lane

static_assert(sizeof(MeasDev) == 24 && sizeof(TrackData) % 8 == 0 && TMPL_PITCH % 8 == 0 && sizeof(Pose) % 8 == 0, "the clears below store 8-byte words");

template <class T>
DEVFN void clear_words(T* p, size_t n_words, size_t tid, size_t nth) {
  unsigned long long* q = (unsigned long long*)p;
  for (size_t i = tid; i < n_words; i += nth) q[i] = 0ull;
}
DEVFN void clear_ints(int* p, size_t n, size_t tid, size_t nth) { for (size_t i = tid; i < n; i += nth) p[i] = 0; }

// blockIdx.y = stream; the RESET_BLOCKS workgroups of a flagged stream share every array, consecutive lanes store consecutive words
__global__ __launch_bounds__(RESET_THREADS) void k_reset_clear(MapDev m, TrackParams tp, const unsigned char* flags, RelocInfo* reloc) {
  const int s = blockIdx.y;
  if (!flags[s]) return;
  const TrackerState* st = &m.st[s];                                // still the old one: k_reset_state is the next launch
  const size_t P = tp.max_points, K = tp.max_keyframes;
  const size_t np = st->n_points < 0 ? 0 : ((size_t)st->n_points < P ? (size_t)st->n_points : P);
  size_t nk = st->n_kf < 0 ? 0 : (size_t)st->n_kf + 1;              // + the slot a keyframe that never joined the map may have been copied into
  if (nk > K) nk = K;
  const size_t tid = (size_t)blockIdx.x * RESET_THREADS + threadIdx.x, nth = (size_t)gridDim.x * RESET_THREADS;
  const size_t row = np * (sizeof(MeasDev) / 8);
  unsigned long long* km = (unsigned long long*)(m.kf_meas + (size_t)s * K * P);
  for (size_t i = tid; i < nk * row; i += nth) { const size_t k = i / row; km[k * P * (sizeof(MeasDev) / 8) + (i - k * row)] = 0ull; }
  clear_words(m.cur_meas + (size_t)s * P, row, tid, nth);
  clear_words(m.td + (size_t)s * P, np * (sizeof(TrackData) / 8), tid, nth);
  clear_words(m.tmpl + (size_t)s * P * TMPL_PITCH, np * (TMPL_PITCH / 8), tid, nth);
  clear_ints(m.pt_flags + (size_t)s * P, np, tid, nth);
  clear_ints(m.pt_level + (size_t)s * P, np, tid, nth);
  if (m.never_retry) clear_words(m.never_retry + (size_t)s * P * 2, np * 2, tid, nth);
  clear_words(m.kf_pose + (size_t)s * K, K * (sizeof(Pose) / 8), tid, nth);
  clear_words(m.kf_depth + (size_t)s * K * 2, K * 2, tid, nth);
  clear_ints(m.kf_fixed + (size_t)s * K, K, tid, nth);
  if (m.kf_ncorners) clear_ints(m.kf_ncorners + (size_t)s * K * NLEV, K * NLEV, tid, nth);
  if (reloc && tid == 0) { const RelocInfo z = {}; reloc[s] = z; }
}

// one lane per stream: what the reset dropped, then the state of a new system's stream
__global__ void k_reset_state(MapDev m, int S, const unsigned char* flags, int* info, int* retire_info, int* merge_info, int* fuse_info, int* overlay_ran, unsigned char* sbi_restart, unsigned pvs_seed) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S || !flags[s]) return;
  TrackerState* st = &m.st[s];
  int* o = info + 4 * (size_t)s;
  o[0]++; o[1] = st->frame; o[2] = st->n_kf; o[3] = st->n_points;
  *st = tracker_reset_state(pvs_seed);
  if (retire_info) for (int k = 0; k < 6; k++) retire_info[6 * (size_t)s + k] = 0;   // vslam_get_retire_info: a new system's
  if (merge_info) for (int k = 0; k < 6; k++) merge_info[6 * (size_t)s + k] = 0;     // vslam_get_merge_info: a new system's
  if (fuse_info) for (int k = 0; k < 8; k++) fuse_info[8 * (size_t)s + k] = 0;       // vslam_get_fuse_info and the pairs: a new system's
  if (overlay_ran) overlay_ran[s] = -1;                                              // no discs until TrackMap has run again
  if (sbi_restart) sbi_restart[s] = 1;
}

#define RESET_RING 4

int reset_alloc(vslam_system* sys) {
  DevOwner& own = sys->own;
  VCHK(own.alloc(&sys->reset_flags, (size_t)sys->S, sys->stream));
  VCHK(own.alloc(&sys->reset_info, (size_t)sys->S * 4, sys->stream));
  if (sys->p.use_sbi) VCHK(own.alloc(&sys->sbi_restart, (size_t)sys->S, sys->stream));
  for (int q = 0; q < RESET_RING; q++) {
    VCHK(own.pinned((void**)&sys->reset_stage[q], (size_t)sys->S));
    VCHK(own.event(&sys->ev_reset_stage[q], false));
  }
  VCHK(own.event(&sys->ev_reset, false));
  for (int k = 0; k < 2; k++) VCHK(own.event(&sys->ev_reset_t[k], true));
  sys->ev_reset_ba.assign(sys->ba_streams.size(), nullptr);
  for (hipEvent_t& e : sys->ev_reset_ba) VCHK(own.event(&e, false));
  return VSLAM_OK;
}

extern "C" int vslam_reset_streams(vslam_system* sys, const int* streams, int n) {
  if (!sys || (streams && n < 0)) { vslam_set_error("reset_streams: bad argument"); return VSLAM_E_INVALID; }
  if (sys->frame_open) { vslam_set_error("reset_streams: a frame is open (vslam_finish_frame first)"); return VSLAM_E_STATE; }
  if (streams) for (int i = 0; i < n; i++)
    if (streams[i] < 0 || streams[i] >= sys->S) { vslam_set_error("reset_streams: stream %d of %d (entry %d); nothing was reset", streams[i], sys->S, i); return VSLAM_E_INVALID; }
  if (streams && n == 0) return VSLAM_OK;
  // the flags travel through pinned memory, so the copy is ordered on the stream and the host goes on; an entry of the ring is
  // reused four calls later, and only then does the host look at whether that old copy has left (it has, unless four resets queue up
  // behind one frame)
  const int q = (int)(sys->reset_calls++ % RESET_RING);
  HIPCHK(hipEventSynchronize(sys->ev_reset_stage[q]));
  unsigned char* f = sys->reset_stage[q];
  memset(f, streams ? 0 : 1, (size_t)sys->S);
  if (streams) for (int i = 0; i < n; i++) f[streams[i]] = 1;
  HIPCHK(hipEventRecord(sys->ev_reset_t[0], sys->stream));
  HIPCHK(hipMemcpyAsync(sys->reset_flags, f, (size_t)sys->S, hipMemcpyHostToDevice, sys->stream));
  HIPCHK(hipEventRecord(sys->ev_reset_stage[q], sys->stream));
  int r = ba_reset_streams(sys, sys->reset_flags); if (r) return r;
  hipLaunchKernelGGL(k_reset_clear, dim3(RESET_BLOCKS, sys->S), dim3(RESET_THREADS), 0, sys->stream, sys->map, sys->tp, sys->reset_flags, sys->reloc.info);
  hipLaunchKernelGGL(k_reset_state, dim3((sys->S + 63) / 64), dim3(64), 0, sys->stream, sys->map, sys->S, sys->reset_flags, sys->reset_info, sys->retire_info, sys->merge_info, sys->fuse_info, sys->overlay_ran, sys->sbi_restart, sys->p.pvs_shuffle_seed);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(sys->ev_reset_t[1], sys->stream));
  // whatever the other streams of the system launch from now on comes after the reset
  HIPCHK(hipEventRecord(sys->ev_reset, sys->stream));
  HIPCHK(hipStreamWaitEvent(sys->fe_stream, sys->ev_reset, 0));
  for (hipStream_t st : sys->ba_streams) HIPCHK(hipStreamWaitEvent(st, sys->ev_reset, 0));
  if (sys->p.use_sbi) sys->sbi_restart_pending = true;
  for (int s = 0; s < sys->S; s++) if (f[s]) transform_forget(sys, s);   // the transform record is the host's: a new system's
  return VSLAM_OK;
}

extern "C" int vslam_get_reset_info(vslam_system* sys, int stream, int out[4]) {
  if (!sys || stream < 0 || stream >= sys->S || !out) { vslam_set_error("get_reset_info: bad argument"); return VSLAM_E_INVALID; }
  return host_get(sys->stream, out, sys->reset_info + 4 * (size_t)stream, 4);
}

extern "C" int vslam_get_reset_timing(vslam_system* sys, double* ms) {
  if (!sys || !ms) { vslam_set_error("get_reset_timing: bad argument"); return VSLAM_E_INVALID; }
  if (sys->reset_calls == 0) { vslam_set_error("get_reset_timing: no vslam_reset_streams call yet"); return VSLAM_E_STATE; }
  HIPCHK(hipStreamSynchronize(sys->stream));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, sys->ev_reset_t[0], sys->ev_reset_t[1]));
  *ms = t;
  return VSLAM_OK;
}
