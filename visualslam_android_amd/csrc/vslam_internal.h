// Internal layout of a vslam_system: every buffer lives in HBM for the lifetime of the handle.
// gfx950 only.  Host-side bookkeeping + device pointers; kernels receive POD views.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/vslam_c.h"
#include "dev_math.h"

#define NLEV VSLAM_LEVELS

void vslam_set_error(const char* fmt, ...);

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      vslam_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return VSLAM_E_HIP;                                                                    \
    }                                                                                        \
  } while (0)

// a failed call inside csrc/ has set the error string: pass its status up
#define VCHK(expr) do { int _r = (expr); if (_r) return _r; } while (0)

// the C ABI's pose12 (R row-major, then t) <-> Pose
static inline Pose pose_from12(const double* q) { Pose p; for (int i = 0; i < 9; i++) p.R[i] = q[i]; for (int i = 0; i < 3; i++) p.t[i] = q[9 + i]; return p; }
static inline void pose_to12(const Pose& p, double* q) { for (int i = 0; i < 9; i++) q[i] = p.R[i]; for (int i = 0; i < 3; i++) q[9 + i] = p.t[i]; }

// Geometry of one pyramid level (same for every stream).
struct LevelGeom {
  int w, h;        // level size: (W >> l, H >> l)            (jni/KeyFrame.cc:21)
  int pitch;       // bytes between rows of the internal level image (multiple of 64)
  int nchunk;      // ceil(w / 64): 64-bit corner-mask words per row
  int cap;         // corner capacity per stream
  int thr;         // FAST threshold                          (jni/KeyFrame.cc:32-39)
};

// Device view of the current frame of all streams (front-end outputs).
struct FrameDev {
  // level images: img[l] + s*img_sstride[l] + y*pitch.  Level 0 may point into caller memory.
  const uint8_t* img[NLEV];
  size_t img_sstride[NLEV];
  int img_pitch[NLEV];
  unsigned long long* cmask[NLEV];  // [S][h][nchunk] corner bit masks (bit i of word c = pixel 64c+i)
  int* rowcnt[NLEV];                // [S][h]
  int* rowlut[NLEV];                // [S][h+1]  rowlut[y] = first corner index with y' >= y; [h] = n
  uint32_t* corners[NLEV];          // [S][cap]  x | y<<16, raster order
  int* ncorners;                    // [S][NLEV]
  int* overflow;                    // [1] set when any corner list hit its capacity
  // non-max products (MakeKeyFrame_Rest)
  int* scores[NLEV];                // [S][cap]
  uint32_t* maxcorners[NLEV];       // [S][cap]
  int* nmax;                        // [S][NLEV]
  // SmallBlurryImage of the frame (jni/SmallBlurryImage.h) and the rotation prior computed against the previous frame's
  uint8_t* sbi_small;               // [S][hs*ws]       mimSmall
  float* sbi_tmpl;                  // [S][hs*ws]       mimTemplate (zero-mean, blurred)
  float* sbi_jacs;                  // [S][hs*ws][2]    mimImageJacs
  double* sbi_rot;                  // [S][8]           mv6SBIRot (6), final ESM score, spare
  // subset steps (vslam_make_keyframe_lite_subset): the streams of the step this buffer was built for, written by that step only
  int* step_list;                   // [S]  launch ordinal -> stream, the first n entries
  unsigned char* held;              // [S]  1: the stream is not in the step (directly behind step_list: one upload brings both)
};


// ---- map + tracker state (all device resident) -------------------------------------------------------------------
#define POSE_WS_COMPS 12
#define TMPL_PITCH 128      // bytes reserved per cached template (11 x 11 = 121)

struct MapPointDev {        // MapPoint, jni/MapPoint.h:22-69
  double pos[3], right[3], down[3];   // v3WorldPos, v3PixelRight_W, v3PixelDown_W
  int src_kf, src_level, irx, iry;    // pPatchSourceKF, nSourceLevel, irCenter
  int bad, n_in, n_out, n_meas_kfs;   // bBad, nMEstimatorInlier/OutlierCount, |MapMakerData::sMeasurementKFs|
};

#define TDF_IN_IMAGE 1
#define TDF_FOUND 2
#define TDF_SEARCHED 4
#define TDF_SUBPIX 8
#define TDF_TMPL_BAD 16
#define TDF_HAVE_LAST 32

struct TrackData {          // TrackerData (jni/TrackerData.h:36-66) + persistent PatchFinder state (jni/PatchFinder.h:96-128)
  double cam[3], image[2], derivs[4];
  double vfound[2], sqrt_inv_noise;      // the 2x6 Jacobian and the residual live in k_pose's registers only
  double warp_inv[4], last_warp[4];
  int tsum, tsumsq;                      // nSearchLevel and the TDF_* flags live in MapDev::pt_level / pt_flags (coalesced)
};

struct MeasDev {            // Measurement, jni/KeyFrame.h:46-51 (one slot per keyframe x map point)
  double root[2];
  signed char valid, level, subpix, source;
  int pad;
};

#define BOOT_MAX_TRAILS 1000   // MaxInitialTrails, jni/Tracker.cc:305

struct TrackerState {       // Tracker members, jni/Tracker.h:77-150 (+ MapMaker flags used by the BA driver)
  Pose pose_final, start_pose, pose_cur;
  double velocity[6];
  double msd_vel, depth_mean, depth_sigma, wiggle_depth_norm;
  int frame, last_kf_dropped, lost_frames, quality;
  int attempted[NLEV], found[NLEV];
  int did_coarse, just_recovered, map_good, kf_pending;
  int n_points, n_kf;
  int pvs_count[NLEV], pvs_head[NLEV];
  int n_coarse, n_search, n_iter, n_l3;
  int coarse_range, fine_range, coarse_found;
  int ba_accepted, kf_added, ba_converged_recent, ba_converged_full;
  int ba_countdown;         // > 0: a bundle adjustment is in flight, its results are applied when this reaches 0
  unsigned long long n_zmssd, n_ba_trials;
  // the map-maker's idle jobs (vslam_params.idle_iterations)
  int newq_head;            // mqNewQueue = the points [newq_head, n_points): made by AddPointEpipolar, not yet seen by ReFindNewlyMade
  int fq_n;                 // mvFailureQueue length
  int idle_count;           // evaluations of the lowest-priority job's condition (rand() % 20 == 0 made deterministic: every 20th)
  int idle_do_fail;         // this pass runs ReFindFromFailureQueue
  int n_refound_new, n_refound_failed, n_ba_all, n_ba_recent_idle;   // statistics
  // map bootstrap (vslam_params.bootstrap; boot.hip): Tracker::TrackForInitialMap, jni/Tracker.cc:247-288
  int init_stage;           // mnInitialStage: 0 TRAIL_TRACKING_NOT_STARTED, 1 STARTED, 2 COMPLETE
  int spacebar;             // mbUserPressedSpacebar
  int n_trails, trail_buf;  // mlTrails (double-buffered: a frame's survivors are compacted into the other buffer)
  int boot_action;          // this frame: 1 TrailTracking_Start, 2 TrailTracking_Advance
  int boot_run;             // InitFromStereo is running for this stream (gates its kernels)
  int boot_ok, n_hom_inliers, n_init_points;
  unsigned boot_seed;       // stands in for the reference's rand() state
  int boot_host_matches;    // vslam_init_from_stereo: the trails are the caller's matches; this frame's TrailTracking_Advance does not search
  int recovered_now;        // vslam_params.relocalise: AttemptRecovery succeeded in this frame (jni/Tracker.cc:133-139), cleared at the frame's end
  unsigned pvs_seed;        // seed of the PVS shuffle (pvs_perm.h; jni/Tracker.cc:396-397, 525); 0: this stream keeps the identity order
};
// Tracker::Reset (jni/Tracker.cc:45-62) and MapMaker::Reset (jni/MapMaker.cc:60-74) on a zeroed TrackerState: the members that do not
// start at zero.  The only statement of them: a new system's streams (map_init_states) and a reset stream (k_reset_state) both hold
// tracker_reset_state(); pvs_seed is vslam_params.pvs_shuffle_seed.
HDFN void tracker_reset_fields(TrackerState& st, unsigned pvs_seed) {
  st.boot_seed = 1u; st.pvs_seed = pvs_seed;
  st.quality = 2; st.last_kf_dropped = -20; st.depth_mean = 1.0; st.depth_sigma = 1.0;       // jni/Tracker.cc:50-60
  st.ba_accepted = -2; st.ba_countdown = -1;
  st.ba_converged_recent = 1; st.ba_converged_full = 1;                                     // jni/MapMaker.cc:72-73
  for (int i = 0; i < 9; i++) st.pose_final.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  st.pose_cur = st.pose_final; st.start_pose = st.pose_final;
}
HDFN TrackerState tracker_reset_state(unsigned pvs_seed) { TrackerState st = {}; tracker_reset_fields(st, pvs_seed); return st; }
// Subset steps: `held` is the step's mask (FrameDev::held of the step's buffer), null in a full step and between steps.  A held stream
// is not in the step: no kernel of the step reads a decision out of its state or writes to it.  Stated once, for every gate:
DEVFN bool trk_in_step(const unsigned char* held, int s) { return !held || !held[s]; }
// jni/Tracker.cc:103-104 and :135-136: TrackMap runs for a stream that is not lost, or that the relocaliser has just recovered
DEVFN bool trk_runs_track_map(const unsigned char* held, int s, const TrackerState* st) {
  return trk_in_step(held, s) && st->map_good && (st->lost_frames < 3 || st->recovered_now);
}
// the tracker's keyframe request of THIS step (a held stream keeps the flag of its last frame, which has been served)
DEVFN bool trk_kf_pending(const unsigned char* held, int s, const TrackerState* st) { return trk_in_step(held, s) && st->kf_pending; }

struct TrackParams {        // device copy of the tunables the kernels read
  CamModel cam;
  int P;                    // patch size
  int max_ssd;              // 500 * P * P (jni/PatchFinder.cc:19-20)
  int max_patches, coarse_min, coarse_max, coarse_range, coarse_subpix_its, coarse_disabled, fine_subpix_its;
  double coarse_min_vel, wls_prior;
  int min_frames_between_kf; double max_kf_dist_wiggle_mult, wiggle_scale;
  int ba_max_iterations; double ba_convergence_limit, ba_min_sigma2; int ba_window, ba_min_keyframes;
  int quirks;
  int max_points, max_keyframes;
  int ba_delay;             // vslam_params.ba_delay_frames
  int ba_batch;             // vslam_params.ba_batch_frames (>= 1)
  int ba_sum_order;         // vslam_params.ba_sum_order
  int grow_map;             // vslam_params.grow_map
  int idle;                 // vslam_params.idle_iterations
  int fq_cap;               // capacity of a stream's failure queue
  double one_pixel_dist;    // ATANCamera::OnePixelDist, jni/ATANCamera.cc:86-91
  int kcap[NLEV];           // capacity of a keyframe's stored corner list per level (grow_map)
  int keyframe_retire;      // vslam_params.keyframe_retire: a full stream asks for its keyframe after all, retire.hip frees the slot
};

struct MapDev {             // device pointers of the map + tracker of all streams
  MapPointDev* pts;         // [S][max_points]
  TrackData* td;            // [S][max_points]
  uint8_t* tmpl;            // [S][max_points][TMPL_PITCH]
  MeasDev* kf_meas;         // [S][max_keyframes][max_points]
  MeasDev* cur_meas;        // [S][max_points]            mCurrentKF.mMeasurements
  Pose* kf_pose;            // [S][max_keyframes]
  int* kf_fixed;            // [S][max_keyframes]
  double* kf_depth;         // [S][max_keyframes][2]
  uint8_t* kf_img[NLEV];    // [S][max_keyframes][h*pitch]
  uint32_t* kf_corners[NLEV];   // [S][max_keyframes][kcap_l]  Level::vCorners of the keyframes (grow_map only: epipolar search)
  int* kf_ncorners;         // [S][max_keyframes][NLEV]
  unsigned long long* never_retry;   // [S][max_points][2]  MapMakerData::sNeverRetryKFs as a bit set over the keyframes (idle jobs only)
  int2* fq;                 // [S][fq_cap]  mvFailureQueue: (keyframe, point)
  // map bootstrap (vslam_params.bootstrap): the trails and InitFromStereo's work arrays
  uint8_t* trail_patch;     // [S][2][BOOT_MAX_TRAILS][81]  Trail::mPatch
  int* trail_pos;           // [S][2][BOOT_MAX_TRAILS][4]   irInitialPos, irCurrentPos
  double* boot_match;       // [S][BOOT_MAX_TRAILS][8]      HomographyMatch
  int* boot_inl;            // [S][BOOT_MAX_TRAILS]
  double* boot_ws;          // [S][max(3 * max_points, BOOT_MAX_TRAILS)]
  TrackerState* st;         // [S]
  int* pvs_list;            // [S][NLEV][max_points]
  int2* search_list;        // [S][max_points]  (point index, sub-pixel iterations)
  int* pt_level;            // [S][max_points]  PatchFinder::mnSearchLevel of the frame, -1 = not in the PVS (read by every planning pass)
  int* pt_flags;            // [S][max_points]  TDF_* flags
  int* iter_list;           // [S][max_points]  vIterationSet
  double* pose_ws;          // [S][POSE_WS_COMPS][max_points]  k_pose working set, component-major, indexed by iteration-set entry
  int* pose_wsi;            // [S][2][max_points]  flags, map point index
  const unsigned char* held;   // [S] the open subset step's mask (trk_in_step); null in a full step and between steps
};

// ---- relocaliser (vslam_params.relocalise; reloc.hip): Relocaliser members, jni/Relocaliser.h ----------------------------------
struct RelocInfo {
  int attempts, successes, best, frame;   // AttemptRecovery calls / those that returned true, mnBest and mnFrame of the last one
  double best_zmssd, score;               // mdBestScore, IteratePosRelToTarget's final score
  double ln_adj[6];                       // ln(SE3fromSE2(mse2))
  Pose best_pose;                         // mse3Best
};
struct RelocDev {             // all null with relocalise = 0
  float* kf_tmpl;           // [S][max_keyframes][hs*ws]      KeyFrame::pSBI->mimTemplate
  float* kf_jacs;           // [S][max_keyframes][hs*ws][2]   KeyFrame::pSBI->mimImageJacs
  float* cur_tmpl;          // [S][hs*ws]                     kCurrent.pSBI->mimTemplate of the last attempt
  double* scores;           // [S][max_keyframes]             ZMSSD against every keyframe in the last attempt
  RelocInfo* info;          // [S]
};

// What a handle holds on the device: device memory, pinned host memory, streams and events.  Every acquisition of a handle goes through
// its owner and nothing else in csrc/ creates, frees or destroys one of these, so one release() gives everything back -- after a
// destroy and after a create that failed half way alike.  Each acquiring method sets the error string and returns VSLAM_E_HIP on failure.
struct DevOwner {
  enum Kind : int { MEM, PINNED, STREAM, EVENT };
  struct Held { Kind kind; void* h; };
  std::vector<Held> held;      // in order of acquisition
  // count zeroed elements of T (and 64 bytes of slack) in HBM.  The zeroing contract, stated once: the memory is zero for every stream
  // once vslam_create / vslam_bundle_create has returned (both end with a wait for zero_on); inside create it is zero only for work
  // queued behind it on zero_on.
  template <class T> int alloc(T** out, size_t count, hipStream_t zero_on) {
    void* ptr = nullptr;
    HIPCHK(hipMalloc(&ptr, count * sizeof(T) + 64));
    held.push_back({MEM, ptr});
    HIPCHK(hipMemsetAsync(ptr, 0, count * sizeof(T) + 64, zero_on));
    *out = (T*)ptr;
    return VSLAM_OK;
  }
  int pinned(void** out, size_t bytes) {
    HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
    held.push_back({PINNED, *out});
    return VSLAM_OK;
  }
  int stream(hipStream_t* out) {
    HIPCHK(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    held.push_back({STREAM, *out});
    return VSLAM_OK;
  }
  int event(hipEvent_t* out, bool timing) {
    HIPCHK(hipEventCreateWithFlags(out, timing ? hipEventDefault : hipEventDisableTiming));
    held.push_back({EVENT, *out});
    return VSLAM_OK;
  }
  // waits for its streams, then gives everything back in reverse order of acquisition (the streams, acquired first, go last); idempotent
  void release() {
    for (const Held& x : held) if (x.kind == STREAM) (void)hipStreamSynchronize((hipStream_t)x.h);
    for (size_t i = held.size(); i-- > 0;) {
      const Held& x = held[i];
      if (x.kind == MEM) (void)hipFree(x.h);
      else if (x.kind == PINNED) (void)hipHostFree(x.h);
      else if (x.kind == EVENT) (void)hipEventDestroy((hipEvent_t)x.h);
      else (void)hipStreamDestroy((hipStream_t)x.h);
    }
    held.clear();
  }
};

// A device buffer that lives for one call: freed when it goes out of scope, on every return path.  Not zeroed.
template <class T> struct DevTemp {
  T* p = nullptr;
  DevTemp() = default;
  DevTemp(const DevTemp&) = delete;
  DevTemp& operator=(const DevTemp&) = delete;
  ~DevTemp() { if (p) (void)hipFree(p); }
  hipError_t get(size_t count) { return hipMalloc((void**)&p, count * sizeof(T)); }
};

// Host copies: every synchronous copy between the host and a handle's memory.  A handle's streams are
// non-blocking, so a copy is ordered only by the stream it is enqueued on: each goes onto the stream named here, never the null stream,
// and the wait belongs to the batch -- wait() reports it, and a batch that ends without one (an error return) waits as it goes out of
// scope (so it is declared behind the host arrays it copies).  After the wait every get() has landed and every put()'s source may be
// reused.  Kernels may be launched on q in between.
struct HostCopy {
  hipStream_t q;
  bool pending = false;        // something has been enqueued since the last wait
  explicit HostCopy(hipStream_t stream) : q(stream) {}
  HostCopy(const HostCopy&) = delete;
  ~HostCopy() { if (pending) (void)hipStreamSynchronize(q); }
  int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (bytes) { pending = true; HIPCHK(hipMemcpyAsync(dst, src, bytes, kind, q)); }
    return VSLAM_OK;
  }
  template <class T> int get(T* host, const T* dev, size_t n = 1) { return copy(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost); }
  template <class T> int put(T* dev, const T* host, size_t n = 1) { return copy(dev, host, sizeof(T) * n, hipMemcpyHostToDevice); }
  template <class T> int get(std::vector<T>& host, const T* dev, int n) { host.resize(n > 0 ? n : 0); return get(host.data(), dev, host.size()); }
  // rows of `width` bytes, the pitches in bytes
  int copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipMemcpyKind kind) {
    if (width && rows) { pending = true; HIPCHK(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, q)); }
    return VSLAM_OK;
  }
  int get2d(void* host, size_t hpitch, const void* dev, size_t dpitch, size_t width, size_t rows) { return copy2d(host, hpitch, dev, dpitch, width, rows, hipMemcpyDeviceToHost); }
  int put2d(void* dev, size_t dpitch, const void* host, size_t hpitch, size_t width, size_t rows) { return copy2d(dev, dpitch, host, hpitch, width, rows, hipMemcpyHostToDevice); }
  int wait() {
    if (pending) { pending = false; HIPCHK(hipStreamSynchronize(q)); }
    return VSLAM_OK;
  }
  // The counted read-back: a count that has landed, clamped to the caller's capacity, and that many elements (of `per` Ts each) behind it
  template <class T> int take(T* host, const T* dev, int count, int cap, size_t per = 1) {
    const int m = count < cap ? count : cap;
    return host && m > 0 ? get(host, dev, (size_t)m * per) : VSLAM_OK;
  }
  // ... the whole sequence for one array: the device's count into *count (either may be null), then the elements
  template <class T> int counted(const int* d_count, int* count, T* host, const T* dev, int cap, size_t per = 1) {
    int cnt = 0;
    VCHK(get(&cnt, d_count)); VCHK(wait());
    if (count) *count = cnt;
    VCHK(take(host, dev, cnt, cap, per)); return wait();
  }
};
// a batch of one
template <class T> static inline int host_get(hipStream_t q, T* host, const T* dev, size_t n = 1) { HostCopy c(q); VCHK(c.get(host, dev, n)); return c.wait(); }
template <class T> static inline int host_put(hipStream_t q, T* dev, const T* host, size_t n = 1) { HostCopy c(q); VCHK(c.put(dev, host, n)); return c.wait(); }

struct BaSystemWs;             // bundle-adjustment workspace (ba.hip)

// vslam_get_transform_info: the transforms a stream has seen since its creation, reset or restore, mnFrame at the last one, and the
// accumulated similarity from the original gauge to the current one (similarity_dev.h, sim_compose).  Kept on the host.
struct TransformRecord { int count, frame; Pose T; double s; };

struct vslam_system {
  vslam_params p;
  int S;
  hipStream_t stream = nullptr;
  LevelGeom geom[NLEV];
  FrameDev fr;                 // view of the CURRENT frame's front-end products (= frbuf[fr_idx])
  uint8_t* d_lvl[NLEV];        // owned level images of the current buffer (level 0 = staging copy for host input)
  // Front-end products are double-buffered and built on their own HIP stream so MakeKeyFrame_Lite of frame t+1
  // overlaps TrackMap / pose / bundle adjustment of frame t (which are latency-bound and leave the CUs mostly idle).
  FrameDev frbuf[2];
  uint8_t* d_lvl_buf[2][NLEV];
  int fr_idx = 0;
  hipStream_t fe_stream = nullptr;
  hipEvent_t ev_fe_done[2] = {nullptr, nullptr}, ev_track_done[2] = {nullptr, nullptr};
  // asynchronous map-maker (ba_delay_frames > 0): Bundle::Compute runs on ba_stream beside the following frames
  hipStream_t ba_stream = nullptr;   // the map-maker stream of the frame being enqueued (= ba_streams[frame_no % ba_streams.size()])
  std::vector<hipStream_t> ba_streams;   // a bundle adjustment outlasts a frame: successive keyframe frames' launches overlap on a ring of streams
  double* grow_implane = nullptr;   // [S][kcap_0][2]: the epipolar search's target corners on the image plane (mapgrow.hip)
  int n_cu = 0;             // compute units of the device (asynchronous map-maker: size of the background BA grid)
  std::vector<hipEvent_t> ev_asm, ev_ba;   // rings of ba_delay + 2 events, indexed by batch number
  long frame_no = 0;
  long ba_token = 0;           // ba_run calls so far: k_ba_select marks the problems it wants with the call's token, k_ba_assemble takes only those
  // batches of the asynchronous map-maker: the problems assembled in ba_batch consecutive frames share one work list and one launch
  long ba_batch_id = 0;        // the open batch
  int ba_batch_fill = 0;       // frames assembled into it so far
  std::vector<long> frame_batch;   // ring [ba_delay + 2]: the batch a frame's keyframes were assembled into
  std::vector<int> prof_ba_launched;    // per profiled frame: 0, or 1 + the launch record (BaPool::lstat) of the k_ba_compute it launched
  long ba_launch_no = 0;       // k_ba_compute launches of this system so far (ring index of the launch records)
  hipEvent_t ev_mm[4] = {nullptr, nullptr, nullptr, nullptr};   // host-driven BundleAdjustRecent / All: before select+assemble, compute, write-back, after
  int mm_lrec = -1;            // launch record of the last host-driven call
  DevOwner own;               // everything the handle holds on the device; vslam_destroy releases it
  bool have_frame;
  bool frame_open = false;  // stage-wise TrackFrame (vslam_patch_search ... vslam_finish_frame) in progress
  bool frame_tracked = false;   // ... and its vslam_pose_update(sys, 1) has been enqueued: the frame's tracker read-backs are final
  bool have_sbi;            // a SmallBlurryImage of a previous frame exists (mpSBILastFrame)
  // subset steps.  The list and the mask of a step travel through pinned memory, one block per front-end buffer: the front end of
  // step t+1 uploads its own while the tracker of step t still reads the other buffer's.
  unsigned char* step_stage[2] = {nullptr, nullptr};   // pinned: [S] ints (the list), then [S] bytes (the mask)
  hipEvent_t ev_step_stage[2] = {nullptr, nullptr};    // the upload out of step_stage[b] has finished
  bool step_stage_used[2] = {false, false};
  bool step_subset = false;                  // the current / last step was a subset step
  std::vector<unsigned char> step_in;        // [S] host: 1 for the streams of the current / last step
  const unsigned char* fe_held = nullptr;    // the current buffer's mask (device) while step_subset, else null: gates the front-end products
  std::vector<unsigned char> sbi_seen;       // [S] host (use_sbi): the stream has had a frame; a first frame in a subset step aligns to itself
  bool sbi_all_seen = false;
  // KeyFrame::Level::vCandidates of the current frame (jni/KeyFrame.h:62-70), filled by vslam_make_keyframe_rest
  uint32_t* cand[NLEV]; double* cand_score[NLEV]; int* ncand; bool have_candidates;
  // vslam_reset_streams (reset.hip)
  unsigned char* reset_flags = nullptr;      // [S] device: the streams the reset kernels of the call in flight work on
  unsigned char* reset_stage[4] = {nullptr, nullptr, nullptr, nullptr};   // pinned host copies of the flags, a ring: a call never waits for the one before it
  hipEvent_t ev_reset_stage[4] = {nullptr, nullptr, nullptr, nullptr};    // ... the copy out of a ring entry has finished
  long reset_calls = 0;
  int* reset_info = nullptr;                 // [S][4] device: vslam_get_reset_info
  unsigned char* sbi_restart = nullptr;      // [S] device (use_sbi): the stream's next frame is its first, "last frame" = itself (jni/Tracker.cc:90-92)
  bool sbi_restart_pending = false;          // some flag of sbi_restart is set: the next frame launches k_sbi_restart once
  hipEvent_t ev_reset_t[2] = {nullptr, nullptr};   // around the last call's work on the system's stream (vslam_get_reset_timing)
  hipEvent_t ev_reset = nullptr;             // the reset kernels are done (the front-end and map-maker streams wait for it)
  std::vector<hipEvent_t> ev_reset_ba;       // one per map-maker stream: what it held when the reset was called
  // keyframe retirement (retire.hip): allocated with keyframe_retire != 0 or by the first vslam_retire_keyframes, else null
  int* retire_remap = nullptr;               // [S][max_points] device: new index of a surviving point, -1 of a dropped one
  int* retire_plan = nullptr;                // [S][RETIRE_PLAN_N] device: what k_retire_plan decided, for the kernels that move
  int* retire_req = nullptr;                 // [S] device: the explicit call's request per stream
  int* retire_info = nullptr;                // [S][6] device: vslam_get_retire_info
  int* retire_req_stage = nullptr;           // [S] pinned host copy of the request
  hipEvent_t ev_retire_t[2] = {nullptr, nullptr};   // around the last explicit call's launches (vslam_get_retire_timing)
  long retire_calls = 0;
  // vslam_transform_maps (transform.hip): the call's argument array, sized for every stream at creation
  void* transform_args = nullptr;            // [S] device: stream, T, T^-1 and s per ordinal of the call in flight
  void* transform_stage = nullptr;           // [S] pinned host copy of them
  std::vector<TrackerState> transform_states;   // [S] host: the listed streams' states, read once per call
  std::vector<TransformRecord> transform_rec;   // [S] host: vslam_get_transform_info
  hipEvent_t ev_transform_t[2] = {nullptr, nullptr};   // around the last call's launch (vslam_get_transform_timing)
  long transform_calls = 0;
  // vslam_merge_maps (merge.hip): allocated by the first call, else null
  int* merge_plan = nullptr;                 // [S][MERGE_PLAN_N] device: the plan record of each pair of the call in flight
  int* merge_info = nullptr;                 // [S][6] device: vslam_get_merge_info
  int* merge_plan_stage = nullptr;           // pinned host copy of the request the plan starts from
  hipEvent_t ev_merge_t[2] = {nullptr, nullptr};   // around the last call's launches (vslam_get_merge_timing)
  long merge_calls = 0;
  // vslam_fuse_points (fuse.hip): allocated by the first call, else null
  int* fuse_partner = nullptr;               // [S][max_points] device: partner(p) of the call in flight, -1 none
  int2* fuse_pairs = nullptr;                // [S][max_points] device: the (dropped, kept) pairs of a stream's last call, ascending by dropped
  int* fuse_info = nullptr;                  // [S][8] device: vslam_get_fuse_info's six, then whether the stream has been listed
  int* fuse_list = nullptr;                  // [S] device: ordinal -> stream of the call in flight
  int* fuse_list_stage = nullptr;            // pinned host copy of it
  hipEvent_t ev_fuse_t[2] = {nullptr, nullptr};   // around the last call's launches (vslam_get_fuse_timing)
  long fuse_calls = 0;
  // the overlay renderer (overlay.hip; vslam_params.overlay): null with overlay = 0
  int* overlay_ran = nullptr;                // [S] device: mnFrame at which TrackMap last ran for the stream, -1 never (or forgotten by a reset)
  int* overlay_info = nullptr;               // [S][3] device: discs, lines, marks of the stream's last render
  int* overlay_list = nullptr;               // [S] device: image -> stream of the last render that had a list
  hipEvent_t ev_overlay_t[2] = {nullptr, nullptr};   // around the last render's launches (vslam_get_render_timing)
  long overlay_calls = 0;
  // vslam_snapshot_stream / vslam_restore_stream (snapshot.hip)
  hipEvent_t ev_snap_t[4] = {nullptr, nullptr, nullptr, nullptr};   // around the last pack [0, 1] and the last unpack [2, 3] on the system's stream
  bool snap_timed[2] = {false, false};       // a pack / an unpack has run
  bool boot_key_pressed = false;   // vslam_press_spacebar since the last frame: that frame launches the start / InitFromStereo pipelines
  std::vector<unsigned char> boot_key_stream;   // [S] host: ... for which streams (a subset step serves only its own)
  TrackParams tp;
  MapDev map;
  BaSystemWs* ba_ws = nullptr; // bundle-adjustment workspace (ba.hip): ba_alloc makes it, ba_free deletes it
  RelocDev reloc = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // per-stage HIP-event timing of vslam_track_frame (vslam_profile_begin/end)
  std::vector<hipEvent_t> prof_ev;
  int prof_cap = 0, prof_frame = 0;
  bool prof_on = false;
};

// The profile's stages, in the order of vslam_stage_name (kStageNames, map.hip); a stage's mark is the event at its start, and
// PROF_FRAME_END, the mark after the last stage, closes the frame.
enum ProfStage : int {
  PROF_PYR_FAST0, PROF_FAST_LVL, PROF_COMPACT, PROF_PVS, PROF_PLAN_COARSE, PROF_SEARCH_COARSE, PROF_POSE_COARSE, PROF_PLAN_FINE,
  PROF_SEARCH_FINE, PROF_POSE_FINE, PROF_ADD_KEYFRAME, PROF_BA_ASSEMBLE, PROF_BA_COMPUTE, PROF_BA_WRITEBACK, PROF_FRAME_END
};
static_assert(PROF_FRAME_END == VSLAM_N_STAGES, "ProfStage names every stage of include/vslam_c.h");
#define PROF_MARKS (VSLAM_N_STAGES + 3)   // the front end's marks + PROF_FE_END on the front-end stream, PROF_PVS..PROF_FRAME_END on the main stream
#define PROF_FE_END (VSLAM_N_STAGES + 1)
#define PROF_BA_END (VSLAM_N_STAGES + 2)  // asynchronous map-maker: PROF_BA_COMPUTE and PROF_BA_END live on the BA stream
static inline void prof_mark(vslam_system* sys, int k) {
  if (!(sys->prof_on && sys->prof_frame < sys->prof_cap)) return;
  hipStream_t st = sys->stream;
  if (k <= PROF_COMPACT || k == PROF_FE_END) st = sys->fe_stream;
  else if (sys->tp.ba_delay > 0 && (k == PROF_BA_COMPUTE || k == PROF_BA_END)) st = sys->ba_stream;
  (void)hipEventRecord(sys->prof_ev[(size_t)sys->prof_frame * PROF_MARKS + k], st);
}

// frontend.hip
int fe_make_keyframe_lite(vslam_system* sys, const uint8_t* gray, size_t row_stride, size_t stream_stride,
                          int on_device, const int* streams = nullptr, int n = -1);   // n >= 0: a subset step for streams[0..n)
int fe_stream_in_step(vslam_system* sys, int stream, const char* who);   // VSLAM_E_STATE for a stream the current / last step held
int fe_fast_nonmax(vslam_system* sys);
int fe_keyframe_corners(vslam_system* sys, int s, int kf);   // FAST corners of a stored keyframe into MapDev::kf_corners (map upload)
int fe_keyframe_rest_gated(vslam_system* sys);               // non-max + candidates of the current frame for the streams with kf_pending
int fe_thin_new_keyframe(vslam_system* sys, int level);      // ThinCandidates(new keyframe, level) for the streams with kf_pending
int grow_alloc(vslam_system* sys);
int grow_on_keyframe(vslam_system* sys);                      // AddSomeMapPoints(3, 0, 1, 2) for the streams with kf_pending
enum IdleRefind : int { REFIND_NEWLY_MADE = 0, REFIND_FAILURE_QUEUE = 1 };
int grow_idle_refind(vslam_system* sys, int mode);            // idle jobs: an IdleRefind (gated per stream on device)
int mm_idle(vslam_system* sys);
int boot_alloc(vslam_system* sys);
int boot_frame(vslam_system* sys);                                        // TrackForInitialMap for the streams without a map (vslam_params.bootstrap)
int grow_copy_corners(vslam_system* sys);                                 // Level::vCorners of the current frame into the keyframe slot n_kf (streams with kf_pending)
int grow_levels(vslam_system* sys, const int* order, int n);              // ThinCandidates + AddPointEpipolar per level, in this order (streams with kf_pending)
int ba_launch_add_keyframe(vslam_system* sys);                            // k_add_keyframe for the streams with kf_pending
enum IdleJob : int { IDLE_BA_RECENT = 0, IDLE_REFIND_NEW = 1, IDLE_BA_ALL = 2, IDLE_REFIND_FAILED = 3, IDLE_N_JOBS };   // the job numbers of vslam_mapmaker_idle_job
int mm_idle_job(vslam_system* sys, int job);                               // vslam_params.idle_iterations passes through MapMaker::run's idle jobs
int fe_sbi(vslam_system* sys, const FrameDev& last, const int* list, int n);   // k_sbi on the front-end stream: this frame's SBI + rotation prior against `last`, for n streams (list: null = all, identity)
int fe_sbi_carry(vslam_system* sys, const FrameDev& last);   // subset step: the held streams' SBI products move from `last` into the current buffer
int fe_sbi_restart(vslam_system* sys);                 // ... again against the frame itself for the streams vslam_reset_streams flagged (once, then the flags are clear)
void cam_fill(CamModel& c, const double cam5[5], double width, double height, int quirks);
int fe_make_keyframe_rest(vslam_system* sys, double min_score);
int fe_thin_candidates(vslam_system* sys, int keyframe);
// track.hip
void trk_fill_params(const vslam_params& p, TrackParams& t);
int trk_alloc(vslam_system* sys);
int trk_track_map(vslam_system* sys);
int trk_search_stage(vslam_system* sys, int stage);
int trk_pose_stage(vslam_system* sys, int stage);
// ba.hip
// What a caller asks of the map-maker (ba_run; k_ba_select gates it per stream).  Line numbers: jni/MapMaker.cc.
enum class BaJob : int {
  Keyframe = 0,        // AddKeyFrame + BundleAdjustRecent for the streams with kf_pending (tracker- or host-driven)
  Recent = 1,          // BundleAdjustRecent, every stream
  All = 2,             // BundleAdjustAll, every stream (:776-851)
  IdleRecent = 3,      // idle job of MapMaker::run: Recent for the streams whose adjustment has not converged (:97-98)
  IdleAll = 4,         // ... All for the streams whose Recent has converged and whose All has not (:107-108)
  BootAll = 5,         // InitFromStereo's five BundleAdjustAll, for the streams it runs for (:344-345)
  BootAllUntilConverged = 6,   // ... and its BundleAdjustAll until mbBundleConverged_Full (:361-365)
};
// What k_ba_writeback is asked to do with the results in the pool
enum class BaWriteback : int {
  Keyframe = 0,        // this frame's keyframe (streams with kf_pending); left to IfDue / Drain when ba_delay > 0
  Recent = 1,          // apply now: a BundleAdjustRecent
  All = 2,             // apply now: a BundleAdjustAll
  IfDue = 3,           // asynchronous map-maker: apply a stream's pending (Recent) result if its countdown says it is due
  Drain = 4,           // ... make the pending result due now
  Boot = 5,            // a BundleAdjustAll of InitFromStereo: only the streams it runs for
};
// What each job implies, stated once:
constexpr bool ba_job_all(BaJob j) { return j == BaJob::All || j == BaJob::IdleAll || j >= BaJob::BootAll; }   // all keyframes, or the window around the newest
constexpr bool ba_job_on_request(BaJob j) { return j == BaJob::Recent || j == BaJob::All; }   // vslam_bundle_adjust_recent / _all: drains first, is timed
constexpr BaWriteback ba_job_writeback(BaJob j) {
  return j == BaJob::Keyframe ? BaWriteback::Keyframe : j >= BaJob::BootAll ? BaWriteback::Boot : ba_job_all(j) ? BaWriteback::All : BaWriteback::Recent;
}
DEVFN bool ba_job_gate(BaJob j, const TrackerState& st) {   // the streams it runs for, beside map_good and no adjustment in flight
  switch (j) {
    case BaJob::Keyframe: return st.kf_pending;
    case BaJob::IdleRecent: return !st.ba_converged_recent;
    case BaJob::IdleAll: return st.ba_converged_recent && !st.ba_converged_full;
    case BaJob::BootAll: return st.boot_run;
    case BaJob::BootAllUntilConverged: return st.boot_run && !st.ba_converged_full;
    default: return true;
  }
}
DEVFN int* ba_job_idle_counter(BaJob j, TrackerState* st) {   // the counter of vslam_get_idle_stats it bumps for them
  return j == BaJob::IdleRecent ? &st->n_ba_recent_idle : j == BaJob::IdleAll ? &st->n_ba_all : nullptr;
}
int ba_alloc(vslam_system* sys);
void ba_free(vslam_system* sys);          // the host-side workspace (its device memory is the owner's)
int ba_add_keyframe_and_adjust(vslam_system* sys);
int ba_run(vslam_system* sys, BaJob job, bool host_driven_keyframe = false);
int ba_frame_start(vslam_system* sys);    // asynchronous map-maker: apply the results that are due at this frame
int ba_sync_streams(vslam_system* sys);   // host wait for every map-maker stream (an open batch is launched first)
// reloc.hip
int reloc_alloc(vslam_system* sys);
int reloc_keyframe_sbi_pending(vslam_system* sys);                        // SmallBlurryImage of the keyframe k_add_keyframe has just stored (streams with kf_pending)
int reloc_keyframe_sbi(vslam_system* sys, int s, int first, int n);       // ... of the uploaded keyframes [first, first + n) of stream s
int reloc_attempt_recovery(vslam_system* sys);
int ba_reset_streams(vslam_system* sys, const unsigned char* d_flags);   // the pool records (and work-list entries) of the flagged streams, as a new system's
// map.hip
int map_init_states(vslam_system* sys);
// reset.hip
int reset_alloc(vslam_system* sys);
// snapshot.hip
int snapshot_alloc(vslam_system* sys);
// overlay.hip
int overlay_alloc(vslam_system* sys);
int overlay_note_track_map(vslam_system* sys);   // overlay = 1: records the frame for the streams whose TrackMap runs; the launch in front of k_motion
int overlay_forget_listed(vslam_system* sys, const int* d_req, int not_listed);   // ... back to -1 for the streams a retirement lists
// transform.hip
int transform_alloc(vslam_system* sys);
void transform_forget(vslam_system* sys, int s);   // a reset or restored stream: no transforms, the identity
// retire.hip
int retire_alloc(vslam_system* sys);          // the scratch of keyframe retirement, if the system does not hold it yet
int retire_on_keyframe(vslam_system* sys);    // keyframe_retire: one keyframe by policy for the full streams with kf_pending, before k_add_keyframe

