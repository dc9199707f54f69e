// vslam_system lifetime, parameters and read-back entry points of the C ABI (include/vslam_c.h).
#include "vslam_internal.h"
#include "grow_dev.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static thread_local char g_err[512] = "";

void vslam_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* vslam_last_error(void) { return g_err; }

extern "C" int vslam_default_params(vslam_params* p, int width, int height, int n_streams) {
  if (!p || width < 48 || height < 48 || n_streams < 1) { vslam_set_error("default_params: bad size"); return VSLAM_E_INVALID; }
  memset(p, 0, sizeof(*p));
  p->width = width; p->height = height; p->n_streams = n_streams;
  p->fast_threshold[0] = 10; p->fast_threshold[1] = 15; p->fast_threshold[2] = 15; p->fast_threshold[3] = 10;
  p->nonmax_barrier = 10;
  p->patch_size = 11;
  for (int l = 0; l < NLEV; l++) {
    const int n = ((width >> l) * (height >> l)) / 2;
    p->max_corners[l] = n < 256 ? 256 : n;
  }
  p->max_points = 4096;
  p->max_keyframes = 32;
  p->max_patches_per_frame = 1000;
  p->coarse_min = 20; p->coarse_max = 60; p->coarse_range = 30; p->coarse_subpix_its = 8;
  p->coarse_disabled = 0; p->coarse_min_vel = 0.006;
  p->fine_subpix_its = 8;
  p->wls_prior = 100.0;
  p->use_sbi = 0;
  p->min_frames_between_kf = 20;
  p->max_kf_dist_wiggle_mult = 0.2;
  p->wiggle_scale = 0.1;
  p->ba_max_iterations = 20;
  p->ba_convergence_limit = 1e-6;
  p->ba_min_tukey_sigma = 0.4;
  p->ba_window = 5;
  p->ba_min_keyframes = 8;
  p->cam[0] = 0.841906; p->cam[1] = 1.10893; p->cam[2] = 0.505171; p->cam[3] = 0.470265; p->cam[4] = -0.0133843;
  p->quirks = 0;
  p->device = 0;
  p->ba_delay_frames = 0;
  p->grow_map = 0;
  p->ba_batch_frames = 1;
  p->idle_iterations = 0;
  p->bootstrap = 0;
  p->ba_sum_order = 0;
  p->relocalise = 0;
  p->reloc_blur = 2.5;                                  // jni/SmallBlurryImage.h:19-20
  p->pvs_shuffle_seed = 0;                              // identity order (jni/Tracker.cc:396-397, 525 shuffle with rand())
  p->keyframe_retire = 0;                               // a full map stops making keyframes
  p->overlay = 0;                                       // no renderer: nothing allocated, nothing launched
  return VSLAM_OK;
}

// Everything a new handle acquires, through its owner; vslam_create gives a handle that failed here to vslam_destroy.
static int sys_acquire(vslam_system* sys) {
  const vslam_params* p = &sys->p;
  DevOwner& own = sys->own;
  // (default priorities: the tracker's stream at the highest priority, with or without the front end's at the lowest, was measured at
  // 3072 streams: 376 k against 398-400 k frames/s -- the front end of frame t+1 then finishes late and the tracker waits for it)
  VCHK(own.stream(&sys->stream));
  hipStream_t q = sys->stream;
  const int S = sys->S;
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, p->device) == hipSuccess && ncu > 0) sys->n_cu = ncu;
  }
  VCHK(own.stream(&sys->fe_stream));
  for (int b = 0; b < 2; b++) { VCHK(own.event(&sys->ev_fe_done[b], false)); VCHK(own.event(&sys->ev_track_done[b], false)); }
  for (int k = 0; k < 4; k++) VCHK(own.event(&sys->ev_mm[k], true));
  for (int l = 0; l < NLEV; l++) {
    LevelGeom& g = sys->geom[l];
    g.w = p->width >> l; g.h = p->height >> l;
    g.pitch = (g.w + 63) & ~63;
    g.nchunk = (g.w + 63) >> 6;
    g.cap = p->max_corners[l];
    g.thr = p->fast_threshold[l];
  }
  for (int b = 0; b < 2; b++) {
    FrameDev& fr = sys->frbuf[b];
    for (int l = 0; l < NLEV; l++) {
      const LevelGeom& g = sys->geom[l];
      VCHK(own.alloc(&sys->d_lvl_buf[b][l], (size_t)S * g.pitch * g.h, q));
      VCHK(own.alloc(&fr.cmask[l], (size_t)S * g.h * g.nchunk, q));
      VCHK(own.alloc(&fr.rowcnt[l], (size_t)S * g.h, q));
      VCHK(own.alloc(&fr.rowlut[l], (size_t)S * (g.h + 1), q));
      VCHK(own.alloc(&fr.corners[l], (size_t)S * g.cap, q));
      VCHK(own.alloc(&fr.scores[l], (size_t)S * g.cap, q));
      VCHK(own.alloc(&fr.maxcorners[l], (size_t)S * g.cap, q));
      fr.img[l] = sys->d_lvl_buf[b][l];
      fr.img_sstride[l] = (size_t)g.pitch * g.h;
      fr.img_pitch[l] = g.pitch;
    }
    {
      const size_t ns = (size_t)(sys->geom[3].w / 2) * (sys->geom[3].h / 2);
      VCHK(own.alloc(&fr.sbi_small, (size_t)S * ns, q)); VCHK(own.alloc(&fr.sbi_tmpl, (size_t)S * ns, q));
      VCHK(own.alloc(&fr.sbi_jacs, (size_t)S * ns * 2, q)); VCHK(own.alloc(&fr.sbi_rot, (size_t)S * 8, q));
    }
    VCHK(own.alloc(&fr.ncorners, (size_t)S * NLEV, q));
    VCHK(own.alloc(&fr.nmax, (size_t)S * NLEV, q));
    VCHK(own.alloc(&fr.overflow, 1, q));
    {                                                                // a subset step's list and mask (all zero: nothing held), and their pinned staging block
      unsigned char* blk = nullptr;
      VCHK(own.alloc(&blk, (size_t)S * (sizeof(int) + 1), q));
      fr.step_list = (int*)blk; fr.held = blk + (size_t)S * sizeof(int);
      void* pin = nullptr;
      VCHK(own.pinned(&pin, (size_t)S * (sizeof(int) + 1)));
      sys->step_stage[b] = (unsigned char*)pin;
      VCHK(own.event(&sys->ev_step_stage[b], false));
    }
  }
  sys->step_in.assign((size_t)S, 1);
  sys->sbi_seen.assign((size_t)S, 0);
  sys->boot_key_stream.assign((size_t)S, 0);
  sys->map.held = nullptr;
  for (int l = 0; l < NLEV; l++) { VCHK(own.alloc(&sys->cand[l], (size_t)S * sys->geom[l].cap, q)); VCHK(own.alloc(&sys->cand_score[l], (size_t)S * sys->geom[l].cap, q)); }
  VCHK(own.alloc(&sys->ncand, (size_t)S * NLEV, q));
  sys->have_candidates = false;
  sys->have_sbi = false;
  if (p->ba_delay_frames > 0) {
    // (default priority: giving the map-maker's streams the lowest one was measured -- the adjustments then finish late and the
    // frames that apply them wait: 215 k against 243 k frames/s; the highest one changes nothing: 340 k either way at 2048 streams)
    sys->ba_streams.assign(p->ba_delay_frames < 8 ? p->ba_delay_frames : 8, nullptr);
    for (hipStream_t& st : sys->ba_streams) VCHK(own.stream(&st));
    sys->ba_stream = sys->ba_streams[0];
    sys->frame_batch.assign((size_t)p->ba_delay_frames + 2, -1L);
    sys->ev_asm.assign((size_t)p->ba_delay_frames + 2, nullptr); sys->ev_ba = sys->ev_asm;
    for (size_t i = 0; i < sys->ev_asm.size(); i++) { VCHK(own.event(&sys->ev_asm[i], false)); VCHK(own.event(&sys->ev_ba[i], false)); }
  }
  sys->fr_idx = 0;
  sys->fr = sys->frbuf[0];
  for (int l = 0; l < NLEV; l++) sys->d_lvl[l] = sys->d_lvl_buf[0][l];
  VCHK(trk_alloc(sys));
  VCHK(ba_alloc(sys));
  VCHK(grow_alloc(sys));
  VCHK(boot_alloc(sys));
  VCHK(reloc_alloc(sys));
  VCHK(reset_alloc(sys));
  VCHK(snapshot_alloc(sys));
  if (p->keyframe_retire) VCHK(retire_alloc(sys));
  VCHK(overlay_alloc(sys));
  VCHK(transform_alloc(sys));
  VCHK(map_init_states(sys));            // (on q, behind the zeroing of the states)
  HIPCHK(hipStreamSynchronize(q));       // the zeroing contract (DevOwner::alloc): from here on the memory is zero for every stream
  return VSLAM_OK;
}

extern "C" int vslam_create(const vslam_params* p, vslam_system** out) {
  if (!p || !out) { vslam_set_error("create: null argument"); return VSLAM_E_INVALID; }
  if (p->width < 48 || p->height < 48 || p->width > 4096 || p->height > 4096 || p->n_streams < 1 ||
      (p->patch_size != 8 && p->patch_size != 11) || p->ba_delay_frames < 0 || p->ba_delay_frames >= 20 ||
      (p->ba_delay_frames > 0 && p->ba_delay_frames >= p->min_frames_between_kf) || p->ba_batch_frames < 0 ||
      (p->ba_batch_frames > 1 && p->ba_batch_frames > p->ba_delay_frames) || p->idle_iterations < -1 ||
      (p->idle_iterations != 0 && p->ba_delay_frames > 0)) {
    vslam_set_error("create: unsupported parameters: size %dx%d (48..4096), streams %d (>= 1), patch %d (8 or 11), ba_delay_frames %d (0..19 and below min_frames_between_kf %d), ba_batch_frames %d (0..ba_delay_frames), idle_iterations %d (>= -1, non-zero only with ba_delay_frames = 0)",
                    p->width, p->height, p->n_streams, p->patch_size, p->ba_delay_frames, p->min_frames_between_kf, p->ba_batch_frames, p->idle_iterations);
    return VSLAM_E_INVALID;
  }
  if (p->bootstrap && (p->grow_map == 0 || p->ba_delay_frames > 0)) {
    vslam_set_error("create: bootstrap needs grow_map != 0 (keyframe corner lists for InitFromStereo's AddSomeMapPoints) and ba_delay_frames = 0, got grow_map %d, ba_delay_frames %d", p->grow_map, p->ba_delay_frames);
    return VSLAM_E_INVALID;
  }
  if (p->keyframe_retire && p->max_keyframes < 3) { vslam_set_error("create: keyframe_retire needs max_keyframes >= 3 (a map keeps at least two), got %d", p->max_keyframes); return VSLAM_E_INVALID; }
  if (p->relocalise && !(p->reloc_blur > 0.0)) { vslam_set_error("create: relocalise needs reloc_blur > 0, got %g", p->reloc_blur); return VSLAM_E_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    vslam_set_error("create: no HIP device visible (the MI355X path has no CPU fallback)");
    return VSLAM_E_HIP;
  }
  HIPCHK(hipSetDevice(p->device));
  vslam_system* sys = new vslam_system();
  sys->p = *p;
  sys->S = p->n_streams;
  sys->have_frame = false;
  const int r = sys_acquire(sys);
  if (r) { vslam_destroy(sys); return r; }
  *out = sys;
  return VSLAM_OK;
}

extern "C" int vslam_destroy(vslam_system* sys) {
  if (!sys) return VSLAM_OK;
  sys->own.release();
  ba_free(sys);
  delete sys;
  return VSLAM_OK;
}

extern "C" int vslam_synchronize(vslam_system* sys) {
  if (!sys) return VSLAM_E_INVALID;
  HIPCHK(hipStreamSynchronize(sys->stream));
  return ba_sync_streams(sys);
}

extern "C" int vslam_make_keyframe_lite(vslam_system* sys, const uint8_t* gray, size_t row_stride, size_t stream_stride,
                                        int on_device) {
  if (!sys) return VSLAM_E_INVALID;
  return fe_make_keyframe_lite(sys, gray, row_stride, stream_stride, on_device);
}

extern "C" int vslam_make_keyframe_lite_subset(vslam_system* sys, const int* streams, int n, const uint8_t* gray, size_t row_stride,
                                               size_t stream_stride, int on_device) {
  if (!sys) return VSLAM_E_INVALID;
  if (n < 0) { vslam_set_error("make_keyframe_lite_subset: n %d", n); return VSLAM_E_INVALID; }
  return fe_make_keyframe_lite(sys, gray, row_stride, stream_stride, on_device, streams, n);
}

extern "C" int vslam_get_step_streams(vslam_system* sys, unsigned char* in_step) {
  if (!sys || !in_step) { vslam_set_error("get_step_streams: null argument"); return VSLAM_E_INVALID; }
  memcpy(in_step, sys->step_in.data(), (size_t)sys->S);
  return VSLAM_OK;
}

extern "C" int vslam_fast_nonmax(vslam_system* sys) {
  if (!sys) return VSLAM_E_INVALID;
  return fe_fast_nonmax(sys);
}

static int check_sl(vslam_system* sys, int stream, int level) {
  if (!sys || stream < 0 || stream >= sys->S || level < 0 || level >= NLEV) { vslam_set_error("bad stream/level"); return VSLAM_E_INVALID; }
  if (!sys->have_frame) { vslam_set_error("no current frame"); return VSLAM_E_STATE; }
  return fe_stream_in_step(sys, stream, "front-end read-back");
}

static int check_overflow(vslam_system* sys) {
  int ov = 0;
  VCHK(host_get(sys->stream, &ov, sys->fr.overflow));
  if (ov) { vslam_set_error("corner capacity exceeded (raise vslam_params.max_corners)"); return VSLAM_E_CAPACITY; }
  return VSLAM_OK;
}

extern "C" int vslam_read_level_image(vslam_system* sys, int stream, int level, uint8_t* dst, size_t dst_stride) {
  int r = check_sl(sys, stream, level); if (r) return r;
  const LevelGeom& g = sys->geom[level];
  HostCopy c(sys->stream);
  VCHK(c.get2d(dst, dst_stride, sys->fr.img[level] + (size_t)stream * sys->fr.img_sstride[level], sys->fr.img_pitch[level], g.w, g.h));
  return c.wait();
}

extern "C" int vslam_read_corners(vslam_system* sys, int stream, int level, uint32_t* corners, int cap, int* n) {
  int r = check_sl(sys, stream, level); if (r) return r;
  r = check_overflow(sys); if (r) return r;
  return HostCopy(sys->stream).counted(sys->fr.ncorners + stream * NLEV + level, n, corners, sys->fr.corners[level] + (size_t)stream * sys->geom[level].cap, cap);
}

extern "C" int vslam_read_row_lut(vslam_system* sys, int stream, int level, int* lut) {
  int r = check_sl(sys, stream, level); if (r) return r;
  const int h = sys->geom[level].h;
  return host_get(sys->stream, lut, sys->fr.rowlut[level] + (size_t)stream * (h + 1), h);
}

extern "C" int vslam_read_sbi(vslam_system* sys, int stream, uint8_t* small_img, float* tmpl, double rot8[8]) {
  if (!sys || stream < 0 || stream >= sys->S) { vslam_set_error("bad stream/level"); return VSLAM_E_INVALID; }
  if (!sys->have_frame) { vslam_set_error("no current frame"); return VSLAM_E_STATE; }   // (a held stream's products are carried: no check_sl)
  if (!sys->p.use_sbi || !sys->have_sbi) { vslam_set_error("read_sbi: use_sbi is off or no frame yet"); return VSLAM_E_STATE; }
  const size_t ns = (size_t)(sys->geom[3].w / 2) * (sys->geom[3].h / 2);
  HostCopy c(sys->fe_stream);                  // the SmallBlurryImage is the front-end stream's product
  if (small_img) VCHK(c.get(small_img, sys->fr.sbi_small + stream * ns, ns));
  if (tmpl) VCHK(c.get(tmpl, sys->fr.sbi_tmpl + stream * ns, ns));
  if (rot8) VCHK(c.get(rot8, sys->fr.sbi_rot + (size_t)stream * 8, 8));
  return c.wait();
}

extern "C" int vslam_make_keyframe_rest(vslam_system* sys, double min_shi_tomasi_score) {
  if (!sys) return VSLAM_E_INVALID;
  return fe_make_keyframe_rest(sys, min_shi_tomasi_score);
}

extern "C" int vslam_thin_candidates(vslam_system* sys, int keyframe) {
  if (!sys) return VSLAM_E_INVALID;
  return fe_thin_candidates(sys, keyframe);
}

extern "C" int vslam_read_candidates(vslam_system* sys, int stream, int level, uint32_t* pos, double* score, int cap, int* n) {
  int r = check_sl(sys, stream, level); if (r) return r;
  if (!sys->have_candidates) { vslam_set_error("read_candidates: call vslam_make_keyframe_rest first"); return VSLAM_E_STATE; }
  int cnt = 0;
  HostCopy c(sys->stream);
  VCHK(c.get(&cnt, sys->ncand + stream * NLEV + level)); VCHK(c.wait());
  if (n) *n = cnt;
  const size_t off = (size_t)stream * sys->geom[level].cap;
  VCHK(c.take(pos, sys->cand[level] + off, cnt, cap));
  VCHK(c.take(score, sys->cand_score[level] + off, cnt, cap));
  return c.wait();
}

extern "C" int vslam_read_max_corners(vslam_system* sys, int stream, int level, uint32_t* corners, int* scores, int cap,
                                      int* n) {
  int r = check_sl(sys, stream, level); if (r) return r;
  int cnt = 0, nc = 0;
  HostCopy c(sys->stream);
  VCHK(c.get(&cnt, sys->fr.nmax + stream * NLEV + level)); VCHK(c.get(&nc, sys->fr.ncorners + stream * NLEV + level)); VCHK(c.wait());
  if (n) *n = cnt;
  const size_t off = (size_t)stream * sys->geom[level].cap;
  VCHK(c.take(corners, sys->fr.maxcorners[level] + off, cnt, cap));
  VCHK(c.take(scores, sys->fr.scores[level] + off, nc, cap));   // scores of ALL corners of the level (same order as vslam_read_corners)
  return c.wait();
}

// ---- self-test hook: the transcendentals of vslam_libm.h evaluated on the device ---------------------------------------
__global__ void k_eval_transcendental(int fn, int n, const double* x, double* y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double v = x[i];
  double r;
  switch (fn) {
    case 0: r = vlm::vsin(v); break;
    case 1: r = vlm::vcos(v); break;
    case 2: r = vlm::vtan(v); break;
    case 3: r = vlm::vatan(v); break;
    case 4: r = vlm::vasin(v); break;
    case 5: r = vlm::vacos(v); break;
    case 6: r = sqrt(v); break;
    default: r = 1.0 / v; break;
  }
  y[i] = r;
}

extern "C" int vslam_eval_transcendental(int fn, int n, const double* x, double* y, int on_host) {
  if (fn < 0 || fn > 7 || n < 0 || !x || !y) { vslam_set_error("eval_transcendental: bad argument"); return VSLAM_E_INVALID; }
  if (on_host) {                                      // the same source compiled for the host (what cam_fill and the oracle evaluate)
    for (int i = 0; i < n; i++) {
      const double v = x[i];
      y[i] = fn == 0 ? vlm::vsin(v) : fn == 1 ? vlm::vcos(v) : fn == 2 ? vlm::vtan(v) : fn == 3 ? vlm::vatan(v) : fn == 4 ? vlm::vasin(v)
           : fn == 5 ? vlm::vacos(v) : fn == 6 ? sqrt(v) : 1.0 / v;
    }
    return VSLAM_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { vslam_set_error("eval_transcendental: no HIP device visible"); return VSLAM_E_HIP; }
  if (n == 0) return VSLAM_OK;
  DevTemp<double> dx, dy;
  HIPCHK(dx.get(n));
  HIPCHK(dy.get(n));
  HIPCHK(hipMemcpy(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_eval_transcendental, dim3((n + 255) / 256), dim3(256), 0, 0, fn, n, (const double*)dx.p, dy.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(y, dy.p, sizeof(double) * n, hipMemcpyDeviceToHost));
  return VSLAM_OK;
}

// ---- self-test hook: the camera arithmetic every projecting kernel reads through CamModel ---------------------------------
// Per image-plane point 17 doubles: cam_project (im[2], r, factor, invalid), cam_derivs [4], cam_unproject(im) [2],
// unproject_with_derivs(im) (out[2], jac[4]).  One function for both sides.
#define CAM_EVAL_DOUBLES 17
HDFN void cam_eval_point(const CamModel& c, double x, double y, double* o) {
  const CamProj p = cam_project(c, x, y);
  o[0] = p.im[0]; o[1] = p.im[1]; o[2] = p.r; o[3] = p.factor; o[4] = p.invalid ? 1.0 : 0.0;
  double d[4], u[2], bo[2], bj[4];
  cam_derivs(c, p, d);
  cam_unproject(c, p.im[0], p.im[1], u);
  unproject_with_derivs(c, p.im[0], p.im[1], bo, bj);
  o[5] = d[0]; o[6] = d[1]; o[7] = d[2]; o[8] = d[3];
  o[9] = u[0]; o[10] = u[1]; o[11] = bo[0]; o[12] = bo[1];
  o[13] = bj[0]; o[14] = bj[1]; o[15] = bj[2]; o[16] = bj[3];
}

__global__ __launch_bounds__(64) void k_eval_camera(CamModel cam, int n, const double* xy, double* out) {
  for (int i = threadIdx.x; i < n; i += 64) {
    double o[CAM_EVAL_DOUBLES];
    cam_eval_point(cam, xy[2 * i], xy[2 * i + 1], o);
#pragma unroll
    for (int k = 0; k < CAM_EVAL_DOUBLES; k++) out[(size_t)CAM_EVAL_DOUBLES * i + k] = o[k];
  }
}

extern "C" int vslam_eval_camera(const double* cam5, int width, int height, int quirks, int n, const double* xy, double* out17, double* derived5,
                                 int on_host) {
  if (!cam5 || width < 1 || height < 1 || n < 0 || (n > 0 && (!xy || !out17)) || !derived5) { vslam_set_error("eval_camera: bad argument"); return VSLAM_E_INVALID; }
  vslam_params p;
  memset(&p, 0, sizeof(p));
  p.width = width; p.height = height; p.quirks = quirks;
  for (int k = 0; k < 5; k++) p.cam[k] = cam5[k];
  TrackParams tp;
  trk_fill_params(p, tp);                               // cam_fill and OnePixelDist as every handle takes them
  derived5[0] = tp.cam.two_tan; derived5[1] = tp.cam.winv; derived5[2] = tp.cam.largest_radius; derived5[3] = tp.cam.max_r; derived5[4] = tp.one_pixel_dist;
  if (on_host) {                                        // the same functions compiled for the host
    for (int i = 0; i < n; i++) cam_eval_point(tp.cam, xy[2 * i], xy[2 * i + 1], out17 + (size_t)CAM_EVAL_DOUBLES * i);
    return VSLAM_OK;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { vslam_set_error("eval_camera: no HIP device visible"); return VSLAM_E_HIP; }
  if (n == 0) return VSLAM_OK;
  DevTemp<double> d_xy, d_out;
  HIPCHK(d_xy.get((size_t)2 * n));
  HIPCHK(d_out.get((size_t)CAM_EVAL_DOUBLES * n));
  HostCopy c(nullptr);                                  // no handle: the null stream from start to end, through the copy primitive
  VCHK(c.put(d_xy.p, xy, (size_t)2 * n));
  hipLaunchKernelGGL(k_eval_camera, dim3(1), dim3(64), 0, 0, tp.cam, n, (const double*)d_xy.p, d_out.p);
  HIPCHK(hipGetLastError());
  VCHK(c.get(out17, (const double*)d_out.p, (size_t)CAM_EVAL_DOUBLES * n));
  return c.wait();
}

// ---- self-test hook: the line geometry of AddPointEpipolar and the triangulation, as k_epipolar runs them (grow_dev.h) ------
// One launch, one lane per case: first the n_lines epipolar_line cases, then the n_tri reproject_vector / reproject_point cases.
#define EPI_IN_DOUBLES 30
#define EPI_OUT_DOUBLES 12
#define TRI_IN_DOUBLES 16
#define TRI_OUT_DOUBLES 7
static DEVFN Pose pose_from12(const double* a) {
  Pose T;
  for (int i = 0; i < 9; i++) T.R[i] = a[i];
  for (int i = 0; i < 3; i++) T.t[i] = a[9 + i];
  return T;
}

__global__ __launch_bounds__(64) void k_eval_epipolar(CamModel cam, int n_lines, const double* lines, int* line_flags, double* line_out, int n_tri,
                                                       const double* tri, double* tri_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n_lines) {
    const double* in = lines + (size_t)EPI_IN_DOUBLES * i;
    const EpiLine e = epipolar_line(pose_from12(in), pose_from12(in + 12), cam, in[24], in[25], (int)in[26], in[27], in[28], in[29]);
    line_flags[2 * i] = e.why; line_flags[2 * i + 1] = e.clipped;
    double* o = line_out + (size_t)EPI_OUT_DOUBLES * i;
    o[0] = e.root[0]; o[1] = e.root[1]; o[2] = e.along[0]; o[3] = e.along[1]; o[4] = e.normal[0]; o[5] = e.normal[1];
    o[6] = e.dNormDist; o[7] = e.dMinLen; o[8] = e.dMaxLen; o[9] = e.startZ; o[10] = e.endZ; o[11] = e.alongSq;
  } else if (i - n_lines < n_tri) {
    const int j = i - n_lines;
    const double* in = tri + (size_t)TRI_IN_DOUBLES * j;
    const Pose T = pose_from12(in);
    double* o = tri_out + (size_t)TRI_OUT_DOUBLES * j;
    double v[4], p[3];
    reproject_vector(T, in + 12, in + 14, v);
    reproject_point(T, in + 12, in + 14, p);
    for (int k = 0; k < 4; k++) o[k] = v[k];
    for (int k = 0; k < 3; k++) o[4 + k] = p[k];
  }
}

extern "C" int vslam_eval_epipolar(vslam_system* sys, int n_lines, const double* lines30, int* line_flags2, double* line_out12, int n_tri,
                                   const double* tri16, double* tri_out7) {
  if (!sys || n_lines < 0 || n_tri < 0 || (n_lines > 0 && (!lines30 || !line_flags2 || !line_out12)) || (n_tri > 0 && (!tri16 || !tri_out7))) { vslam_set_error("eval_epipolar: bad argument"); return VSLAM_E_INVALID; }
  if (n_lines > 65536 || n_tri > 65536) { vslam_set_error("eval_epipolar: at most 65536 cases of a kind"); return VSLAM_E_CAPACITY; }
  for (int i = 0; i < n_lines; i++) {
    const double l = lines30[(size_t)EPI_IN_DOUBLES * i + 26];
    if (!(l == 0.0 || l == 1.0 || l == 2.0 || l == 3.0)) { vslam_set_error("eval_epipolar: case %d: level outside 0..%d", i, NLEV - 1); return VSLAM_E_INVALID; }
  }
  if (n_lines + n_tri == 0) return VSLAM_OK;
  DevTemp<double> d_in, d_out;
  DevTemp<int> d_flags;
  const size_t nin = (size_t)EPI_IN_DOUBLES * n_lines + (size_t)TRI_IN_DOUBLES * n_tri, nout = (size_t)EPI_OUT_DOUBLES * n_lines + (size_t)TRI_OUT_DOUBLES * n_tri;
  HIPCHK(d_in.get(nin));
  HIPCHK(d_out.get(nout));
  HIPCHK(d_flags.get((size_t)2 * (n_lines > 0 ? n_lines : 1)));
  hipStream_t q = sys->stream;
  HostCopy c(q);                                        // (behind the buffers: it waits before they are freed)
  VCHK(c.put(d_in.p, lines30, (size_t)EPI_IN_DOUBLES * n_lines));
  VCHK(c.put(d_in.p + (size_t)EPI_IN_DOUBLES * n_lines, tri16, (size_t)TRI_IN_DOUBLES * n_tri));
  hipLaunchKernelGGL(k_eval_epipolar, dim3((n_lines + n_tri + 63) / 64), dim3(64), 0, q, sys->tp.cam, n_lines, (const double*)d_in.p, d_flags.p, d_out.p, n_tri,
                     (const double*)(d_in.p + (size_t)EPI_IN_DOUBLES * n_lines), d_out.p + (size_t)EPI_OUT_DOUBLES * n_lines);
  HIPCHK(hipGetLastError());
  VCHK(c.get(line_flags2, (const int*)d_flags.p, (size_t)2 * n_lines));
  VCHK(c.get(line_out12, (const double*)d_out.p, (size_t)EPI_OUT_DOUBLES * n_lines));
  VCHK(c.get(tri_out7, (const double*)(d_out.p + (size_t)EPI_OUT_DOUBLES * n_lines), (size_t)TRI_OUT_DOUBLES * n_tri));
  return c.wait();
}

// ---- self-test hooks: the median's select and the tail of a pose iteration, each in one workgroup of its kernel's size ----
// The values are handed over as their producers do: the range of what can be selected is gathered while they are read (+inf
// marks an entry outside the median, as in the bundle adjustment's scratch) and published before the barrier in front of the select.
template <int THREADS, int BATCH, bool IN_LDS>
__global__ __launch_bounds__(THREADS) void k_eval_select(const double* v, int n, int k, double* out) {
  __shared__ __attribute__((aligned(16))) int hist[768];
  __shared__ unsigned long long sel[1];
  __shared__ unsigned mm[2 * (THREADS / 64)];
  __shared__ double buf[IN_LDS ? VSLAM_SELECT_LDS_CAP : 1];
  SelectRange sr = select_range_empty();
  for (int i = threadIdx.x; i < n; i += THREADS) {
    const double x = v[i];
    if (IN_LDS) buf[i] = x;
    select_range_add(sr, x, x != __builtin_huge_val());
  }
  block_select_publish(sr, hist, mm);
  __syncthreads();
  double r;
  if (IN_LDS) r = block_radix_select<BATCH>(buf, n, k, hist, sel, mm);
  else r = block_radix_select<BATCH>((const double __attribute__((address_space(1)))*)v, n, k, hist, sel, mm);
  if (threadIdx.x == 0) out[0] = r;
}

extern "C" int vslam_eval_select(int form, int n, const double* v, int k, double* out) {
  if (form < 0 || form > 1 || n < 1 || k < 0 || k >= n || !v || !out || (form == 0 && n > VSLAM_SELECT_LDS_CAP)) { vslam_set_error("eval_select: bad argument"); return VSLAM_E_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { vslam_set_error("eval_select: no HIP device visible"); return VSLAM_E_HIP; }
  DevTemp<double> dv, dr;
  HIPCHK(dv.get(n));
  HIPCHK(dr.get(1));
  HIPCHK(hipMemcpy(dv.p, v, sizeof(double) * n, hipMemcpyHostToDevice));
  if (form == 0) hipLaunchKernelGGL((k_eval_select<VSLAM_POSE_WG, RS_BATCH, true>), dim3(1), dim3(VSLAM_POSE_WG), 0, 0, (const double*)dv.p, n, k, dr.p);
  else if (n > 4096) hipLaunchKernelGGL((k_eval_select<VSLAM_BA_WG, 16, false>), dim3(1), dim3(VSLAM_BA_WG), 0, 0, (const double*)dv.p, n, k, dr.p);   // (ba_lm's switch)
  else hipLaunchKernelGGL((k_eval_select<VSLAM_BA_WG, 8, false>), dim3(1), dim3(VSLAM_BA_WG), 0, 0, (const double*)dv.p, n, k, dr.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dr.p, sizeof(double), hipMemcpyDeviceToHost));
  return VSLAM_OK;
}

__global__ __launch_bounds__(VSLAM_POSE_WG) void k_eval_pose_tail(const double* io_in, double* io_out) {   // in: 27 sums, pose12; out: update[6], pose12
  __shared__ Pose pose;
  __shared__ double up[6];
  if (threadIdx.x < 12) ((double*)&pose)[threadIdx.x] = io_in[27 + threadIdx.x];
  __syncthreads();
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0) {
    const int lane = threadIdx.x & 63;
    const double acc = lane < 27 ? io_in[lane] : 0.0;
    double mu[6];
    wave_pose_solve(acc, mu);
    wave_pose_apply(mu, (double*)&pose);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 6; r++) up[r] = mu[r];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) io_out[threadIdx.x] = up[threadIdx.x];
  if (threadIdx.x < 12) io_out[6 + threadIdx.x] = ((const double*)&pose)[threadIdx.x];
}

extern "C" int vslam_eval_pose_tail(const double* sums27, const double* pose12, double* update6, double* pose12_out) {
  if (!sums27 || !pose12 || !update6 || !pose12_out) { vslam_set_error("eval_pose_tail: bad argument"); return VSLAM_E_INVALID; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { vslam_set_error("eval_pose_tail: no HIP device visible"); return VSLAM_E_HIP; }
  DevTemp<double> din, dout;
  HIPCHK(din.get(39));
  HIPCHK(dout.get(18));
  double in[39], outv[18];
  memcpy(in, sums27, 27 * sizeof(double)); memcpy(in + 27, pose12, 12 * sizeof(double));
  HIPCHK(hipMemcpy(din.p, in, sizeof(in), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_eval_pose_tail, dim3(1), dim3(VSLAM_POSE_WG), 0, 0, (const double*)din.p, dout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(outv, dout.p, sizeof(outv), hipMemcpyDeviceToHost));
  memcpy(update6, outv, 6 * sizeof(double)); memcpy(pose12_out, outv + 6, 12 * sizeof(double));
  return VSLAM_OK;
}
