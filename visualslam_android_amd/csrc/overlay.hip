// The overlay renderer: what Tracker::TrackFrame draws on its colour frame (jni/Tracker.cc:580-588 the patches TrackMap found, as discs
// coloured by pyramid level; :322-336 the bootstrap trails, as lines; :148-155 drawFast's corner marks), into RGBA images, for any
// streams of a batch.  The raster rules are overlay_dev.h's; what is drawn for a stream is a pure function of the read-backs
// vslam_get_search_plan, vslam_get_point_tracks, vslam_get_trails, vslam_read_corners and vslam_read_level_image at the time of the
// call, which the kernel reads where they live on the device.
//
//   k_overlay   one workgroup per (image, band of rows).  The band holds one 32-bit key per pixel in LDS: the rank (overlay_dev.h) of
//               the topmost primitive there, 0 = the base image.  Scatter: lanes take the image's primitives (a mark or a disc per
//               lane, a line per wavefront), skip those whose rows miss the band, and raise the key of every covered pixel with an LDS
//               atomic max -- the rank is unique per primitive, so the result is the drawing order whatever order the lanes run in.
//               Resolve: every output pixel is written once and nothing is read back from the output; a lane takes four
//               neighbouring pixels (one dword of gray, four keys) and stores 16 bytes where the output allows it, single pixels at
//               a row's unaligned head and tail, bytes where a row is not even 4-byte aligned.  In-place mode stores only where the
//               key is not 0.  A pixel's colour is looked up from its key's primitive, not stored per pixel.
//   k_overlay_note   vslam_params.overlay = 1: one lane per stream, enqueued immediately before k_motion, records the mnFrame of the
//               frames in which TrackMap runs (after a frame TrackerState cannot tell: k_motion leaves a lost stream's counters and
//               iteration set as they were, and recovered_now is cleared at the frame's end).  Discs are drawn only if that is the
//               stream's latest frame.
#include "vslam_internal.h"
#include "overlay_dev.h"
#include <string.h>

#define OV_THREADS 256
#define OV_PLANE_WORDS 16384       // 64 KB of the CU's 160 KiB: 16 rows at 640 wide, 4 at 4096
#define OV_MAX_ROWS 16
#define OV_FLAGS_ALL (VSLAM_DRAW_POINTS | VSLAM_DRAW_TRAILS | VSLAM_DRAW_FAST | VSLAM_DRAW_IN_PLACE | VSLAM_DRAW_ALPHA0)

struct OvArgs {
  // output: image i at out + i * stream_stride, rows row_stride bytes apart
  uint8_t* out; size_t row_stride, stream_stride;
  int W, H, rows, bands, flags;
  // base (not read in place): level 0 of image i's stream
  const uint8_t* gray; size_t gray_sstride, gray_pitch;
  const int* list;                 // image -> stream; null: the identity
  // the tracker's lists (k_overlay<false>)
  const TrackerState* st; const int* ran; const int* iter_list; const int* pt_flags; const int* pt_level; const TrackData* td;
  const int* trail_pos; const uint32_t* corners; const int* ncorners;
  int max_points, corner_cap;
  int* info;                       // [S][3] discs, lines, marks of the stream's last render
  // the caller's primitives (k_overlay<true>)
  const int* marks; const int* lines; const int* discs;
  int nm, nl, nd;
};

// The primitives of one image: counts, and each primitive by list position
template <bool EXPLICIT> struct OvSrc;
template <> struct OvSrc<true> {
  const OvArgs& a; int nm, nl, nd;
  __device__ OvSrc(const OvArgs& args, int) : a(args), nm(args.nm), nl(args.nl), nd(args.nd) {}
  DEVFN void mark(int i, int* x, int* y) const { *x = a.marks[2 * i]; *y = a.marks[2 * i + 1]; }
  DEVFN void line(int i, int* p) const { for (int k = 0; k < 4; k++) p[k] = a.lines[4 * i + k]; }
  DEVFN bool disc(int j, int* x, int* y) const { *x = a.discs[3 * j]; *y = a.discs[3 * j + 1]; return true; }
  DEVFN int disc_level(int j) const { return a.discs[3 * j + 2]; }
};
template <> struct OvSrc<false> {
  const OvArgs& a; int s, nm, nl, nd;
  const int* iter; const int* fl; const int* lv; const TrackData* td; const int* trail; const uint32_t* cor;
  __device__ OvSrc(const OvArgs& args, int stream) : a(args), s(stream) {
    const TrackerState* st = a.st + s;
    const size_t P = (size_t)a.max_points;
    iter = a.iter_list + s * P; fl = a.pt_flags + s * P; lv = a.pt_level + s * P; td = a.td + s * P;
    cor = a.corners + (size_t)s * a.corner_cap;
    nm = 0; nl = 0; nd = 0;
    if (a.flags & VSLAM_DRAW_FAST) nm = min(max(a.ncorners[s * NLEV], 0), a.corner_cap);
    trail = nullptr;
    if ((a.flags & VSLAM_DRAW_TRAILS) && a.trail_pos && st->init_stage == 1) {
      nl = min(max(st->n_trails, 0), BOOT_MAX_TRAILS);
      trail = a.trail_pos + ((size_t)s * 2 + (st->trail_buf & 1)) * BOOT_MAX_TRAILS * 4;
    }
    if ((a.flags & VSLAM_DRAW_POINTS) && a.ran[s] >= 0 && a.ran[s] == st->frame) nd = min(max(st->n_iter, 0), a.max_points);
  }
  DEVFN void mark(int i, int* x, int* y) const { const uint32_t c = cor[i]; *x = (int)(c & 0xFFFFu); *y = (int)(c >> 16); }
  DEVFN void line(int i, int* p) const { for (int k = 0; k < 4; k++) p[k] = trail[4 * i + k]; }
  // entry j of the iteration set: drawn if its point was found; the centre is v2Image truncated (cv::Point(double, double))
  DEVFN bool disc(int j, int* x, int* y) const {
    const int pi = iter[j];
    if (pi < 0 || pi >= a.max_points || !(fl[pi] & TDF_FOUND)) return false;
    const double u = td[pi].image[0], v = td[pi].image[1];
    if (!(u > -(double)OV_COORD_MAX && u < (double)OV_COORD_MAX && v > -(double)OV_COORD_MAX && v < (double)OV_COORD_MAX)) { *x = OV_COORD_MAX + 1; *y = 0; return true; }
    *x = (int)u; *y = (int)v;
    return true;
  }
  DEVFN int disc_level(int j) const { const int pi = iter[j]; return pi >= 0 && pi < a.max_points ? lv[pi] : 0; }
};

DEVFN void ov_put(uint32_t* plane, int W, int r0, int r1, int x, int y, uint32_t rank) {
  if ((unsigned)x < (unsigned)W && y >= r0 && y < r1) atomicMax(&plane[(y - r0) * W + x], rank);
}

template <bool EXPLICIT>
DEVFN uint32_t ov_key_colour(const OvSrc<EXPLICIT>& src, uint32_t key, bool alpha0) {
  int idx;
  const int kind = ov_rank_kind(key, src.nm, src.nl, src.nd, &idx);
  const int cls = kind == 0 ? OV_MARK : kind == 1 ? OV_TRAIL : (src.disc_level(idx) & 3);
  return ov_colour(cls, alpha0);
}

DEVFN void ov_store_bytes(uint8_t* p, uint32_t c) { p[0] = (uint8_t)c; p[1] = (uint8_t)(c >> 8); p[2] = (uint8_t)(c >> 16); p[3] = (uint8_t)(c >> 24); }

template <bool EXPLICIT>
__global__ __launch_bounds__(OV_THREADS) void k_overlay(OvArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t plane[];
  const int img = blockIdx.x / a.bands, band = blockIdx.x - img * a.bands;
  const int s = a.list ? a.list[img] : img;
  const int W = a.W, r0 = band * a.rows, r1 = min(r0 + a.rows, a.H), nr = r1 - r0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool alpha0 = (a.flags & VSLAM_DRAW_ALPHA0) != 0;
  const OvSrc<EXPLICIT> src(a, s);
  for (int k = tid; k < nr * W; k += OV_THREADS) plane[k] = 0u;
  // band 0 keeps the stream's counts (the whole plane is the workgroup's LDS, so the disc count is summed in the record itself)
  int* const counts = a.info + 3 * (size_t)s;
  if (!EXPLICIT && band == 0 && tid == 0) { atomicExch(&counts[0], 0); counts[1] = src.nl; counts[2] = src.nm; }
  __syncthreads();

  // ---- scatter ----
  for (int i = tid; i < src.nm; i += OV_THREADS) {
    int x, y;
    src.mark(i, &x, &y);
    if (!ov_coord_ok(x) || !ov_coord_ok(y) || y + 1 < r0 || y - 1 >= r1) continue;
    const uint32_t rank = ov_rank_mark(i);
#pragma unroll
    for (int k = 0; k < OV_MARK_PIXELS; k++) { int dx, dy; ov_mark_pixel(k, &dx, &dy); ov_put(plane, W, r0, r1, x + dx, y + dy, rank); }
  }
  for (int i = wave; i < src.nl; i += OV_THREADS / 64) {
    int p[4];
    src.line(i, p);
    if (!ov_coord_ok(p[0]) || !ov_coord_ok(p[1]) || !ov_coord_ok(p[2]) || !ov_coord_ok(p[3])) continue;
    if (max(p[1], p[3]) < r0 || min(p[1], p[3]) >= r1) continue;
    const OvLine L = ov_line_setup(p[0], p[1], p[2], p[3]);
    // the stretch of the line that can touch the band: along the major axis the pixel index is the coordinate's offset
    int lo = 0, hi = L.a;
    if (L.ymajor) {
      if (L.sy > 0) { lo = max(lo, r0 - L.y0); hi = min(hi, r1 - 1 - L.y0); }
      else { lo = max(lo, L.y0 - (r1 - 1)); hi = min(hi, L.y0 - r0); }
    } else { lo = max(lo, -L.x0); hi = min(hi, W - 1 - L.x0); }
    const uint32_t rank = ov_rank_line(src.nm, i);
    for (int k = lo + lane; k <= hi; k += 64) { int x, y; ov_line_pixel(L, k, &x, &y); ov_put(plane, W, r0, r1, x, y, rank); }
  }
  int mine = 0;
  for (int j = tid; j < src.nd; j += OV_THREADS) {
    int x, y;
    if (!src.disc(j, &x, &y)) continue;
    mine++;
    if (!ov_coord_ok(x) || !ov_coord_ok(y) || y + OV_DISC_R < r0 || y - OV_DISC_R >= r1) continue;
    const uint32_t rank = ov_rank_disc(src.nm, src.nl, src.nd, j);
    for (int dy = -OV_DISC_R; dy <= OV_DISC_R; dy++) {
      const int h = ov_disc_half_width(dy);
      for (int dx = -h; dx <= h; dx++) ov_put(plane, W, r0, r1, x + dx, y + dy, rank);
    }
  }
  if (!EXPLICIT && band == 0 && mine) atomicAdd(&counts[0], mine);
  __syncthreads();

  // ---- resolve: wavefront w takes the rows w, w + 4, ... of the band ----
  uint8_t* const obase = a.out + (size_t)img * a.stream_stride;
  for (int r = wave; r < nr; r += OV_THREADS / 64) {
    const int y = r0 + r;
    uint8_t* const orow = obase + (size_t)y * a.row_stride;
    const uint32_t* const krow = plane + r * W;
    const bool dword_ok = ((uintptr_t)orow & 3) == 0;
    if (a.flags & VSLAM_DRAW_IN_PLACE) {
      for (int x = lane; x < W; x += 64) {
        const uint32_t key = krow[x];
        if (!key) continue;
        const uint32_t c = ov_key_colour(src, key, alpha0);
        if (dword_ok) *(uint32_t*)(orow + 4 * (size_t)x) = c; else ov_store_bytes(orow + 4 * (size_t)x, c);
      }
      continue;
    }
    const uint8_t* const grow = a.gray + (size_t)s * a.gray_sstride + (size_t)y * a.gray_pitch;
    if (!dword_ok) {                                                     // a row that is not 4-byte aligned: bytes
      for (int x = lane; x < W; x += 64) {
        const uint32_t key = krow[x];
        ov_store_bytes(orow + 4 * (size_t)x, key ? ov_key_colour(src, key, alpha0) : ov_gray(grow[x]));
      }
      continue;
    }
    const int head = min(W, (int)(((16u - ((uintptr_t)orow & 15u)) & 15u) >> 2));   // single pixels up to the first 16-byte boundary
    const int ngroups = (W - head) >> 2, tail0 = head + 4 * ngroups;
    for (int t = lane; t < ngroups; t += 64) {
      const int x = head + 4 * t;
      uint32_t g4;
      if (((uintptr_t)(grow + x) & 3) == 0) g4 = *(const uint32_t*)(grow + x);
      else g4 = (uint32_t)grow[x] | ((uint32_t)grow[x + 1] << 8) | ((uint32_t)grow[x + 2] << 16) | ((uint32_t)grow[x + 3] << 24);
      uint32_t c[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t key = krow[x + k];
        c[k] = key ? ov_key_colour(src, key, alpha0) : ov_gray((g4 >> (8 * k)) & 0xFFu);
      }
      *(uint4*)(orow + 4 * (size_t)x) = make_uint4(c[0], c[1], c[2], c[3]);
    }
    for (int t = lane; t < head + (W - tail0); t += 64) {
      const int x = t < head ? t : tail0 + (t - head);
      const uint32_t key = krow[x];
      *(uint32_t*)(orow + 4 * (size_t)x) = key ? ov_key_colour(src, key, alpha0) : ov_gray(grow[x]);
    }
  }
}

static int ov_band_rows(int W) { int r = OV_MAX_ROWS; while (r > 1 && r * W > OV_PLANE_WORDS) r >>= 1; return r; }

template <bool EXPLICIT>
static int ov_launch(OvArgs& a, int n_images, hipStream_t q) {
  a.rows = ov_band_rows(a.W);
  a.bands = (a.H + a.rows - 1) / a.rows;
  const size_t lds = (size_t)a.rows * a.W * sizeof(uint32_t);
  if (n_images < 1) return VSLAM_OK;
  if (lds > OV_PLANE_WORDS * sizeof(uint32_t)) { vslam_set_error("overlay: width %d does not fit the key plane", a.W); return VSLAM_E_INVALID; }
  hipLaunchKernelGGL(k_overlay<EXPLICIT>, dim3((unsigned)a.bands * (unsigned)n_images), dim3(OV_THREADS), lds, q, a);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

// ---- vslam_params.overlay: the record of the frames in which TrackMap ran --------------------------------------------------------
__global__ __launch_bounds__(64) void k_overlay_note(MapDev m, int S, int* ran) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const TrackerState* st = &m.st[s];
  if (trk_runs_track_map(m.held, s, st)) ran[s] = st->frame + 1;     // k_motion, the next launch, makes this the stream's mnFrame (jni/Tracker.cc:100)
}

// the streams a retirement lists: not_listed marks the others in req
__global__ __launch_bounds__(64) void k_overlay_forget(int* ran, int S, const int* req, int not_listed) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s < S && req[s] != not_listed) ran[s] = -1;
}

int overlay_alloc(vslam_system* sys) {
  if (!sys->p.overlay) return VSLAM_OK;
  DevOwner& own = sys->own;
  const size_t S = (size_t)sys->S;
  VCHK(own.alloc(&sys->overlay_ran, S, sys->stream));
  HIPCHK(hipMemsetAsync(sys->overlay_ran, 0xFF, S * sizeof(int), sys->stream));   // -1: TrackMap has never run
  VCHK(own.alloc(&sys->overlay_info, S * 3, sys->stream));
  VCHK(own.alloc(&sys->overlay_list, S, sys->stream));
  for (int k = 0; k < 2; k++) VCHK(own.event(&sys->ev_overlay_t[k], true));
  return VSLAM_OK;
}

int overlay_note_track_map(vslam_system* sys) {
  if (!sys->overlay_ran) return VSLAM_OK;
  hipLaunchKernelGGL(k_overlay_note, dim3((sys->S + 63) / 64), dim3(64), 0, sys->stream, sys->map, sys->S, sys->overlay_ran);
  return VSLAM_OK;
}

int overlay_forget_listed(vslam_system* sys, const int* d_req, int not_listed) {
  if (!sys->overlay_ran) return VSLAM_OK;
  hipLaunchKernelGGL(k_overlay_forget, dim3((sys->S + 63) / 64), dim3(64), 0, sys->stream, sys->overlay_ran, sys->S, d_req, not_listed);
  HIPCHK(hipGetLastError());
  return VSLAM_OK;
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------
extern "C" int vslam_render_overlay(vslam_system* sys, const int* streams, int n, uint8_t* rgba, size_t row_stride, size_t stream_stride,
                                    int on_device, int flags) {
  if (!sys) { vslam_set_error("render_overlay: null system"); return VSLAM_E_INVALID; }
  const int S = sys->S, W = sys->p.width, H = sys->p.height;
  if (!streams) n = S;                                                  // every stream, image s = stream s
  if (n < 0 || n > S) { vslam_set_error("render_overlay: n %d of %d streams", n, S); return VSLAM_E_INVALID; }
  if (flags & ~OV_FLAGS_ALL) { vslam_set_error("render_overlay: unknown flag bits 0x%x", flags & ~OV_FLAGS_ALL); return VSLAM_E_INVALID; }
  if (streams) {
    std::vector<unsigned char> seen((size_t)S, 0);
    for (int i = 0; i < n; i++) {
      if (streams[i] < 0 || streams[i] >= S) { vslam_set_error("render_overlay: stream %d of %d (entry %d)", streams[i], S, i); return VSLAM_E_INVALID; }
      if (seen[(size_t)streams[i]]) { vslam_set_error("render_overlay: stream %d is listed twice", streams[i]); return VSLAM_E_INVALID; }
      seen[(size_t)streams[i]] = 1;
    }
  }
  if (n > 0 && !rgba) { vslam_set_error("render_overlay: null image"); return VSLAM_E_INVALID; }
  if (row_stride < 4 * (size_t)W) { vslam_set_error("render_overlay: row_stride %zu below 4 * width", row_stride); return VSLAM_E_INVALID; }
  if (n > 1 && stream_stride < row_stride * (size_t)H) { vslam_set_error("render_overlay: stream_stride %zu below row_stride * height", stream_stride); return VSLAM_E_INVALID; }
  if (!sys->overlay_ran) { vslam_set_error("render_overlay: created with overlay = 0"); return VSLAM_E_STATE; }
  if (!sys->have_frame) { vslam_set_error("render_overlay: no current frame"); return VSLAM_E_STATE; }
  if (sys->frame_open && !sys->frame_tracked) { vslam_set_error("render_overlay: a frame is open and its tracking has not finished (vslam_pose_update(sys, 1) first)"); return VSLAM_E_STATE; }
  for (int i = 0; i < n; i++) VCHK(fe_stream_in_step(sys, streams ? streams[i] : i, "render_overlay"));
  if (n == 0) return VSLAM_OK;

  OvArgs a = {};
  a.W = W; a.H = H; a.flags = flags;
  a.gray = sys->fr.img[0]; a.gray_sstride = sys->fr.img_sstride[0]; a.gray_pitch = (size_t)sys->fr.img_pitch[0];
  const MapDev& m = sys->map;
  a.st = m.st; a.ran = sys->overlay_ran; a.iter_list = m.iter_list; a.pt_flags = m.pt_flags; a.pt_level = m.pt_level; a.td = m.td;
  a.trail_pos = m.trail_pos; a.corners = sys->fr.corners[0]; a.ncorners = sys->fr.ncorners;
  a.max_points = sys->p.max_points; a.corner_cap = sys->geom[0].cap;
  a.info = sys->overlay_info;
  hipStream_t q = sys->stream;
  DevTemp<uint8_t> tmp;                                                 // host output: the images on the device (behind it, the batch that copies them)
  HostCopy c(q);
  if (streams) {                                                        // the one wait of a call with a list: its upload
    VCHK(c.put(sys->overlay_list, streams, (size_t)n)); VCHK(c.wait());
    a.list = sys->overlay_list;
  }
  if (on_device) { a.out = rgba; a.row_stride = row_stride; a.stream_stride = stream_stride; }
  else {                                                                // host memory: rows as far apart as the caller's, images packed
    a.row_stride = row_stride; a.stream_stride = row_stride * (size_t)H;
    HIPCHK(tmp.get(a.stream_stride * (size_t)n));
    a.out = tmp.p;
    if (flags & VSLAM_DRAW_IN_PLACE)
      for (int i = 0; i < n; i++) VCHK(c.put2d(tmp.p + (size_t)i * a.stream_stride, row_stride, rgba + (size_t)i * stream_stride, row_stride, 4 * (size_t)W, (size_t)H));
  }
  HIPCHK(hipEventRecord(sys->ev_overlay_t[0], q));
  VCHK(ov_launch<false>(a, n, q));
  HIPCHK(hipEventRecord(sys->ev_overlay_t[1], q));
  sys->overlay_calls++;
  // the front end may rebuild this buffer's products only behind the render that reads them (a frame that is still open records at its end)
  if (!sys->frame_open) HIPCHK(hipEventRecord(sys->ev_track_done[sys->fr_idx], q));
  if (!on_device) {
    for (int i = 0; i < n; i++) VCHK(c.get2d(rgba + (size_t)i * stream_stride, row_stride, tmp.p + (size_t)i * a.stream_stride, row_stride, 4 * (size_t)W, (size_t)H));
    VCHK(c.wait());
  }
  return VSLAM_OK;
}

extern "C" int vslam_get_overlay_info(vslam_system* sys, int stream, int out[4]) {
  if (!sys || stream < 0 || stream >= sys->S || !out) { vslam_set_error("get_overlay_info: bad argument"); return VSLAM_E_INVALID; }
  if (!sys->overlay_ran) { vslam_set_error("get_overlay_info: created with overlay = 0"); return VSLAM_E_STATE; }
  HostCopy c(sys->stream);
  VCHK(c.get(out, sys->overlay_ran + stream)); VCHK(c.get(out + 1, sys->overlay_info + 3 * (size_t)stream, 3));
  return c.wait();
}

extern "C" int vslam_get_render_timing(vslam_system* sys, double* ms) {
  if (!sys || !ms) { vslam_set_error("get_render_timing: bad argument"); return VSLAM_E_INVALID; }
  if (!sys->overlay_ran || sys->overlay_calls == 0) { vslam_set_error("get_render_timing: no vslam_render_overlay call yet"); return VSLAM_E_STATE; }
  HIPCHK(hipEventSynchronize(sys->ev_overlay_t[1]));
  float t = 0.f;
  HIPCHK(hipEventElapsedTime(&t, sys->ev_overlay_t[0], sys->ev_overlay_t[1]));
  *ms = t;
  return VSLAM_OK;
}

// Self-test hook, no system: the same kernel over the caller's primitives, one image in host memory, on the null stream.
extern "C" int vslam_eval_overlay(int width, int height, const uint8_t* gray, size_t gray_stride, int n_marks, const int* marks_xy, int n_lines,
                                  const int* lines_xyxy, int n_discs, const int* discs_xy_level, uint8_t* rgba, size_t row_stride, int flags) {
  const bool in_place = (flags & VSLAM_DRAW_IN_PLACE) != 0;
  if (width < 1 || height < 1 || width > 4096 || height > 4096 || n_marks < 0 || n_lines < 0 || n_discs < 0 || (n_marks && !marks_xy) || (n_lines && !lines_xyxy) ||
      (n_discs && !discs_xy_level) || !rgba || row_stride < 4 * (size_t)width || (!in_place && (!gray || gray_stride < (size_t)width)) ||
      (flags & ~(VSLAM_DRAW_IN_PLACE | VSLAM_DRAW_ALPHA0)) || (long long)n_marks + n_lines + n_discs > 0x7FFFFFF0ll) {
    vslam_set_error("eval_overlay: bad argument (size 1..4096, flags IN_PLACE / ALPHA0 only)"); return VSLAM_E_INVALID;
  }
  for (int i = 0; i < 2 * n_marks; i++) if (!ov_coord_ok(marks_xy[i])) { vslam_set_error("eval_overlay: a coordinate beyond +-%d", OV_COORD_MAX); return VSLAM_E_INVALID; }
  for (int i = 0; i < 4 * n_lines; i++) if (!ov_coord_ok(lines_xyxy[i])) { vslam_set_error("eval_overlay: a coordinate beyond +-%d", OV_COORD_MAX); return VSLAM_E_INVALID; }
  for (int i = 0; i < n_discs; i++)
    if (!ov_coord_ok(discs_xy_level[3 * i]) || !ov_coord_ok(discs_xy_level[3 * i + 1]) || discs_xy_level[3 * i + 2] < 0 || discs_xy_level[3 * i + 2] >= NLEV) {
      vslam_set_error("eval_overlay: disc %d: a coordinate beyond +-%d or a level outside 0..3", i, OV_COORD_MAX); return VSLAM_E_INVALID;
    }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { vslam_set_error("eval_overlay: no HIP device visible"); return VSLAM_E_HIP; }
  const size_t W = (size_t)width, H = (size_t)height, out_bytes = row_stride * (H - 1) + 4 * W;
  DevTemp<uint8_t> dout, dgray; DevTemp<int> dprim;
  HIPCHK(dout.get(out_bytes));
  if (!in_place) HIPCHK(dgray.get(W * H));
  const size_t np = 2 * (size_t)n_marks + 4 * (size_t)n_lines + 3 * (size_t)n_discs;
  HIPCHK(dprim.get(np ? np : 1));
  OvArgs a = {};
  a.W = width; a.H = height; a.flags = flags;
  a.out = dout.p; a.row_stride = row_stride; a.stream_stride = 0;
  a.gray = dgray.p; a.gray_sstride = 0; a.gray_pitch = W;
  a.nm = n_marks; a.nl = n_lines; a.nd = n_discs;
  int* pm = dprim.p; int* pl = pm + 2 * (size_t)n_marks; int* pd = pl + 4 * (size_t)n_lines;
  a.marks = pm; a.lines = pl; a.discs = pd;
  HostCopy c(nullptr);
  VCHK(c.put(pm, marks_xy, 2 * (size_t)n_marks)); VCHK(c.put(pl, lines_xyxy, 4 * (size_t)n_lines)); VCHK(c.put(pd, discs_xy_level, 3 * (size_t)n_discs));
  if (in_place) VCHK(c.put2d(dout.p, row_stride, rgba, row_stride, 4 * W, H));
  else VCHK(c.put2d(dgray.p, W, gray, gray_stride, W, H));
  VCHK(ov_launch<true>(a, 1, nullptr));
  VCHK(c.get2d(rgba, row_stride, dout.p, row_stride, 4 * W, H));
  return c.wait();
}
