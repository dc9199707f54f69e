// Stream snapshots: one stream of a live batch packed into a blob (csrc/snapshot_format.h) and a blob unpacked into any slot of any
// compatible system.  The reference persists a map only as MapMaker::GUICommandHandler("SaveMap")'s text dump (jni/MapMaker.cc:1254-1286,
// vslam_save_map); this carries the Map (jni/Map.h:21-34) and the per-stream members of Tracker and MapMaker bit for bit, so that the
// restored stream's next frame is the source stream's next frame.
//
// reset.hip says what a stream's state is; the list here is that list with the arrays a reset may leave stale because a count bounds
// them (MapPointDev, the failure queue, keyframe images) added, since a snapshot has to carry them:
//   carried   TrackerState; MapPointDev, TrackData, templates, pt_flags, pt_level, cur_meas [n_points]; kf_meas [n_kf][n_points];
//             kf_pose, kf_fixed, kf_depth, the four pyramid levels [n_kf]; iter_list [n_iter] (vslam_get_search_plan);
//             never_retry [n_points] and the failure queue [fq_n] (idle jobs); the last frame's SmallBlurryImage (use_sbi);
//             RelocInfo, the last attempt's frame template and scores [n_kf] (relocalise)
//   remade    keyframe corner lists (fe_keyframe_corners) and keyframe SmallBlurryImages (reloc_keyframe_sbi), from the restored pyramids
//             through the map upload's own path: FAST and the SmallBlurryImage are pure functions of the stored images, the read-backs come
//             out equal, and a blob of a system without grow_map / relocalise restores into one with it
//   not       the frame's front-end products, reset_info, retire_info, profile and timing records, the bundle-adjustment pool record (every
//             adjustment rewrites it from the map before it reads it: k_ba_select, k_ba_assemble)
//
// One kernel moves the bytes in both directions, driven by a table of copies passed by value: a section of the blob is `rows` dense
// rows, the device side of it `rows` rows dev_stride apart.  The planner (snap_plan) is the same for pack and unpack; only the system
// whose pointers and strides enter differs.
#include "vslam_internal.h"
#include "snapshot_format.h"
#include <stddef.h>
#include <stdio.h>
#include <string.h>

static_assert(sizeof(TrackerState) == SNAP_STATE_BYTES && sizeof(MapPointDev) == SNAP_POS_BYTES + SNAP_POINT_REST_BYTES && offsetof(MapPointDev, pos) == 0 &&
              sizeof(TrackData) == SNAP_TRACKDATA_BYTES && TMPL_PITCH == SNAP_TMPL_BYTES && sizeof(MeasDev) == SNAP_MEAS_BYTES &&
              sizeof(Pose) == SNAP_POSE_BYTES && sizeof(RelocInfo) == SNAP_RELOC_INFO_BYTES && NLEV == SNAP_LEVELS && sizeof(int2) == 8,
              "snapshot_format.h states the sizes of the carried structs: a change of one of them is a new SNAP_VERSION");

#define SNAP_THREADS 256
#define SNAP_CHUNK 4096          // bytes of a row one team moves at a time: 64 lanes x 4 x 16 bytes
#define SNAP_MAX_BLOCKS 1024
#define SNAP_BYTES_PER_BLOCK 16384

struct SnapCopy { uint8_t* dev; unsigned long long blob_off, rows, row_bytes, dev_stride; };
struct SnapPlan { SnapCopy c[SNAP_N_SECTIONS]; };

// n bytes by a team of T lanes in words of V, where d and s are congruent modulo sizeof(V): the bytes before d's first aligned word
// and after its last one singly, consecutive lanes on consecutive words in between
template <class V>
DEVFN void copy_span_as(uint8_t* d, const uint8_t* s, size_t n, unsigned lane, unsigned T) {
  size_t head = (size_t)(0 - (uintptr_t)d) & (sizeof(V) - 1);
  if (head > n) head = n;
  const size_t body = (n - head) / sizeof(V), done = head + body * sizeof(V);
  for (size_t i = lane; i < head; i += T) d[i] = s[i];
  V* dv = (V*)(d + head); const V* sv = (const V*)(s + head);
  for (size_t i = lane; i < body; i += T) dv[i] = sv[i];
  for (size_t i = done + lane; i < n; i += T) d[i] = s[i];
}
// ... in the widest words both sides allow: 16 bytes wherever they are aligned alike (every section of a 640 x 480 stream but the
// re-strided point and measurement rows), else 8, 4 or single bytes (image rows of odd width, odd point counts)
DEVFN void copy_span(uint8_t* d, const uint8_t* s, size_t n, unsigned lane, unsigned T) {
  const unsigned diff = (unsigned)((uintptr_t)d - (uintptr_t)s) & 15u;
  if (diff == 0) copy_span_as<uint4>(d, s, n, lane, T);
  else if ((diff & 7u) == 0) copy_span_as<uint2>(d, s, n, lane, T);
  else if ((diff & 3u) == 0) copy_span_as<uint32_t>(d, s, n, lane, T);
  else copy_span_as<uint8_t>(d, s, n, lane, T);
}

// The workgroups of the grid share every section (as k_reset_clear's share every array).  A row is cut into chunks of SNAP_CHUNK bytes
// and a (row, chunk) goes to a team of T lanes: a whole wavefront for rows of 1 KiB and more, the power of two that covers the row in
// 16-byte words below that, so that the 80-byte rows of a level-3 image or the 24-byte position of a map point do not idle 59 lanes.
// PACK writes the zero bytes between a section's end and the next multiple of 16 as well.
template <bool PACK>
__global__ __launch_bounds__(SNAP_THREADS) void k_snapshot(SnapPlan plan, uint8_t* blob) {
  const size_t tid = (size_t)blockIdx.x * SNAP_THREADS + threadIdx.x, nth = (size_t)gridDim.x * SNAP_THREADS;
  for (int i = 0; i < SNAP_N_SECTIONS; i++) {
    const SnapCopy c = plan.c[i];
    if (c.rows == 0) continue;
    const size_t words = (c.row_bytes + 15) / 16;
    unsigned T = 1;
    while (T < 64 && T < words) T <<= 1;
    const size_t chunks = (c.row_bytes + SNAP_CHUNK - 1) / SNAP_CHUNK, items = c.rows * chunks;
    const size_t team = tid / T, nteams = nth / T;
    const unsigned lane = (unsigned)(tid % T);
    for (size_t it = team; it < items; it += nteams) {
      const size_t r = it / chunks, o = (it - r * chunks) * SNAP_CHUNK;
      size_t n = c.row_bytes - o;
      if (n > SNAP_CHUNK) n = SNAP_CHUNK;
      uint8_t* b = blob + c.blob_off + r * c.row_bytes + o;
      uint8_t* d = c.dev + r * c.dev_stride + o;
      if (PACK) copy_span(b, d, n, lane, T); else copy_span(d, b, n, lane, T);
    }
    if (PACK) {
      const size_t end = c.blob_off + c.rows * c.row_bytes, pad = snap_align16(end) - end;
      if (tid < pad) blob[end + tid] = 0;
    }
  }
}

// The failure queue is filled through an atomic counter by the lanes of k_ba_writeback, so the order of its entries in memory is an
// accident of scheduling and no part of the state: every reader treats it as a set (k_refind_idle; the reference sorts mvFailureQueue
// before it uses it, jni/MapMaker.cc:1083-1096).  The blob holds it sorted by (keyframe, point), so that equal states give equal bytes:
// each lane ranks its entry among the n and stores it there (n <= fq_cap = 8192), and the eight bytes after an odd count are zeroed.
__global__ __launch_bounds__(SNAP_THREADS) void k_pack_failure_queue(const int2* fq, int n, int2* out) {
  const int i = blockIdx.x * SNAP_THREADS + threadIdx.x;
  if (i == 0 && (n & 1)) out[n] = make_int2(0, 0);
  if (i >= n) return;
  const int2 e = fq[i];
  const unsigned long long key = ((unsigned long long)(unsigned)e.x << 32) | (unsigned)e.y;
  int rank = 0;
  for (int j = 0; j < n; j++) {
    const int2 f = fq[j];
    const unsigned long long kj = ((unsigned long long)(unsigned)f.x << 32) | (unsigned)f.y;
    rank += (kj < key || (kj == key && j < i)) ? 1 : 0;
  }
  out[rank] = e;
}

// ---- host side ------------------------------------------------------------------------------------------------------
int snapshot_alloc(vslam_system* sys) {
  for (int k = 0; k < 4; k++) VCHK(sys->own.event(&sys->ev_snap_t[k], true));
  return VSLAM_OK;
}

static size_t small_pixels(const vslam_system* sys) { return (size_t)(sys->geom[3].w / 2) * (sys->geom[3].h / 2); }

// The copies between a blob with these counts and stream s of this system.  A section of a part the system does not keep moves nothing.
// Rows that lie back to back on the device as they do in the blob become one row (levels 0 and 1 of a 640 x 480 pyramid, every
// per-point array but the two halves of MapPointDev).
static void snap_plan(const vslam_system* sys, int s, const SnapCounts& c, const SnapTable& t, SnapPlan& plan) {
  const MapDev& m = sys->map;
  const size_t P = sys->p.max_points, K = sys->p.max_keyframes, N = small_pixels(sys);
  for (int i = 0; i < SNAP_N_SECTIONS; i++) {
    const SnapRows r = snap_section_rows(c, i);
    uint8_t* dev = nullptr; size_t stride = r.row_bytes;
    switch (i) {
      case SNAP_STATE: dev = (uint8_t*)(m.st + s); break;
      case SNAP_POINT_POS: dev = (uint8_t*)(m.pts + (size_t)s * P); stride = sizeof(MapPointDev); break;
      case SNAP_POINT_REST: dev = (uint8_t*)(m.pts + (size_t)s * P) + SNAP_POS_BYTES; stride = sizeof(MapPointDev); break;
      case SNAP_TRACKDATA: dev = (uint8_t*)(m.td + (size_t)s * P); break;
      case SNAP_TMPL: dev = m.tmpl + (size_t)s * P * TMPL_PITCH; break;
      case SNAP_PT_FLAGS: dev = (uint8_t*)(m.pt_flags + (size_t)s * P); break;
      case SNAP_PT_LEVEL: dev = (uint8_t*)(m.pt_level + (size_t)s * P); break;
      case SNAP_CUR_MEAS: dev = (uint8_t*)(m.cur_meas + (size_t)s * P); break;
      case SNAP_KF_MEAS: dev = (uint8_t*)(m.kf_meas + (size_t)s * K * P); stride = P * sizeof(MeasDev); break;
      case SNAP_KF_POSE: dev = (uint8_t*)(m.kf_pose + (size_t)s * K); break;
      case SNAP_KF_FIXED: dev = (uint8_t*)(m.kf_fixed + (size_t)s * K); break;
      case SNAP_KF_DEPTH: dev = (uint8_t*)(m.kf_depth + (size_t)s * K * 2); break;
      case SNAP_KF_IMG0: case SNAP_KF_IMG1: case SNAP_KF_IMG2: case SNAP_KF_IMG3: {
        const LevelGeom& g = sys->geom[i - SNAP_KF_IMG0];
        dev = m.kf_img[i - SNAP_KF_IMG0] + (size_t)s * K * g.pitch * g.h; stride = (size_t)g.pitch;   // an image is h rows: the next one follows at the same stride
        break;
      }
      case SNAP_ITER_LIST: dev = (uint8_t*)(m.iter_list + (size_t)s * P); break;
      case SNAP_NEVER_RETRY: if (m.never_retry) dev = (uint8_t*)(m.never_retry + (size_t)s * P * 2); break;
      case SNAP_FAIL_QUEUE: if (m.fq) dev = (uint8_t*)(m.fq + (size_t)s * sys->tp.fq_cap); break;
      case SNAP_SBI_SMALL: if (sys->p.use_sbi) dev = sys->fr.sbi_small + (size_t)s * N; break;
      case SNAP_SBI_TMPL: if (sys->p.use_sbi) dev = (uint8_t*)(sys->fr.sbi_tmpl + (size_t)s * N); break;
      case SNAP_SBI_JACS: if (sys->p.use_sbi) dev = (uint8_t*)(sys->fr.sbi_jacs + (size_t)s * N * 2); break;
      case SNAP_SBI_ROT: if (sys->p.use_sbi) dev = (uint8_t*)(sys->fr.sbi_rot + (size_t)s * 8); break;
      case SNAP_RELOC_INFO: if (sys->reloc.info) dev = (uint8_t*)(sys->reloc.info + s); break;
      case SNAP_RELOC_CUR_TMPL: if (sys->reloc.cur_tmpl) dev = (uint8_t*)(sys->reloc.cur_tmpl + (size_t)s * N); break;
      case SNAP_RELOC_SCORES: if (sys->reloc.scores) dev = (uint8_t*)(sys->reloc.scores + (size_t)s * K); break;
      default: break;
    }
    SnapCopy& o = plan.c[i];
    o.dev = dev; o.blob_off = t.sec[i].off; o.rows = dev ? r.rows : 0; o.row_bytes = r.row_bytes; o.dev_stride = stride;
    if (o.rows > 1 && stride == r.row_bytes) { o.row_bytes = r.rows * r.row_bytes; o.dev_stride = o.row_bytes; o.rows = 1; }
  }
}

static int snap_blocks(size_t bytes) {
  const size_t b = (bytes + SNAP_BYTES_PER_BLOCK - 1) / SNAP_BYTES_PER_BLOCK;
  return b < 1 ? 1 : (b > SNAP_MAX_BLOCKS ? SNAP_MAX_BLOCKS : (int)b);
}

#define SNAP_CHK_STREAM(sys, s, who) do { if (!(sys) || (s) < 0 || (s) >= (sys)->S) { vslam_set_error("%s: bad system/stream", who); return VSLAM_E_INVALID; } } while (0)

// The stream's state and the counts its blob has; refuses the states a snapshot cannot carry
static int snap_source(vslam_system* sys, int s, const char* who, TrackerState* st, SnapCounts* c) {
  SNAP_CHK_STREAM(sys, s, who);
  if (sys->frame_open) { vslam_set_error("%s: a frame is open (vslam_finish_frame first)", who); return VSLAM_E_STATE; }
  VCHK(host_get(sys->stream, st, sys->map.st + s));
  if (st->init_stage == 1) { vslam_set_error("%s: the stream's trails are running (the trail tracker reads the previous frame in place)", who); return VSLAM_E_STATE; }
  if (sys->tp.ba_delay > 0 && st->ba_countdown > 0) { vslam_set_error("%s: an adjustment of the stream is pending (due in %d frames)", who, st->ba_countdown); return VSLAM_E_STATE; }
  const int P = sys->p.max_points, K = sys->p.max_keyframes;
  if (st->n_points < 0 || st->n_points > P || st->n_kf < 0 || st->n_kf > K || st->n_iter > P || st->fq_n < 0) {
    vslam_set_error("%s: the stream's counts exceed the system's capacities (%d points, %d keyframes, %d planned, %d queued)", who, st->n_points, st->n_kf, st->n_iter, st->fq_n);
    return VSLAM_E_STATE;
  }
  bool sbi = sys->p.use_sbi && sys->have_sbi;
  if (sbi && sys->sbi_restart_pending) {        // reset since its last frame: its next frame is its first, there is nothing to carry
    unsigned char f = 0;
    VCHK(host_get(sys->stream, &f, sys->sbi_restart + s));
    sbi = !f;
  }
  c->width = sys->p.width; c->height = sys->p.height;
  c->n_kf = st->n_kf; c->n_points = st->n_points; c->n_iter = st->n_iter < 0 ? 0 : st->n_iter;
  c->parts = (sys->map.never_retry ? SNAP_PART_IDLE : 0u) | (sbi ? SNAP_PART_SBI : 0u) | (sys->p.relocalise ? SNAP_PART_RELOC : 0u);
  // the entries that exist: k_ba_writeback counts past the queue's capacity and stores below it, the readers clamp (k_refind_idle).
  // TrackerState keeps the count as it is.
  c->fq_n = (c->parts & SNAP_PART_IDLE) ? (st->fq_n < sys->tp.fq_cap ? st->fq_n : sys->tp.fq_cap) : 0;
  if (!snap_counts_ok(*c)) { vslam_set_error("%s: the stream's counts are outside the snapshot format's range", who); return VSLAM_E_STATE; }
  return VSLAM_OK;
}

extern "C" int vslam_snapshot_size(vslam_system* sys, int s, size_t* bytes) {
  TrackerState st; SnapCounts c;
  if (!bytes) { vslam_set_error("snapshot_size: null argument"); return VSLAM_E_INVALID; }
  VCHK(snap_source(sys, s, "snapshot_size", &st, &c));
  *bytes = (size_t)snap_table(c).total;
  return VSLAM_OK;
}

extern "C" int vslam_snapshot_stream(vslam_system* sys, int s, void* dst, size_t cap, int dst_on_device, size_t* bytes) {
  TrackerState st; SnapCounts c;
  VCHK(snap_source(sys, s, "snapshot_stream", &st, &c));
  const SnapTable t = snap_table(c);
  const size_t total = (size_t)t.total;
  if (bytes) *bytes = total;
  if (!dst || cap < total) { vslam_set_error("snapshot_stream: the blob is %zu bytes, the buffer holds %zu", total, dst ? cap : (size_t)0); return dst ? VSLAM_E_CAPACITY : VSLAM_E_INVALID; }
  SnapHeader h;
  snap_fill_header(h, c, t);
  h.patch_size = sys->p.patch_size; h.quirks = sys->p.quirks; h.frame = st.frame; h.map_good = st.map_good;
  for (int i = 0; i < 5; i++) h.cam[i] = sys->p.cam[i];
  SnapPlan plan;
  snap_plan(sys, s, c, t, plan);
  plan.c[SNAP_FAIL_QUEUE].rows = 0;             // packed in sorted order by its own kernel
  DevTemp<uint8_t> stage;                       // sized by this blob, for this call
  HIPCHK(stage.get(total));
  HIPCHK(hipMemcpyAsync(stage.p, &h, sizeof(h), hipMemcpyHostToDevice, sys->stream));
  HIPCHK(hipEventRecord(sys->ev_snap_t[0], sys->stream));
  hipLaunchKernelGGL(k_snapshot<true>, dim3(snap_blocks(total)), dim3(SNAP_THREADS), 0, sys->stream, plan, stage.p);
  if (c.fq_n > 0)
    hipLaunchKernelGGL(k_pack_failure_queue, dim3((c.fq_n + SNAP_THREADS - 1) / SNAP_THREADS), dim3(SNAP_THREADS), 0, sys->stream,
                       (const int2*)(sys->map.fq + (size_t)s * sys->tp.fq_cap), c.fq_n, (int2*)(stage.p + t.sec[SNAP_FAIL_QUEUE].off));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(sys->ev_snap_t[1], sys->stream));
  sys->snap_timed[0] = true;
  HIPCHK(hipMemcpyAsync(dst, stage.p, total, dst_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, sys->stream));
  HIPCHK(hipStreamSynchronize(sys->stream));
  return VSLAM_OK;
}

static int snap_invalid(const char* who, int e) { vslam_set_error("%s: %s", who, snap_error_text(e)); return VSLAM_E_INVALID; }

extern "C" int vslam_restore_stream(vslam_system* sys, int s, const void* blob, size_t bytes, int on_device) {
  SNAP_CHK_STREAM(sys, s, "restore_stream");
  if (!blob) { vslam_set_error("restore_stream: null blob"); return VSLAM_E_INVALID; }
  if (sys->frame_open) { vslam_set_error("restore_stream: a frame is open (vslam_finish_frame first)"); return VSLAM_E_STATE; }
  // the header and the tracker state behind it, on the host: everything is decided before anything changes
  struct Head { SnapHeader h; TrackerState st; } head;
  static_assert(offsetof(Head, st) == sizeof(SnapHeader), "the state section follows the header");
  if (bytes < sizeof(head)) return snap_invalid("restore_stream", SNAP_E_SHORT);
  if (on_device) VCHK(host_get(sys->stream, &head, (const Head*)blob));
  else memcpy(&head, blob, sizeof(head));
  SnapHeader h;
  { const int e = snap_validate(&head.h, bytes, &h); if (e) return snap_invalid("restore_stream", e); }
  const TrackerState& st = head.st;
  const SnapCounts c = snap_header_counts(h);
  if (h.sec[SNAP_STATE].off != sizeof(SnapHeader) || st.n_kf != c.n_kf || st.n_points != c.n_points || (st.n_iter < 0 ? 0 : st.n_iter) != c.n_iter ||
      c.fq_n > (st.fq_n < 0 ? 0 : st.fq_n) || st.ba_countdown > 0 || st.init_stage == 1) {
    vslam_set_error("restore_stream: the tracker state in the blob disagrees with its header"); return VSLAM_E_INVALID;
  }
  const vslam_params& p = sys->p;
  bool same = h.width == p.width && h.height == p.height && h.patch_size == p.patch_size && h.quirks == p.quirks;
  for (int i = 0; i < 5; i++) same = same && memcmp(&h.cam[i], &p.cam[i], sizeof(double)) == 0;
  if (!same) {
    vslam_set_error("restore_stream: the blob is of a %d x %d system with patch size %d, quirks %d; this one is %d x %d, %d, %d (or the cameras differ)",
                    h.width, h.height, h.patch_size, h.quirks, p.width, p.height, p.patch_size, p.quirks);
    return VSLAM_E_INVALID;
  }
  if (c.n_kf > p.max_keyframes || c.n_points > p.max_points || c.n_iter > p.max_points || (sys->map.fq && c.fq_n > sys->tp.fq_cap)) {
    vslam_set_error("restore_stream: the blob holds %d keyframes, %d points, %d failure-queue entries; the system's capacities are %d, %d, %d",
                    c.n_kf, c.n_points, c.fq_n, p.max_keyframes, p.max_points, sys->tp.fq_cap);
    return VSLAM_E_CAPACITY;
  }
  SnapTable t;
  for (int i = 0; i < SNAP_N_SECTIONS; i++) t.sec[i] = h.sec[i];    // = snap_table(c): snap_validate has compared them
  t.total = h.total_bytes;
  SnapPlan plan;
  snap_plan(sys, s, c, t, plan);
  DevTemp<uint8_t> stage;                       // a host blob travels through device memory sized by it, for this call
  if (!on_device) HIPCHK(stage.get(bytes));
  HIPCHK(hipEventRecord(sys->ev_snap_t[2], sys->stream));
  VCHK(vslam_reset_streams(sys, &s, 1));        // the slot as a new system's: zero above the counts, a pending adjustment abandoned
  if (!on_device) HIPCHK(hipMemcpyAsync(stage.p, blob, bytes, hipMemcpyHostToDevice, sys->stream));
  const bool sbi = p.use_sbi && (c.parts & SNAP_PART_SBI);
  if (sbi && !sys->have_sbi) {
    // no frame yet: from here on a previous frame's SmallBlurryImage exists for this stream only; the others still start from their own
    HIPCHK(hipMemsetAsync(sys->sbi_restart, 1, (size_t)sys->S, sys->stream));
    sys->have_sbi = true;
  }
  hipLaunchKernelGGL(k_snapshot<false>, dim3(snap_blocks(bytes)), dim3(SNAP_THREADS), 0, sys->stream, plan, on_device ? (uint8_t*)blob : stage.p);
  HIPCHK(hipGetLastError());
  if (sbi) HIPCHK(hipMemsetAsync(sys->sbi_restart + s, 0, 1, sys->stream));   // its next frame is aligned to the carried image, not to itself
  if (sbi) sys->sbi_seen[(size_t)s] = 1;                                      // (... in a subset step too)
  if (sys->map.kf_ncorners) for (int k = 0; k < c.n_kf; k++) VCHK(fe_keyframe_corners(sys, s, k));   // Level::vCorners of the keyframes
  VCHK(reloc_keyframe_sbi(sys, s, 0, c.n_kf));                                                        // KeyFrame::pSBI
  HIPCHK(hipEventRecord(sys->ev_snap_t[3], sys->stream));
  sys->snap_timed[1] = true;
  // whatever the front-end and map-maker streams launch from now on comes after the restore
  HIPCHK(hipEventRecord(sys->ev_reset, sys->stream));
  HIPCHK(hipStreamWaitEvent(sys->fe_stream, sys->ev_reset, 0));
  for (hipStream_t q : sys->ba_streams) HIPCHK(hipStreamWaitEvent(q, sys->ev_reset, 0));
  if (!on_device) HIPCHK(hipStreamSynchronize(sys->stream));        // the caller's bytes and the staging copy are done with
  return VSLAM_OK;
}

extern "C" int vslam_snapshot_info(const void* blob, size_t bytes, vslam_snapshot_desc* out) {
  if (!out) { vslam_set_error("snapshot_info: null argument"); return VSLAM_E_INVALID; }
  SnapHeader h;
  { const int e = snap_validate(blob, bytes, &h); if (e) return snap_invalid("snapshot_info", e); }
  memset(out, 0, sizeof(*out));
  out->version = (int)h.version; out->width = h.width; out->height = h.height; out->patch_size = h.patch_size; out->quirks = h.quirks;
  for (int i = 0; i < 5; i++) out->cam[i] = h.cam[i];
  out->n_keyframes = h.n_kf; out->n_points = h.n_points; out->frame = h.frame; out->map_good = h.map_good;
  out->has_idle_state = (h.parts & SNAP_PART_IDLE) ? 1 : 0; out->has_sbi = (h.parts & SNAP_PART_SBI) ? 1 : 0; out->has_reloc_state = (h.parts & SNAP_PART_RELOC) ? 1 : 0;
  out->total_bytes = h.total_bytes;
  for (int l = 0; l < NLEV; l++) {
    out->image_offset[l] = h.sec[SNAP_KF_IMG0 + l].off;
    out->image_row_stride[l] = (unsigned long long)(h.width >> l);
    out->image_stride[l] = (unsigned long long)(h.width >> l) * (unsigned long long)(h.height >> l);
  }
  out->point_pos_offset = h.sec[SNAP_POINT_POS].off;
  out->keyframe_pose_offset = h.sec[SNAP_KF_POSE].off;
  return VSLAM_OK;
}

extern "C" int vslam_save_stream(vslam_system* sys, int s, const char* path) {
  if (!path) { vslam_set_error("save_stream: null path"); return VSLAM_E_INVALID; }
  size_t n = 0;
  VCHK(vslam_snapshot_size(sys, s, &n));
  std::vector<uint8_t> buf(n);
  VCHK(vslam_snapshot_stream(sys, s, buf.data(), buf.size(), 0, &n));
  FILE* f = fopen(path, "wb");
  if (!f) { vslam_set_error("save_stream: cannot open the file for writing"); return VSLAM_E_INVALID; }
  const size_t w = fwrite(buf.data(), 1, n, f);
  if (fclose(f) != 0 || w != n) { vslam_set_error("save_stream: short write (%zu of %zu bytes)", w, n); return VSLAM_E_INVALID; }
  return VSLAM_OK;
}

extern "C" int vslam_load_stream(vslam_system* sys, int s, const char* path) {
  SNAP_CHK_STREAM(sys, s, "load_stream");
  if (!path) { vslam_set_error("load_stream: null path"); return VSLAM_E_INVALID; }
  FILE* f = fopen(path, "rb");
  if (!f) { vslam_set_error("load_stream: cannot open the file"); return VSLAM_E_INVALID; }
  std::vector<uint8_t> buf;
  uint8_t chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
  fclose(f);
  return vslam_restore_stream(sys, s, buf.data(), buf.size(), 0);
}

extern "C" int vslam_get_snapshot_timing(vslam_system* sys, double ms[2]) {
  if (!sys || !ms) { vslam_set_error("get_snapshot_timing: bad argument"); return VSLAM_E_INVALID; }
  HIPCHK(hipStreamSynchronize(sys->stream));
  for (int k = 0; k < 2; k++) {
    float t = 0.f;
    if (sys->snap_timed[k]) HIPCHK(hipEventElapsedTime(&t, sys->ev_snap_t[2 * k], sys->ev_snap_t[2 * k + 1]));
    ms[k] = t;
  }
  return VSLAM_OK;
}
