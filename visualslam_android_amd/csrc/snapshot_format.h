// The snapshot of one stream (vslam_snapshot_stream / vslam_restore_stream, snapshot.hip): the layout of the blob, stated once for the host
// and for gfx950 (like pvs_perm.h).  The reference's only persistence is MapMaker::GUICommandHandler("SaveMap"), jni/MapMaker.cc:1254-1286,
// a text dump of positions and poses; what is carried here is the whole Map (jni/Map.h:21-34) with the Tracker's and the MapMaker's members
// that belong to it, in the project's own binary form.
//
//   [SnapHeader][section 0][section 1] ... [section SNAP_N_SECTIONS - 1]
//
// Every section starts at a multiple of 16 bytes; the bytes between the end of a section and the next start are zero, so equal states
// give equal blobs.  A section is `rows` rows of `row_bytes` bytes, dense (row stride = row_bytes): the counts in use, never a capacity --
// nothing in the blob depends on the source's max_points, max_keyframes, max_corners, n_streams or slot index.  A section whose part is
// absent (SNAP_PART_*) or whose count is zero has bytes = 0 and the offset the next one has.
//
// snap_table is the one function from the counts to the section table: the pack planner, the unpack planner (snapshot.hip) and
// snap_validate (behind vslam_snapshot_info) all call it, and a header whose stored table differs from it is refused.
//
// There is no checksum: integrity in transit is the transport's job.  snap_validate checks that a blob is well formed (magic, version,
// sizes, every section inside `bytes`), not that its payload is the one that was written.
//
// Little-endian, the structs of vslam_internal.h as gfx950 and x86-64 lay them out; SNAP_VERSION changes whenever one of them does
// (snapshot.hip asserts the sizes below against them).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SNAP_FN __host__ __device__ inline
#else
#define SNAP_FN inline
#endif

#define SNAP_MAGIC "VSLMSNAP"        // 8 bytes, no terminator in the blob
#define SNAP_VERSION 1u
#define SNAP_LEVELS 4

// element sizes (bytes) of the carried structs
#define SNAP_STATE_BYTES 624         // TrackerState
#define SNAP_POS_BYTES 24            // MapPointDev::pos
#define SNAP_POINT_REST_BYTES 80     // MapPointDev after pos
#define SNAP_TRACKDATA_BYTES 168     // TrackData
#define SNAP_TMPL_BYTES 128          // TMPL_PITCH
#define SNAP_MEAS_BYTES 24           // MeasDev
#define SNAP_POSE_BYTES 96           // Pose = the C ABI's pose12: R row-major (9 doubles), t (3)
#define SNAP_RELOC_INFO_BYTES 176    // RelocInfo

// optional parts
#define SNAP_PART_IDLE 1u            // never-retry sets + failure queue (the source keeps idle jobs)
#define SNAP_PART_SBI 2u             // the last frame's SmallBlurryImage (use_sbi, and the source has tracked a frame)
#define SNAP_PART_RELOC 4u           // RelocInfo + the last attempt's arrays (relocalise)

enum SnapSection : int {
  SNAP_STATE = 0,          // 1 x TrackerState
  SNAP_POINT_POS,          // n_points x 3 doubles                 MapPoint::v3WorldPos
  SNAP_POINT_REST,         // n_points x the rest of MapPointDev
  SNAP_TRACKDATA,          // n_points x TrackData
  SNAP_TMPL,               // n_points x 128
  SNAP_PT_FLAGS,           // n_points x int
  SNAP_PT_LEVEL,           // n_points x int
  SNAP_CUR_MEAS,           // n_points x MeasDev                   mCurrentKF.mMeasurements
  SNAP_KF_MEAS,            // n_kf rows of n_points x MeasDev
  SNAP_KF_POSE,            // n_kf x pose12
  SNAP_KF_FIXED,           // n_kf x int
  SNAP_KF_DEPTH,           // n_kf x 2 doubles
  SNAP_KF_IMG0, SNAP_KF_IMG1, SNAP_KF_IMG2, SNAP_KF_IMG3,   // n_kf images of (h >> l) rows of (w >> l) bytes: row stride w >> l, image stride (w >> l) * (h >> l)
  SNAP_ITER_LIST,          // n_iter x int                         vIterationSet of the last frame
  SNAP_NEVER_RETRY,        // n_points x 2 x u64                   (SNAP_PART_IDLE)
  SNAP_FAIL_QUEUE,         // fq_n x (keyframe, point)             (SNAP_PART_IDLE) sorted by (keyframe, point); fq_n = the entries stored, at most the
                           //                                      source queue's capacity (TrackerState::fq_n may count past it)
  SNAP_SBI_SMALL,          // (w/16) x (h/16) bytes                (SNAP_PART_SBI) mimSmall
  SNAP_SBI_TMPL,           // ... floats                           mimTemplate
  SNAP_SBI_JACS,           // ... x 2 floats                       mimImageJacs
  SNAP_SBI_ROT,            // 8 doubles                            mv6SBIRot, score, spare
  SNAP_RELOC_INFO,         // 1 x RelocInfo                        (SNAP_PART_RELOC)
  SNAP_RELOC_CUR_TMPL,     // (w/16) x (h/16) floats
  SNAP_RELOC_SCORES,       // n_kf doubles
  SNAP_N_SECTIONS
};

struct SnapCounts {
  int32_t width, height;
  int32_t n_kf, n_points, n_iter, fq_n;
  uint32_t parts;
};
struct SnapRows { uint64_t rows, row_bytes; };
struct SnapSpan { uint64_t off, bytes; };
struct SnapTable { SnapSpan sec[SNAP_N_SECTIONS]; uint64_t total; };

struct SnapHeader {
  char magic[8];
  uint32_t version, header_bytes;
  uint64_t total_bytes;
  int32_t width, height, patch_size, quirks;
  double cam[5];
  int32_t n_kf, n_points, frame, map_good;
  int32_t n_iter, fq_n;
  uint32_t parts, reserved;
  SnapSpan sec[SNAP_N_SECTIONS];
};
static_assert(sizeof(SnapHeader) % 16 == 0, "the first section starts at a multiple of 16 bytes");

// bounds of a well-formed header: with them no product below leaves 64 bits
#define SNAP_MAX_DIM 4096
#define SNAP_MIN_DIM 48
#define SNAP_MAX_KF 4096
#define SNAP_MAX_POINTS (1 << 24)
#define SNAP_MAX_FQ (1 << 28)

SNAP_FN uint64_t snap_align16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
SNAP_FN uint64_t snap_small_pixels(int width, int height) { return (uint64_t)((width >> 3) / 2) * (uint64_t)((height >> 3) / 2); }

SNAP_FN bool snap_counts_ok(const SnapCounts& c) {
  return c.width >= SNAP_MIN_DIM && c.width <= SNAP_MAX_DIM && c.height >= SNAP_MIN_DIM && c.height <= SNAP_MAX_DIM &&
         c.n_kf >= 0 && c.n_kf <= SNAP_MAX_KF && c.n_points >= 0 && c.n_points <= SNAP_MAX_POINTS && c.n_iter >= 0 && c.n_iter <= SNAP_MAX_POINTS &&
         c.fq_n >= 0 && c.fq_n <= SNAP_MAX_FQ && (c.parts & ~(SNAP_PART_IDLE | SNAP_PART_SBI | SNAP_PART_RELOC)) == 0 &&
         ((c.parts & SNAP_PART_IDLE) || c.fq_n == 0);
}

// rows x row_bytes of one section for these counts (0 x 0 where its part is absent)
SNAP_FN SnapRows snap_section_rows(const SnapCounts& c, int sec) {
  const uint64_t np = (uint64_t)c.n_points, nk = (uint64_t)c.n_kf, N = snap_small_pixels(c.width, c.height);
  const bool idle = c.parts & SNAP_PART_IDLE, sbi = c.parts & SNAP_PART_SBI, reloc = c.parts & SNAP_PART_RELOC;
  SnapRows r = {0, 0};
  switch (sec) {
    case SNAP_STATE: r = {1, SNAP_STATE_BYTES}; break;
    case SNAP_POINT_POS: r = {np, SNAP_POS_BYTES}; break;
    case SNAP_POINT_REST: r = {np, SNAP_POINT_REST_BYTES}; break;
    case SNAP_TRACKDATA: r = {np, SNAP_TRACKDATA_BYTES}; break;
    case SNAP_TMPL: r = {np, SNAP_TMPL_BYTES}; break;
    case SNAP_PT_FLAGS: case SNAP_PT_LEVEL: r = {np, 4}; break;
    case SNAP_CUR_MEAS: r = {np, SNAP_MEAS_BYTES}; break;
    case SNAP_KF_MEAS: r = {nk, np * SNAP_MEAS_BYTES}; break;
    case SNAP_KF_POSE: r = {nk, SNAP_POSE_BYTES}; break;
    case SNAP_KF_FIXED: r = {nk, 4}; break;
    case SNAP_KF_DEPTH: r = {nk, 16}; break;
    case SNAP_KF_IMG0: case SNAP_KF_IMG1: case SNAP_KF_IMG2: case SNAP_KF_IMG3: {
      const int l = sec - SNAP_KF_IMG0;
      r = {nk * (uint64_t)(c.height >> l), (uint64_t)(c.width >> l)};
      break;
    }
    case SNAP_ITER_LIST: r = {(uint64_t)c.n_iter, 4}; break;
    case SNAP_NEVER_RETRY: if (idle) r = {np, 16}; break;
    case SNAP_FAIL_QUEUE: if (idle) r = {(uint64_t)c.fq_n, 8}; break;
    case SNAP_SBI_SMALL: if (sbi) r = {1, N}; break;
    case SNAP_SBI_TMPL: if (sbi) r = {1, N * 4}; break;
    case SNAP_SBI_JACS: if (sbi) r = {1, N * 8}; break;
    case SNAP_SBI_ROT: if (sbi) r = {1, 64}; break;
    case SNAP_RELOC_INFO: if (reloc) r = {1, SNAP_RELOC_INFO_BYTES}; break;
    case SNAP_RELOC_CUR_TMPL: if (reloc) r = {1, N * 4}; break;
    case SNAP_RELOC_SCORES: if (reloc) r = {nk, 8}; break;
    default: break;
  }
  if (r.rows == 0 || r.row_bytes == 0) r = {0, 0};
  return r;
}

// counts -> section table (snap_counts_ok(c) holds)
SNAP_FN SnapTable snap_table(const SnapCounts& c) {
  SnapTable t;
  uint64_t off = sizeof(SnapHeader);
  for (int i = 0; i < SNAP_N_SECTIONS; i++) {
    const SnapRows r = snap_section_rows(c, i);
    t.sec[i].off = off; t.sec[i].bytes = r.rows * r.row_bytes;
    off = snap_align16(off + t.sec[i].bytes);
  }
  t.total = off;
  return t;
}

SNAP_FN SnapCounts snap_header_counts(const SnapHeader& h) {
  SnapCounts c;
  c.width = h.width; c.height = h.height; c.n_kf = h.n_kf; c.n_points = h.n_points; c.n_iter = h.n_iter; c.fq_n = h.fq_n; c.parts = h.parts;
  return c;
}

// the header of a blob with these counts; the caller fills patch_size, quirks, cam, frame and map_good
SNAP_FN void snap_fill_header(SnapHeader& h, const SnapCounts& c, const SnapTable& t) {
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, SNAP_MAGIC, 8);
  h.version = SNAP_VERSION; h.header_bytes = (uint32_t)sizeof(SnapHeader); h.total_bytes = t.total;
  h.width = c.width; h.height = c.height; h.n_kf = c.n_kf; h.n_points = c.n_points; h.n_iter = c.n_iter; h.fq_n = c.fq_n; h.parts = c.parts;
  for (int i = 0; i < SNAP_N_SECTIONS; i++) h.sec[i] = t.sec[i];
}

enum SnapError : int {
  SNAP_OK = 0, SNAP_E_SHORT, SNAP_E_MAGIC, SNAP_E_VERSION, SNAP_E_HEADER_SIZE, SNAP_E_COUNTS, SNAP_E_PATCH, SNAP_E_SECTION, SNAP_E_TOTAL, SNAP_E_TRUNCATED
};
SNAP_FN const char* snap_error_text(int e) {
  switch (e) {
    case SNAP_OK: return "ok";
    case SNAP_E_SHORT: return "fewer bytes than a header";
    case SNAP_E_MAGIC: return "not a stream snapshot (magic)";
    case SNAP_E_VERSION: return "a snapshot of another format version";
    case SNAP_E_HEADER_SIZE: return "header size field";
    case SNAP_E_COUNTS: return "a size or count outside its range";
    case SNAP_E_PATCH: return "patch size is neither 8 nor 11";
    case SNAP_E_SECTION: return "a section offset or size disagrees with the counts";
    case SNAP_E_TOTAL: return "the total size disagrees with the counts";
    default: return "the total size disagrees with the number of bytes given";
  }
}

// Is `blob` (only its first min(bytes, sizeof(SnapHeader)) bytes are read) the head of a well-formed snapshot of exactly `bytes` bytes?
// On SNAP_OK *out holds the header.  No field is used before it has been checked, and every section is checked against `bytes`.
SNAP_FN int snap_validate(const void* blob, uint64_t bytes, SnapHeader* out) {
  if (!blob || bytes < sizeof(SnapHeader)) return SNAP_E_SHORT;
  SnapHeader h;
  memcpy(&h, blob, sizeof(h));
  if (memcmp(h.magic, SNAP_MAGIC, 8) != 0) return SNAP_E_MAGIC;
  if (h.version != SNAP_VERSION) return SNAP_E_VERSION;
  if (h.header_bytes != sizeof(SnapHeader)) return SNAP_E_HEADER_SIZE;
  const SnapCounts c = snap_header_counts(h);
  if (!snap_counts_ok(c) || h.reserved != 0) return SNAP_E_COUNTS;
  if (h.patch_size != 8 && h.patch_size != 11) return SNAP_E_PATCH;
  const SnapTable t = snap_table(c);
  for (int i = 0; i < SNAP_N_SECTIONS; i++) {
    if (h.sec[i].off != t.sec[i].off || h.sec[i].bytes != t.sec[i].bytes) return SNAP_E_SECTION;
    if (h.sec[i].off > bytes || h.sec[i].bytes > bytes - h.sec[i].off) return SNAP_E_TRUNCATED;
  }
  if (h.total_bytes != t.total) return SNAP_E_TOTAL;
  if (h.total_bytes != bytes) return SNAP_E_TRUNCATED;
  if (out) *out = h;
  return SNAP_OK;
}
