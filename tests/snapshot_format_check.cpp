// Stand-alone check of csrc/snapshot_format.h as plain host C++, meant to be built with -fsanitize=address,undefined and run as a program
// (tests/test_snapshot_format_sanitized.py does that).  Every buffer handed to snap_validate is a heap allocation of exactly the length
// it is told, so a read past `bytes` is an AddressSanitizer report.  Prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include "../visualslam_android_amd/csrc/snapshot_format.h"

#include <stdio.h>
#include <stdlib.h>
#include <vector>

static long g_checks = 0;
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// snap_validate on a copy of the first n bytes of src, told that the blob is `told` bytes long
static int validate_prefix(const std::vector<uint8_t>& src, size_t n, uint64_t told, SnapHeader* out) {
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(p, src.data(), n);
  const int e = snap_validate(n ? p : nullptr, told, out);
  free(p);
  return e;
}

static std::vector<uint8_t> header_bytes(const SnapCounts& c) {
  const SnapTable t = snap_table(c);
  SnapHeader h;
  snap_fill_header(h, c, t);
  h.patch_size = 11; h.quirks = 0; h.frame = 17; h.map_good = c.n_kf > 0;
  for (int i = 0; i < 5; i++) h.cam[i] = 0.1 * (i + 1);
  std::vector<uint8_t> v(sizeof(h));
  memcpy(v.data(), &h, sizeof(h));
  return v;
}

static void check_counts(const SnapCounts& c) {
  CHECK(snap_counts_ok(c), "%d x %d, %d kf, %d points", c.width, c.height, c.n_kf, c.n_points);
  const SnapTable t = snap_table(c);
  // the table: in order, 16-byte aligned, sized rows x row_bytes, gaps below 16 bytes, total = the aligned end of the last section
  uint64_t prev_end = sizeof(SnapHeader);
  for (int i = 0; i < SNAP_N_SECTIONS; i++) {
    const SnapRows r = snap_section_rows(c, i);
    CHECK(t.sec[i].off % 16 == 0 && t.sec[i].off == snap_align16(prev_end), "section %d at %llu after %llu", i, (unsigned long long)t.sec[i].off, (unsigned long long)prev_end);
    CHECK(t.sec[i].bytes == r.rows * r.row_bytes, "section %d", i);
    prev_end = t.sec[i].off + t.sec[i].bytes;
  }
  CHECK(t.total == snap_align16(prev_end), "total");
  CHECK(t.sec[SNAP_POINT_POS].bytes == (uint64_t)c.n_points * 24 && t.sec[SNAP_KF_POSE].bytes == (uint64_t)c.n_kf * 96, "positions and poses");
  for (int l = 0; l < SNAP_LEVELS; l++)
    CHECK(t.sec[SNAP_KF_IMG0 + l].bytes == (uint64_t)c.n_kf * (uint64_t)(c.width >> l) * (uint64_t)(c.height >> l), "level %d", l);
  // round trip through the validator
  const std::vector<uint8_t> hb = header_bytes(c);
  SnapHeader back;
  CHECK(validate_prefix(hb, hb.size(), t.total, &back) == SNAP_OK, "a well-formed header is refused");
  CHECK(memcmp(&back, hb.data(), sizeof(back)) == 0, "the header comes back changed");
  const SnapCounts cb = snap_header_counts(back);
  CHECK(cb.width == c.width && cb.height == c.height && cb.n_kf == c.n_kf && cb.n_points == c.n_points && cb.n_iter == c.n_iter && cb.fq_n == c.fq_n && cb.parts == c.parts, "counts");
  // told one byte less or more than the total
  CHECK(validate_prefix(hb, hb.size(), t.total - 1, nullptr) != SNAP_OK && validate_prefix(hb, hb.size(), t.total + 1, nullptr) != SNAP_OK, "a wrong total is accepted");
  // told a length that ends one byte before each section's end
  for (int i = 0; i < SNAP_N_SECTIONS; i++) {
    if (!t.sec[i].bytes) continue;
    CHECK(validate_prefix(hb, hb.size(), t.sec[i].off + t.sec[i].bytes - 1, nullptr) != SNAP_OK, "cut inside section %d accepted", i);
  }
}

int main() {
  const int dims[][2] = {{48, 48}, {330, 250}, {640, 480}, {4096, 4096}};
  const int kfs[] = {0, 1, 8, 128, SNAP_MAX_KF};
  const int pts[] = {0, 1, 63, 64, 65, 4096, SNAP_MAX_POINTS};
  for (const auto& d : dims) for (int nk : kfs) for (int np : pts) for (unsigned parts = 0; parts < 8; parts++) {
    SnapCounts c;
    c.width = d[0]; c.height = d[1]; c.n_kf = nk; c.n_points = np; c.n_iter = np < 1000 ? np : 1000; c.parts = parts;
    c.fq_n = (parts & SNAP_PART_IDLE) ? np / 3 : 0;
    check_counts(c);
  }
  SnapCounts c;
  c.width = 640; c.height = 480; c.n_kf = 8; c.n_points = 65; c.n_iter = 40; c.fq_n = 5; c.parts = SNAP_PART_IDLE | SNAP_PART_SBI | SNAP_PART_RELOC;
  const SnapTable t = snap_table(c);
  const std::vector<uint8_t> hb = header_bytes(c);
  // every truncation length of one header, with the true total and with the truncated length as `bytes`
  for (size_t n = 0; n < hb.size(); n++) {
    CHECK(validate_prefix(hb, n, n, nullptr) != SNAP_OK, "a header cut to %zu bytes is accepted", n);
  }
  CHECK(validate_prefix(hb, 0, t.total, nullptr) != SNAP_OK, "a null blob is accepted");
  // each offset or size field pushed past the end, and to the values that wrap
  const uint64_t bad[] = {t.total, t.total + 1, t.total + 16, ~(uint64_t)0, ~(uint64_t)0 - 15, (uint64_t)1 << 63};
  for (int i = 0; i < SNAP_N_SECTIONS; i++) for (int field = 0; field < 2; field++) for (uint64_t v : bad) {
    std::vector<uint8_t> m = hb;
    SnapHeader h;
    memcpy(&h, m.data(), sizeof(h));
    (field ? h.sec[i].bytes : h.sec[i].off) = v;
    memcpy(m.data(), &h, sizeof(h));
    CHECK(validate_prefix(m, m.size(), t.total, nullptr) != SNAP_OK, "section %d %s = %llu accepted", i, field ? "bytes" : "off", (unsigned long long)v);
  }
  {
    std::vector<uint8_t> m = hb;
    SnapHeader h;
    memcpy(&h, m.data(), sizeof(h));
    h.total_bytes = ~(uint64_t)0;
    memcpy(m.data(), &h, sizeof(h));
    CHECK(validate_prefix(m, m.size(), t.total, nullptr) != SNAP_OK && validate_prefix(m, m.size(), ~(uint64_t)0, nullptr) != SNAP_OK, "total_bytes pushed past the end accepted");
  }
  // counts outside their range never reach the table
  const int32_t wild[] = {-1, INT32_MIN, INT32_MAX, SNAP_MAX_POINTS + 1};
  for (int field = 0; field < 6; field++) for (int32_t v : wild) {
    std::vector<uint8_t> m = hb;
    SnapHeader h;
    memcpy(&h, m.data(), sizeof(h));
    int32_t* f[] = {&h.width, &h.height, &h.n_kf, &h.n_points, &h.n_iter, &h.fq_n};
    *f[field] = v;
    memcpy(m.data(), &h, sizeof(h));
    CHECK(validate_prefix(m, m.size(), t.total, nullptr) != SNAP_OK, "count field %d = %d accepted", field, v);
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
