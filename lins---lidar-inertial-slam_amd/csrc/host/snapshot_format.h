// snapshot_format.h — the blob of a stream snapshot (include/lins_snapshot.h) and its copy plan, one text for both
// libraries: lins_streams_snapshot / _restore (lins_snapshot_capi.hip) run it in front of their kernels, liblins_host.so
// exports it as lins_host_snapshot_* (host/snapshot_format.cpp) and tests/native/snapshot_check.cpp holds it under the
// sanitizers.  Pure: no allocation besides the vectors named, nothing read beyond the bytes given.
//
//   blob = header (lins_snapshot_info) | directory (LINS_SNAP_SECTIONS entries) | host-only sections | device sections
// Every section starts at a multiple of 16; its padding is zero.  The directory is a function of (modules, counts) alone
// (layout), so a blob whose directory differs from that function of its own header is refused.  The device sections are
// contiguous: the staging buffer of a pack or an unpack is that part of the blob, byte for byte.
//
// Invariants of a plan (segments_ok checks them for a whole call; tests/test_snapshot_host.py on 200 count sets):
//   1  segments are pairwise disjoint on the module side (same buffer: disjoint unit ranges)
//   2  they lie within the buffers' sizes and within the staging buffer
//   3  on the staging side they are disjoint and, with the sections' padding, cover the device part of every blob
//      exactly once — so with the host-only sections the blob is covered exactly once
// The unpack kernel writes through the table of these segments; the table is what keeps it inside the buffers.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../../include/lins_snapshot.h"

namespace lins_snap {

// rows of the 8-byte-unit buffers, in units
constexpr int kRowState = 19, kRowCov = 324, kRowNoise = 144, kRowAux = 16, kRowPre = 17, kRowOdom = 11, kRowMapPose = 14;
constexpr int kFilterRow = kRowState + kRowCov + kRowNoise + kRowAux + kRowState;
static_assert(sizeof(lins_stream_odom) == 8 * kRowOdom, "odometry record");
static_assert(sizeof(lins_snapshot_info) == 384 && sizeof(lins_snapshot_dirent) == 24, "header layout");
static_assert(sizeof(lins_snapshot_stream_rec) == 272 && sizeof(lins_snapshot_frame) == 88 && sizeof(lins_snapshot_loop) == 112, "record layout");
static_assert(sizeof(lins_snapshot_counts) == 56 && sizeof(lins_snapshot_facts) == 280, "header parts");
constexpr uint64_t kDirBytes = LINS_SNAP_SECTIONS * sizeof(lins_snapshot_dirent);
static_assert(kDirBytes % 16 == 0, "directory keeps the sections aligned");
constexpr uint64_t kPayloadAt = sizeof(lins_snapshot_info) + kDirBytes;
constexpr uint32_t kAllModules = 255u;
constexpr int64_t kMaxPoints = 1ll << 40;  // lins_archive_init's bound

inline uint64_t pad16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// 64-bit sum over 8-byte words (bytes: a multiple of 8): every step is a bijection of the running value, so two inputs
// that differ in one word give different sums
inline uint64_t sum64(const void* p, uint64_t bytes, uint64_t h = 0x9e3779b97f4a7c15ull) {
  const unsigned char* c = (const unsigned char*)p;
  for (uint64_t i = 0; i + 8 <= bytes; i += 8) {
    uint64_t w;
    std::memcpy(&w, c + i, 8);
    h = (h ^ w) * 0x100000001b3ull;
    h = (h << 29) | (h >> 35);
  }
  return h;
}

inline bool counts_ok(uint32_t modules, const lins_snapshot_counts& c) {
  if (!(modules & LINS_SNAP_STREAM) || (modules & ~kAllModules)) return false;
  const int32_t ints[] = {c.less_sharp, c.less_flat, c.outliers, c.ring_frames, c.archive_frames, c.graph_frames, c.graph_loops, c.graph_up_frames, c.surround};
  for (int32_t v : ints)
    if (v < 0) return false;
  if (c.has_scan != 0 && c.has_scan != 1) return false;
  if (!c.has_scan && (c.less_sharp || c.less_flat)) return false;
  if (c.ring_points < 0 || c.archive_points < 0 || c.ring_points > kMaxPoints || c.archive_points > kMaxPoints) return false;
  if (!(modules & LINS_SNAP_RING) && (c.ring_frames || c.ring_points)) return false;
  if (!(modules & LINS_SNAP_ARCHIVE) && (c.archive_frames || c.archive_points)) return false;
  if (!(modules & LINS_SNAP_GRAPH) && (c.graph_frames || c.graph_loops || c.graph_up_frames)) return false;
  if (!(modules & LINS_SNAP_MAP_POSE) && c.surround) return false;
  if (!c.ring_frames && c.ring_points) return false;
  if (!c.archive_frames && c.archive_points) return false;
  if (c.graph_up_frames > c.graph_frames || (!c.graph_frames && c.graph_loops)) return false;
  return true;
}

inline uint32_t unit_of(int sec) { return sec < LINS_SNAP_FIRST_DEVICE_SEC ? 1u : sec < LINS_SNAP_FIRST_UNIT8_SEC ? 16u : 8u; }

inline uint64_t bytes_of(int sec, uint32_t modules, const lins_snapshot_counts& c) {
  switch (sec) {
    case LINS_SNAP_SEC_STREAM_REC: return sizeof(lins_snapshot_stream_rec);
    case LINS_SNAP_SEC_SURROUND: return 4ull * (uint64_t)c.surround;
    case LINS_SNAP_SEC_RING_META: return sizeof(lins_snapshot_frame) * (uint64_t)c.ring_frames;
    case LINS_SNAP_SEC_AR_META: return sizeof(lins_snapshot_frame) * (uint64_t)c.archive_frames;
    case LINS_SNAP_SEC_PG_HOST: return 216ull * (uint64_t)c.graph_frames + sizeof(lins_snapshot_loop) * (uint64_t)c.graph_loops;
    case LINS_SNAP_SEC_SCAN_PTS: return 16ull * ((uint64_t)c.less_flat + (uint64_t)c.less_sharp);
    case LINS_SNAP_SEC_OUTL_PTS: return 16ull * (uint64_t)c.outliers;
    case LINS_SNAP_SEC_RING_PTS: return 16ull * (uint64_t)c.ring_points;
    case LINS_SNAP_SEC_AR_PTS: return 16ull * (uint64_t)c.archive_points;
    case LINS_SNAP_SEC_FILTER_ROWS: return modules & LINS_SNAP_FILTER ? 8ull * kFilterRow : 0;
    case LINS_SNAP_SEC_BOOT_PRE: return modules & LINS_SNAP_BOOT ? 8ull * kRowPre : 0;
    case LINS_SNAP_SEC_ODOM: return modules & LINS_SNAP_ODOM ? 8ull * kRowOdom : 0;
    case LINS_SNAP_SEC_MAP_POSE: return modules & LINS_SNAP_MAP_POSE ? 8ull * kRowMapPose : 0;
    case LINS_SNAP_SEC_PG_D: return 96ull * (uint64_t)c.graph_up_frames;
  }
  return 0;
}

// the directory and the blob's size; *device_at (may be null): where the device sections start
inline int layout(uint32_t modules, const lins_snapshot_counts& c, lins_snapshot_dirent* dir, uint64_t* total, uint64_t* device_at = nullptr) {
  if (!counts_ok(modules, c)) return LINS_E_ARG;
  uint64_t at = kPayloadAt;
  for (int s = 0; s < LINS_SNAP_SECTIONS; ++s) {
    if (s == LINS_SNAP_FIRST_DEVICE_SEC && device_at) *device_at = at;
    const uint64_t b = bytes_of(s, modules, c);
    if (dir) dir[s] = lins_snapshot_dirent{(uint32_t)s, unit_of(s), at, b};
    at += pad16(b);
  }
  if (total) *total = at;
  return LINS_OK;
}

inline uint64_t header_sum(const lins_snapshot_info& h, const lins_snapshot_dirent* dir) {
  lins_snapshot_info z = h;
  z.header_checksum = 0;
  return sum64(dir, kDirBytes, sum64(&z, sizeof z));
}

// header and directory in front of the sections already in place; padding zeroed; both sums
inline int seal(void* blob, uint64_t cap, uint32_t modules, const lins_snapshot_counts& c, const lins_snapshot_facts& facts) {
  lins_snapshot_dirent dir[LINS_SNAP_SECTIONS];
  uint64_t total = 0;
  if (!blob) return LINS_E_ARG;
  if (int rc = layout(modules, c, dir, &total)) return rc;
  if (cap < total) return LINS_E_CAPACITY;
  char* b = (char*)blob;
  for (int s = 0; s < LINS_SNAP_SECTIONS; ++s)
    if (dir[s].bytes % 16) std::memset(b + dir[s].offset + dir[s].bytes, 0, (size_t)(pad16(dir[s].bytes) - dir[s].bytes));
  lins_snapshot_info h;
  std::memset(&h, 0, sizeof h);
  h.magic = LINS_SNAPSHOT_MAGIC, h.version = LINS_SNAPSHOT_VERSION, h.header_bytes = (uint32_t)sizeof h;
  h.total_bytes = total, h.modules = modules, h.n_sections = LINS_SNAP_SECTIONS;
  h.counts = c, h.facts = facts;
  h.checksum = sum64(b + kPayloadAt, total - kPayloadAt);
  h.header_checksum = header_sum(h, dir);
  std::memcpy(b, &h, sizeof h);
  std::memcpy(b + sizeof h, dir, kDirBytes);
  return LINS_OK;
}

// the frame records of a section against the counts: non-negative sizes that add up to `points`
inline bool frames_ok(const char* sec, int n, int64_t points, int max_per_frame, std::vector<int32_t>* totals) {
  int64_t sum = 0;
  if (totals) totals->assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    lins_snapshot_frame f;
    std::memcpy(&f, sec + (size_t)i * sizeof f, sizeof f);
    if (f.n[0] < 0 || f.n[1] < 0 || f.n[2] < 0) return false;
    const int64_t t = (int64_t)f.n[0] + f.n[1] + f.n[2];
    if (t > 0x7fffffff || (max_per_frame >= 0 && t > max_per_frame)) return false;
    if (totals) (*totals)[i] = (int32_t)t;
    sum += t;
  }
  return sum == points;
}

// a blob that has passed check against what a destination offers: LINS_E_STATE (a module the destination lacks), then
// LINS_E_CAPACITY
inline int limits_check(const char* b, const lins_snapshot_info& h, const lins_snapshot_dirent* dir, const lins_snapshot_limits& lim) {
  const lins_snapshot_counts& c = h.counts;
  if (h.modules & ~lim.modules) return LINS_E_STATE;
  if (c.less_sharp > lim.less_sharp_max || c.less_flat > lim.less_flat_max || c.outliers > lim.outlier_max) return LINS_E_CAPACITY;
  if (c.ring_frames > lim.ring_window || !frames_ok(b + dir[LINS_SNAP_SEC_RING_META].offset, c.ring_frames, c.ring_points, lim.ring_max_pts, nullptr))
    return LINS_E_CAPACITY;
  if (c.archive_frames > lim.archive_frames || c.archive_points > lim.archive_points) return LINS_E_CAPACITY;
  if (c.graph_frames > lim.graph_frames || c.graph_loops > lim.graph_loops || c.surround > lim.surround_max) return LINS_E_CAPACITY;
  return LINS_OK;
}

inline int check(const void* blob, uint64_t bytes, const lins_snapshot_facts* facts, const lins_snapshot_limits* lim, lins_snapshot_info* out) {
  if (!blob) return LINS_E_ARG;
  if (bytes < kPayloadAt) return LINS_E_INPUT;
  const char* b = (const char*)blob;
  lins_snapshot_info h;
  std::memcpy(&h, b, sizeof h);
  if (h.magic != LINS_SNAPSHOT_MAGIC || h.version != LINS_SNAPSHOT_VERSION || h.header_bytes != sizeof h || h.n_sections != LINS_SNAP_SECTIONS) return LINS_E_INPUT;
  lins_snapshot_dirent dir[LINS_SNAP_SECTIONS], want[LINS_SNAP_SECTIONS];
  std::memcpy(dir, b + sizeof h, kDirBytes);
  if (h.header_checksum != header_sum(h, dir)) return LINS_E_INPUT;
  uint64_t total = 0;
  if (layout(h.modules, h.counts, want, &total)) return LINS_E_INPUT;
  if (std::memcmp(dir, want, kDirBytes) != 0 || total != h.total_bytes || bytes < total) return LINS_E_INPUT;
  if (h.checksum != sum64(b + kPayloadAt, total - kPayloadAt)) return LINS_E_INPUT;
  const lins_snapshot_counts& c = h.counts;
  if (!frames_ok(b + dir[LINS_SNAP_SEC_RING_META].offset, c.ring_frames, c.ring_points, -1, nullptr)) return LINS_E_INPUT;
  if (!frames_ok(b + dir[LINS_SNAP_SEC_AR_META].offset, c.archive_frames, c.archive_points, -1, nullptr)) return LINS_E_INPUT;
  for (int l = 0; l < c.graph_loops; ++l) {
    lins_snapshot_loop L;
    std::memcpy(&L, b + dir[LINS_SNAP_SEC_PG_HOST].offset + 216ull * (uint64_t)c.graph_frames + (size_t)l * sizeof L, sizeof L);
    if (L.latest < 0 || L.closest < 0 || L.latest >= c.graph_frames || L.closest >= c.graph_frames || L.latest == L.closest) return LINS_E_INPUT;
  }
  for (int i = 0; i < c.surround; ++i) {
    int32_t id;
    std::memcpy(&id, b + dir[LINS_SNAP_SEC_SURROUND].offset + 4ull * (uint64_t)i, 4);
    if (id < 0 || id >= c.archive_frames) return LINS_E_INPUT;
  }
  if (out) *out = h;
  if (facts && std::memcmp(facts, &h.facts, sizeof *facts) != 0) return LINS_E_STATE;
  return lim ? limits_check(b, h, dir, *lim) : LINS_OK;
}

// the copy segments of one stream, appended to segs; staging offsets follow the blob's device sections from stg_base.
// Neighbouring key frames that are neighbours in the arena become one segment.
inline int plan(uint32_t modules, const lins_snapshot_counts& c, const lins_snapshot_place& p, uint64_t stg_base, std::vector<lins_snapshot_segment>& segs) {
  lins_snapshot_dirent dir[LINS_SNAP_SECTIONS];
  uint64_t total = 0, dev_at = 0;
  if (stg_base % 16 || p.row < 0) return LINS_E_ARG;
  if (int rc = layout(modules, c, dir, &total, &dev_at)) return rc;
  if ((c.ring_frames && (!p.ring_off || !p.ring_n)) || (c.archive_frames && (!p.ar_off || !p.ar_n))) return LINS_E_ARG;
  auto stg = [&](int sec, uint32_t unit) { return (int64_t)((stg_base + dir[sec].offset - dev_at) / unit); };
  auto put = [&](int buffer, int unit, int64_t buf_off, int64_t stg_off, int64_t units) {
    if (units > 0) segs.push_back(lins_snapshot_segment{buffer, unit, buf_off, stg_off, units});
  };
  int64_t at = stg(LINS_SNAP_SEC_SCAN_PTS, 16);
  put(LINS_SNAP_BUF_SCAN, 16, p.scan_off[0], at, c.less_flat);
  put(LINS_SNAP_BUF_SCAN, 16, p.scan_off[1], at + c.less_flat, c.less_sharp);
  put(LINS_SNAP_BUF_OUTL, 16, p.outl_off, stg(LINS_SNAP_SEC_OUTL_PTS, 16), c.outliers);
  at = stg(LINS_SNAP_SEC_RING_PTS, 16);
  int64_t sum = 0;
  for (int i = 0; i < c.ring_frames; ++i) {
    if (p.ring_n[i] < 0) return LINS_E_ARG;
    put(LINS_SNAP_BUF_RING, 16, p.ring_off[i], at + sum, p.ring_n[i]);
    sum += p.ring_n[i];
  }
  if (sum != c.ring_points) return LINS_E_ARG;
  at = stg(LINS_SNAP_SEC_AR_PTS, 16), sum = 0;
  for (int i = 0; i < c.archive_frames; ++i) {
    if (p.ar_n[i] < 0) return LINS_E_ARG;
    if (p.ar_n[i] > 0) {
      if (!segs.empty() && segs.back().buffer == LINS_SNAP_BUF_ARENA && segs.back().stg_off + segs.back().units == at + sum &&
          segs.back().buf_off + segs.back().units == p.ar_off[i])
        segs.back().units += p.ar_n[i];
      else
        put(LINS_SNAP_BUF_ARENA, 16, p.ar_off[i], at + sum, p.ar_n[i]);
    }
    sum += p.ar_n[i];
  }
  if (sum != c.archive_points) return LINS_E_ARG;
  if (modules & LINS_SNAP_FILTER) {
    at = stg(LINS_SNAP_SEC_FILTER_ROWS, 8);
    const int rows[5] = {kRowState, kRowCov, kRowNoise, kRowAux, kRowState};
    for (int k = 0; k < 5; ++k) put(LINS_SNAP_BUF_F_STATE + k, 8, p.row * rows[k], at, rows[k]), at += rows[k];
  }
  if (modules & LINS_SNAP_BOOT) put(LINS_SNAP_BUF_B_PRE, 8, p.row * kRowPre, stg(LINS_SNAP_SEC_BOOT_PRE, 8), kRowPre);
  if (modules & LINS_SNAP_ODOM) put(LINS_SNAP_BUF_ODOM, 8, p.row * kRowOdom, stg(LINS_SNAP_SEC_ODOM, 8), kRowOdom);
  if (modules & LINS_SNAP_MAP_POSE) put(LINS_SNAP_BUF_MAP_POSE, 8, p.row * kRowMapPose, stg(LINS_SNAP_SEC_MAP_POSE, 8), kRowMapPose);
  put(LINS_SNAP_BUF_PG_D, 8, p.graph_off, stg(LINS_SNAP_SEC_PG_D, 8), 12ll * c.graph_up_frames);
  return LINS_OK;
}

// invariants 1 and 2, and the staging side of 3 (disjoint, inside stg_bytes), for the segments of a whole call
inline bool segments_ok(long long n, const lins_snapshot_segment* s, const int64_t* buf_units, uint64_t stg_bytes) {
  if (n < 0 || (n && (!s || !buf_units))) return false;
  std::vector<long long> order((size_t)n);
  for (long long i = 0; i < n; ++i) {
    const lins_snapshot_segment& g = s[i];
    if (g.buffer < 0 || g.buffer >= LINS_SNAP_BUFFERS || g.unit != (g.buffer < LINS_SNAP_FIRST_UNIT8_BUF ? 16 : 8)) return false;
    if (g.units < 1 || g.buf_off < 0 || g.stg_off < 0 || g.units > buf_units[g.buffer] || g.buf_off > buf_units[g.buffer] - g.units) return false;
    if ((uint64_t)g.units > stg_bytes / (uint64_t)g.unit || (uint64_t)g.stg_off > stg_bytes / (uint64_t)g.unit - (uint64_t)g.units) return false;
    order[(size_t)i] = i;
  }
  std::sort(order.begin(), order.end(), [&](long long a, long long b) { return s[a].buffer != s[b].buffer ? s[a].buffer < s[b].buffer : s[a].buf_off < s[b].buf_off; });
  for (long long i = 1; i < n; ++i) {
    const lins_snapshot_segment &a = s[order[(size_t)i - 1]], &b = s[order[(size_t)i]];
    if (a.buffer == b.buffer && a.buf_off + a.units > b.buf_off) return false;
  }
  std::sort(order.begin(), order.end(), [&](long long a, long long b) { return s[a].stg_off * s[a].unit < s[b].stg_off * s[b].unit; });
  for (long long i = 1; i < n; ++i) {
    const lins_snapshot_segment &a = s[order[(size_t)i - 1]], &b = s[order[(size_t)i]];
    if ((a.stg_off + a.units) * a.unit > b.stg_off * b.unit) return false;
  }
  return true;
}

}  // namespace lins_snap
