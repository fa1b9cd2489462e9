// snapshot_check.cpp — the snapshot blob's format and copy plan (csrc/host/snapshot_format.h through the exports of
// csrc/host/snapshot_format.cpp) on the CPU, under AddressSanitizer and UBSan (tests/test_snapshot_host.py).  Every blob
// lives in a heap block of exactly its size — and every truncated copy in one of exactly the truncated size — so that a
// check that reads beyond the bytes it was given ends the program.
//   snapshot_check roundtrip | corrupt | capacity | plan     one case each, over the same 200 count sets; exit 0 and
//                                                            "ok <case>" when every check holds
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "host/snapshot_format.h"

namespace {

constexpr int kSets = 200, kWindow = 5, kMaxLoops = 64;

#define REQUIRE(cond)                                                           \
  do {                                                                          \
    if (!(cond)) {                                                              \
      std::fprintf(stderr, "%s:%d: set %d: %s\n", __FILE__, __LINE__, g_set, #cond); \
      std::exit(1);                                                             \
    }                                                                           \
  } while (0)
int g_set = -1;

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int upto(int n) { return n > 0 ? (int)(next() % (uint32_t)(n + 1)) : 0; }  // [0, n]
};

struct Set {
  uint32_t modules = 0;
  lins_snapshot_counts c{};
  lins_snapshot_facts facts{};
  std::vector<lins_snapshot_frame> ring, ar;
  std::vector<lins_snapshot_loop> loops;
  std::vector<int32_t> surround;
};

int total_of(const lins_snapshot_frame& f) { return f.n[0] + f.n[1] + f.n[2]; }

lins_snapshot_frame frame(Rng& r, int a, int b, int c) {
  lins_snapshot_frame f;
  std::memset(&f, 0, sizeof f);
  f.n[0] = a, f.n[1] = b, f.n[2] = c;
  for (float& x : f.pose) x = (float)r.upto(2000) / 100.f - 10.f;
  for (float& x : f.t) x = (float)r.upto(2000) / 1000.f - 1.f;
  f.time = (double)r.upto(100000) / 10.0;
  return f;
}

// set i: 0 a fresh stream, 1 frames without points, 2 a frame without outliers, 3 a full ring, 4 a graph without loops,
// 5 a graph with the most loops; the others random, every module on or off
Set make_set(int i) {
  Rng r{0x5eed0000ull + (uint64_t)i};
  Set s;
  std::memset(&s.facts, 0, sizeof s.facts);
  s.facts.params.num_iter = 8 + i, s.facts.params.lidar_std = 0.01, s.facts.machine = i & 1, s.facts.ring_window = kWindow;
  s.modules = i < 6 ? lins_snap::kAllModules : (LINS_SNAP_STREAM | (r.next() & lins_snap::kAllModules));
  const bool rnd = i >= 6;
  if (rnd && r.upto(3)) s.c.has_scan = 1, s.c.less_sharp = r.upto(300), s.c.less_flat = r.upto(700), s.c.outliers = r.upto(200);
  int ring = 0, ar = 0, gf = 0, gl = 0;
  if (i == 1) ar = 3;
  if (i == 2) ar = 1;
  if (i == 3) ring = kWindow;
  if (i == 4) gf = 7, gl = 0;
  if (i == 5) gf = 70, gl = kMaxLoops;
  if (rnd && (s.modules & LINS_SNAP_RING)) ring = r.upto(kWindow);
  if (rnd && (s.modules & LINS_SNAP_ARCHIVE)) ar = r.upto(12);
  if (rnd && (s.modules & LINS_SNAP_GRAPH)) gf = r.upto(20), gl = gf >= 2 ? r.upto(6) : 0;
  for (int k = 0; k < ring; ++k) s.ring.push_back(frame(r, r.upto(40), r.upto(200), r.upto(30)));
  for (int k = 0; k < ar; ++k) {
    if (i == 1) s.ar.push_back(frame(r, 0, 0, 0));
    else if (i == 2) s.ar.push_back(frame(r, 17, 130, 0));
    else s.ar.push_back(r.upto(5) ? frame(r, r.upto(40), r.upto(600), r.upto(30)) : frame(r, 0, 0, 0));
  }
  for (int k = 0; k < gl; ++k) {
    lins_snapshot_loop L;
    std::memset(&L, 0, sizeof L);
    for (double& z : L.Z) z = (double)r.upto(1000) / 500.0 - 1.0;
    L.var = 0.3, L.latest = 1 + r.upto(gf - 2), L.closest = L.latest - 1 - r.upto(L.latest - 1);
    s.loops.push_back(L);
  }
  if ((s.modules & LINS_SNAP_MAP_POSE) && ar)
    for (int k = r.upto(ar); k > 0; --k) s.surround.push_back(r.upto(ar - 1));
  s.c.ring_frames = ring, s.c.archive_frames = ar, s.c.graph_frames = gf, s.c.graph_loops = gl, s.c.graph_up_frames = gl ? r.upto(gf) : 0;
  s.c.surround = (int32_t)s.surround.size();
  for (const auto& f : s.ring) s.c.ring_points += total_of(f);
  for (const auto& f : s.ar) s.c.archive_points += total_of(f);
  return s;
}

struct Blob {
  std::unique_ptr<char[]> mem;  // exactly `bytes` bytes
  uint64_t bytes = 0;
  lins_snapshot_dirent dir[LINS_SNAP_SECTIONS];
};

Blob exact_copy(const char* p, uint64_t bytes) {
  Blob b;
  b.mem.reset(new char[bytes ? bytes : 1]), b.bytes = bytes;
  if (bytes) std::memcpy(b.mem.get(), p, bytes);
  return b;
}

Blob build(const Set& s) {
  Blob b;
  REQUIRE(lins_host_snapshot_layout(s.modules, &s.c, b.dir, &b.bytes) == LINS_OK);
  b.mem.reset(new char[b.bytes]);
  Rng r{0xb10bull + b.bytes};
  for (uint64_t i = 0; i < b.bytes; ++i) b.mem[i] = (char)r.next();  // (padding too: seal zeroes it)
  char* m = b.mem.get();
  lins_snapshot_stream_rec rec;
  std::memset(&rec, 0, sizeof rec);
  rec.status = 3, rec.map_last_time = 12.5;
  std::memcpy(m + b.dir[LINS_SNAP_SEC_STREAM_REC].offset, &rec, sizeof rec);
  if (!s.surround.empty()) std::memcpy(m + b.dir[LINS_SNAP_SEC_SURROUND].offset, s.surround.data(), 4 * s.surround.size());
  if (!s.ring.empty()) std::memcpy(m + b.dir[LINS_SNAP_SEC_RING_META].offset, s.ring.data(), sizeof(lins_snapshot_frame) * s.ring.size());
  if (!s.ar.empty()) std::memcpy(m + b.dir[LINS_SNAP_SEC_AR_META].offset, s.ar.data(), sizeof(lins_snapshot_frame) * s.ar.size());
  if (!s.loops.empty())
    std::memcpy(m + b.dir[LINS_SNAP_SEC_PG_HOST].offset + 216ull * (uint64_t)s.c.graph_frames, s.loops.data(), sizeof(lins_snapshot_loop) * s.loops.size());
  REQUIRE(lins_host_snapshot_seal(m, b.bytes - 1, s.modules, &s.c, &s.facts) == LINS_E_CAPACITY);
  REQUIRE(lins_host_snapshot_seal(m, b.bytes, s.modules, &s.c, &s.facts) == LINS_OK);
  return b;
}

lins_snapshot_limits exact_limits(const Set& s) {
  lins_snapshot_limits l;
  std::memset(&l, 0, sizeof l);
  l.modules = s.modules;
  l.less_sharp_max = s.c.less_sharp, l.less_flat_max = s.c.less_flat, l.outlier_max = s.c.outliers;
  l.ring_window = s.c.ring_frames;
  for (const auto& f : s.ring) l.ring_max_pts = total_of(f) > l.ring_max_pts ? total_of(f) : l.ring_max_pts;
  l.archive_frames = s.c.archive_frames, l.archive_points = s.c.archive_points;
  l.graph_frames = s.c.graph_frames, l.graph_loops = s.c.graph_loops, l.surround_max = s.c.surround;
  return l;
}

int check(const Blob& b, const lins_snapshot_facts* f = nullptr, const lins_snapshot_limits* l = nullptr, lins_snapshot_info* out = nullptr) {
  return lins_host_snapshot_check(b.mem.get(), b.bytes, f, l, out);
}

void roundtrip(const Set& s) {
  Blob b = build(s);
  REQUIRE(b.bytes % 16 == 0);
  uint64_t at = lins_snap::kPayloadAt;
  for (int k = 0; k < LINS_SNAP_SECTIONS; ++k) {  // the directory: in order, aligned, back to back, the units of the section's kind
    REQUIRE(b.dir[k].id == (uint32_t)k && b.dir[k].offset == at && at % 16 == 0);
    REQUIRE(b.dir[k].unit == (k < LINS_SNAP_FIRST_DEVICE_SEC ? 1u : k < LINS_SNAP_FIRST_UNIT8_SEC ? 16u : 8u));
    REQUIRE(b.dir[k].bytes % b.dir[k].unit == 0);
    for (uint64_t i = b.dir[k].offset + b.dir[k].bytes; i < b.dir[k].offset + lins_snap::pad16(b.dir[k].bytes); ++i) REQUIRE(b.mem[i] == 0);
    at += lins_snap::pad16(b.dir[k].bytes);
  }
  REQUIRE(at == b.bytes);
  lins_snapshot_info h;
  REQUIRE(lins_host_snapshot_info(b.mem.get(), b.bytes, &h) == LINS_OK);
  REQUIRE(h.magic == LINS_SNAPSHOT_MAGIC && h.version == 1 && h.total_bytes == b.bytes && h.modules == s.modules);
  REQUIRE(std::memcmp(&h.counts, &s.c, sizeof s.c) == 0 && std::memcmp(&h.facts, &s.facts, sizeof s.facts) == 0);
  REQUIRE(check(b, &s.facts) == LINS_OK);
  lins_snapshot_facts other = s.facts;
  other.params.num_iter += 1;
  REQUIRE(check(b, &other) == LINS_E_STATE);
  // the same content sealed again gives the same bytes (canonical: nothing but the content goes into the blob)
  Blob again = build(s);
  REQUIRE(again.bytes == b.bytes && std::memcmp(again.mem.get(), b.mem.get(), b.bytes) == 0);
  // counts no blob has
  lins_snapshot_counts bad = s.c;
  bad.less_flat = -1;
  REQUIRE(lins_host_snapshot_layout(s.modules, &bad, nullptr, nullptr) == LINS_E_ARG);
  REQUIRE(lins_host_snapshot_layout(s.modules & ~LINS_SNAP_STREAM, &s.c, nullptr, nullptr) == LINS_E_ARG);
}

// every field of the header: (offset, size)
std::vector<std::pair<int, int>> header_fields() {
  std::vector<std::pair<int, int>> f = {{0, 8}, {8, 4}, {12, 4}, {16, 8}, {24, 8}, {32, 4}, {36, 4}};
  int at = 40;
  for (int k = 0; k < 6; ++k) f.push_back({at, 4}), at += 4;   // counts
  for (int k = 0; k < 2; ++k) f.push_back({at, 8}), at += 8;
  for (int k = 0; k < 4; ++k) f.push_back({at, 4}), at += 4;
  for (int k = 0; k < 4; ++k) f.push_back({at, 4}), at += 4;   // facts: lins_params
  for (int k = 0; k < 4; ++k) f.push_back({at, 8}), at += 8;
  for (int k = 0; k < 25; ++k) f.push_back({at, 8}), at += 8;  // lins_boot_params
  for (int k = 0; k < 4; ++k) f.push_back({at, 4}), at += 4;
  f.push_back({at, 8}), at += 8;
  for (int k = 0; k < 2; ++k) f.push_back({at, 4}), at += 4;
  f.push_back({at, 8}), at += 8;  // header_checksum
  if (at != (int)sizeof(lins_snapshot_info)) std::exit(3);
  return f;
}

void corrupt(const Set& s) {
  const Blob b = build(s);
  REQUIRE(check(b) == LINS_OK);
  auto with = [&](uint64_t off, int size, uint64_t value) {
    Blob c = exact_copy(b.mem.get(), b.bytes);
    std::memcpy(c.mem.get() + off, &value, (size_t)size);
    return check(c);
  };
  for (const auto& f : header_fields()) {
    uint64_t v = 0;
    std::memcpy(&v, b.mem.get() + f.first, (size_t)f.second);
    const uint64_t mask = f.second == 8 ? ~0ull : 0xffffffffull;
    for (uint64_t w : {(uint64_t)0, (v + 1) & mask, (v - 1) & mask, mask, mask >> 1})  // (mask >> 1: the signed types' maximum)
      if (w != v) REQUIRE(with((uint64_t)f.first, f.second, w) == LINS_E_INPUT);
  }
  for (int k = 0; k < LINS_SNAP_SECTIONS; ++k)
    for (int field = 0; field < 2; ++field)  // the entry's offset, its size
      for (long long d : {-16ll, -1ll, 1ll, 16ll}) {
        const uint64_t off = sizeof(lins_snapshot_info) + (size_t)k * sizeof(lins_snapshot_dirent) + 8 + 8 * (size_t)field;
        const uint64_t v = field ? b.dir[k].bytes : b.dir[k].offset;
        REQUIRE(with(off, 8, v + (uint64_t)d) == LINS_E_INPUT);
      }
  std::vector<uint64_t> cuts = {0, 1, sizeof(lins_snapshot_info), lins_snap::kPayloadAt, b.bytes};
  for (int k = 0; k < LINS_SNAP_SECTIONS; ++k) cuts.push_back(b.dir[k].offset), cuts.push_back(b.dir[k].offset + b.dir[k].bytes);
  for (uint64_t cut : cuts)
    for (long long d : {-1ll, 0ll, 1ll}) {
      const long long n = (long long)cut + d;
      if (n < 0 || (uint64_t)n >= b.bytes) continue;
      Blob c = exact_copy(b.mem.get(), (uint64_t)n);
      REQUIRE(check(c) == LINS_E_INPUT);
    }
  Rng r{0xf11bull + b.bytes};
  for (int k = 0; k < 10; ++k) {
    const uint64_t span = b.bytes - lins_snap::kPayloadAt;
    const uint64_t at = lins_snap::kPayloadAt + (k == 0 ? 0 : k == 1 ? span - 1 : r.next() % span);
    Blob c = exact_copy(b.mem.get(), b.bytes);
    c.mem[at] = (char)(c.mem[at] ^ (1 << (k % 8)));
    REQUIRE(check(c) == LINS_E_INPUT);
  }
  // records that contradict the counts behind a right checksum: a frame's size, a loop's frame, a surround id
  auto resealed = [&](int sec, uint64_t off, int32_t value) {
    Blob c = exact_copy(b.mem.get(), b.bytes);
    std::memcpy(c.mem.get() + b.dir[sec].offset + off, &value, 4);
    REQUIRE(lins_host_snapshot_seal(c.mem.get(), c.bytes, s.modules, &s.c, &s.facts) == LINS_OK);
    return check(c);
  };
  if (s.c.ring_frames) REQUIRE(resealed(LINS_SNAP_SEC_RING_META, 4, s.ring[0].n[1] + 1) == LINS_E_INPUT);
  if (s.c.archive_frames) REQUIRE(resealed(LINS_SNAP_SEC_AR_META, 0, -1) == LINS_E_INPUT);
  if (s.c.graph_loops) REQUIRE(resealed(LINS_SNAP_SEC_PG_HOST, 216ull * (uint64_t)s.c.graph_frames + 104, s.c.graph_frames) == LINS_E_INPUT);
  if (s.c.surround) REQUIRE(resealed(LINS_SNAP_SEC_SURROUND, 0, s.c.archive_frames) == LINS_E_INPUT);
}

void capacity(const Set& s) {
  const Blob b = build(s);
  const lins_snapshot_limits exact = exact_limits(s);
  REQUIRE(check(b, &s.facts, &exact) == LINS_OK);
  int32_t lins_snapshot_limits::*ints[] = {&lins_snapshot_limits::less_sharp_max, &lins_snapshot_limits::less_flat_max, &lins_snapshot_limits::outlier_max,
                                           &lins_snapshot_limits::ring_window,    &lins_snapshot_limits::archive_frames, &lins_snapshot_limits::graph_frames,
                                           &lins_snapshot_limits::graph_loops,    &lins_snapshot_limits::surround_max};
  for (auto p : ints) {
    lins_snapshot_limits l = exact;
    l.*p -= 1;
    REQUIRE(check(b, &s.facts, &l) == LINS_E_CAPACITY);
    l.*p += 2;
    REQUIRE(check(b, &s.facts, &l) == LINS_OK);
  }
  lins_snapshot_limits l = exact;
  l.archive_points -= 1;
  REQUIRE(check(b, &s.facts, &l) == LINS_E_CAPACITY);
  if (s.c.ring_frames) {  // one point less than the ring's largest frame
    l = exact, l.ring_max_pts -= 1;
    REQUIRE(check(b, &s.facts, &l) == LINS_E_CAPACITY);
  }
  for (uint32_t bit = 1; bit < 256; bit <<= 1)
    if (s.modules & bit) {  // a module the destination lacks
      l = exact, l.modules &= ~bit;
      REQUIRE(check(b, &s.facts, &l) == LINS_E_STATE);
    }
}

// the module side of a snapshot as a context would place it: key frames interleaved with other slots' (gaps of 0 .. 50
// points), the ring at a random head, rows of slot `row`
void plan(const Set& s, int set) {
  Rng r{0x91a2ull + (uint64_t)set};
  const int row = r.upto(6), max_pts = 900;
  std::vector<int64_t> ring_off, ar_off;
  std::vector<int32_t> ring_n, ar_n;
  const int head = r.upto(kWindow - 1);
  for (size_t i = 0; i < s.ring.size(); ++i) ring_off.push_back(((int64_t)row * kWindow + (head + (int)i) % kWindow) * max_pts), ring_n.push_back(total_of(s.ring[i]));
  int64_t at = r.upto(100);
  for (const auto& f : s.ar) ar_off.push_back(at), ar_n.push_back(total_of(f)), at += total_of(f) + (r.upto(2) ? r.upto(50) : 0);
  lins_snapshot_place p;
  std::memset(&p, 0, sizeof p);
  p.row = row, p.scan_off[0] = (int64_t)row * 4000 + 768, p.scan_off[1] = p.scan_off[0] + 2000, p.outl_off = (int64_t)row * 500;
  p.graph_off = (int64_t)row * 80 * 12;
  p.ring_off = ring_off.data(), p.ring_n = ring_n.data(), p.ar_off = ar_off.data(), p.ar_n = ar_n.data();
  int64_t units[LINS_SNAP_BUFFERS] = {7 * 4000, 7 * 500, 7ll * kWindow * max_pts, at, 7 * 19, 7 * 324, 7 * 144, 7 * 16, 7 * 19, 7 * 17, 7 * 11, 7 * 14, 7 * 80 * 12};
  lins_snapshot_dirent dir[LINS_SNAP_SECTIONS];
  uint64_t total = 0;
  REQUIRE(lins_host_snapshot_layout(s.modules, &s.c, dir, &total) == LINS_OK);
  const uint64_t dev_at = dir[LINS_SNAP_FIRST_DEVICE_SEC].offset, stg_base = 16ull * (uint64_t)r.upto(9), stg_bytes = stg_base + total - dev_at;
  const long long n = lins_host_snapshot_plan(s.modules, &s.c, &p, stg_base, nullptr, 0);
  REQUIRE(n >= 0);
  std::vector<lins_snapshot_segment> segs((size_t)n + 1);
  REQUIRE(lins_host_snapshot_plan(s.modules, &s.c, &p, stg_base, segs.data(), n) == n);
  segs.resize((size_t)n);
  REQUIRE(lins_host_snapshot_segments_ok(n, segs.data(), units, stg_bytes) == LINS_OK);
  // the three invariants, by marking: every unit of a module buffer at most once and inside the buffer; every byte of
  // the device sections exactly once, no byte of their padding, nothing in front of stg_base
  std::vector<std::vector<char>> mod(LINS_SNAP_BUFFERS);
  for (int k = 0; k < LINS_SNAP_BUFFERS; ++k) mod[k].assign((size_t)units[k], 0);
  std::vector<char> stg((size_t)stg_bytes, 0);
  for (const auto& g : segs) {
    REQUIRE(g.buffer >= 0 && g.buffer < LINS_SNAP_BUFFERS && g.units >= 1 && g.unit == (g.buffer < LINS_SNAP_FIRST_UNIT8_BUF ? 16 : 8));
    REQUIRE(g.buf_off >= 0 && g.buf_off + g.units <= units[g.buffer]);
    for (int64_t i = 0; i < g.units; ++i) REQUIRE(!mod[g.buffer][(size_t)(g.buf_off + i)]++);
    REQUIRE(g.stg_off >= 0 && (uint64_t)(g.stg_off + g.units) * (uint64_t)g.unit <= stg_bytes);
    for (int64_t i = g.stg_off * g.unit; i < (g.stg_off + g.units) * g.unit; ++i) REQUIRE(!stg[(size_t)i]++);
  }
  for (uint64_t i = 0; i < stg_base; ++i) REQUIRE(!stg[i]);
  for (int k = LINS_SNAP_FIRST_DEVICE_SEC; k < LINS_SNAP_SECTIONS; ++k) {
    const uint64_t o = stg_base + dir[k].offset - dev_at;
    for (uint64_t i = 0; i < lins_snap::pad16(dir[k].bytes); ++i) REQUIRE(stg[o + i] == (i < dir[k].bytes ? 1 : 0));
  }
  // what segments_ok refuses: a segment twice, a buffer one unit short, a staging buffer one byte short
  if (n) {
    std::vector<lins_snapshot_segment> twice = segs;
    twice.push_back(segs[(size_t)r.upto((int)n - 1)]);
    REQUIRE(lins_host_snapshot_segments_ok(n + 1, twice.data(), units, stg_bytes) == LINS_E_ARG);
    const lins_snapshot_segment& g = segs[(size_t)r.upto((int)n - 1)];
    int64_t end = 0;
    for (const auto& q : segs)
      if (q.buffer == g.buffer) end = q.buf_off + q.units > end ? q.buf_off + q.units : end;
    int64_t shorter[LINS_SNAP_BUFFERS];
    std::memcpy(shorter, units, sizeof units);
    shorter[g.buffer] = end - 1;
    REQUIRE(lins_host_snapshot_segments_ok(n, segs.data(), shorter, stg_bytes) == LINS_E_ARG);
    shorter[g.buffer] = end;
    REQUIRE(lins_host_snapshot_segments_ok(n, segs.data(), shorter, stg_bytes) == LINS_OK);
    uint64_t stg_end = 0;
    for (const auto& q : segs) stg_end = (uint64_t)((q.stg_off + q.units) * q.unit) > stg_end ? (uint64_t)((q.stg_off + q.units) * q.unit) : stg_end;
    REQUIRE(lins_host_snapshot_segments_ok(n, segs.data(), units, stg_end - 1) == LINS_E_ARG);
  }
  // neighbouring key frames that are neighbours in the arena are one segment: appended frames (a restore) are one run
  if (s.c.archive_points) {
    int64_t run = 1000;
    for (size_t i = 0; i < ar_off.size(); ++i) ar_off[i] = run, run += ar_n[i];
    units[LINS_SNAP_BUF_ARENA] = run;
    std::vector<lins_snapshot_segment> v(4);
    lins_snapshot_counts only{};  // (the archive's counts alone)
    only.archive_frames = s.c.archive_frames, only.archive_points = s.c.archive_points;
    const long long m = lins_host_snapshot_plan(LINS_SNAP_STREAM | LINS_SNAP_ARCHIVE, &only, &p, 0, v.data(), 4);
    REQUIRE(m == 1 && v[0].buffer == LINS_SNAP_BUF_ARENA && v[0].buf_off == 1000 && v[0].units == s.c.archive_points);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what != "roundtrip" && what != "corrupt" && what != "capacity" && what != "plan") return 2;
  bool fresh = false, empty_frames = false, full_ring = false, no_loops = false, max_loops = false;
  for (int i = 0; i < kSets; ++i) {
    g_set = i;
    const Set s = make_set(i);
    fresh = fresh || (!s.c.has_scan && !s.c.archive_frames && !s.c.ring_frames && !s.c.graph_frames);
    for (const auto& f : s.ar) empty_frames = empty_frames || total_of(f) == 0;
    full_ring = full_ring || s.c.ring_frames == kWindow;
    no_loops = no_loops || (s.c.graph_frames && !s.c.graph_loops);
    max_loops = max_loops || s.c.graph_loops == kMaxLoops;
    if (what == "roundtrip") roundtrip(s);
    if (what == "corrupt") corrupt(s);
    if (what == "capacity") capacity(s);
    if (what == "plan") plan(s, i);
  }
  g_set = -1;
  REQUIRE(fresh && empty_frames && full_ring && no_loops && max_loops);
  std::printf("ok %s\n", what.c_str());
  return 0;
}
