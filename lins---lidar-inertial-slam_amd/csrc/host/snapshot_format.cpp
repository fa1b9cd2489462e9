// snapshot_format.cpp — liblins_host.so's exports of the snapshot blob's format and plan (host/snapshot_format.h,
// include/lins_snapshot.h).
#include "snapshot_format.h"

extern "C" {

int lins_host_snapshot_layout(uint32_t modules, const lins_snapshot_counts* counts, lins_snapshot_dirent* dir, uint64_t* total_bytes) {
  if (!counts) return LINS_E_ARG;
  return lins_snap::layout(modules, *counts, dir, total_bytes);
}

int lins_host_snapshot_seal(void* blob, uint64_t cap, uint32_t modules, const lins_snapshot_counts* counts, const lins_snapshot_facts* facts) {
  if (!counts || !facts) return LINS_E_ARG;
  return lins_snap::seal(blob, cap, modules, *counts, *facts);
}

int lins_host_snapshot_check(const void* blob, uint64_t bytes, const lins_snapshot_facts* facts, const lins_snapshot_limits* limits,
                             lins_snapshot_info* out) {
  return lins_snap::check(blob, bytes, facts, limits, out);
}

int lins_host_snapshot_info(const void* blob, uint64_t bytes, lins_snapshot_info* out) {
  if (!out) return LINS_E_ARG;
  return lins_snap::check(blob, bytes, nullptr, nullptr, out);
}

long long lins_host_snapshot_plan(uint32_t modules, const lins_snapshot_counts* counts, const lins_snapshot_place* place, uint64_t stg_base,
                                  lins_snapshot_segment* segs, long long cap) {
  if (!counts || !place || cap < 0 || (cap && !segs)) return LINS_E_ARG;
  std::vector<lins_snapshot_segment> v;
  if (int rc = lins_snap::plan(modules, *counts, *place, stg_base, v)) return rc;
  for (size_t i = 0; i < v.size() && (long long)i < cap; ++i) segs[i] = v[i];
  return (long long)v.size();
}

int lins_host_snapshot_segments_ok(long long n, const lins_snapshot_segment* segs, const int64_t* buf_units, uint64_t stg_bytes) {
  return lins_snap::segments_ok(n, segs, buf_units, stg_bytes) ? LINS_OK : LINS_E_ARG;
}

}  // extern "C"
