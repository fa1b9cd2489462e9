// lins_snapshot_capi.hip — snapshot and restore of streams in the C ABI (include/lins_snapshot.h): a stream is a slot of
// every initialised module (snapshot.h: the modules' describe / check / place / apply functions live in their own
// files), the blob's format and the copy plan are host/snapshot_format.h, the copies run in snapshot_kernels.hip.
//   snapshot  describe every entry -> sizes against caps -> plan -> one table upload, two launches (16- and 8-byte
//             units), one copy of the staging buffer to pinned memory, one synchronisation -> the blobs are written
//   restore   check every entry (format, facts, the slot fresh in every module, limits) -> plan -> segments_ok -> one
//             upload of the staging buffer, one table upload, two launches, one synchronisation -> the host fields
// No kernel is launched and no field written before every entry of the call has passed.
#include "../../include/lins_snapshot.h"

#include <climits>

#include "lins_ctx.h"
#include "local_map.h"
#include "snapshot.h"

using namespace lins;

namespace {

size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// a stream is in range, and named once, in every initialised module (as lins_streams_retire asks)
int streams_list_check(lins_ctx* ctx, int n, const int32_t* streams) {
  const int sizes[5] = {ctx->st.n, streams_map_streams(ctx), local_map_slots(ctx), archive_slots(ctx), pose_graph_slots(ctx)};
  for (int limit : sizes)
    if (limit > 0)
      if (int rc = release_list_check(n, streams, limit)) return rc;
  return LINS_OK;
}

SnapContext context_of(lins_ctx* ctx) {
  SnapContext c;
  std::memset(&c.facts, 0, sizeof c.facts);
  streams_snapshot_context(ctx, c);
  streams_map_snapshot_context(ctx, c);
  local_map_snapshot_context(ctx, c);
  archive_snapshot_context(ctx, c);
  pose_graph_snapshot_context(ctx, c);
  return c;
}

// the table of a launch — bases | segments | (segment, tile) entries of the 16-byte units | of the 8-byte units — and the
// staging buffers, grown; nothing is queued
struct Table {
  size_t o_segs = 0, o_t16 = 0, o_t8 = 0, bytes = 0;
  int n16 = 0, n8 = 0;
};
int table_build(lins_ctx* ctx, const SnapContext& c, const std::vector<lins_snapshot_segment>& segs, uint64_t stg_bytes, Table& tb) {
  if (!lins_snap::segments_ok((long long)segs.size(), segs.data(), c.units, stg_bytes)) return LINS_E_STATE;  // (the plan is the library's own)
  for (const lins_snapshot_segment& g : segs)
    if (!c.base[g.buffer]) return LINS_E_STATE;
  std::vector<int2> t16, t8;
  for (size_t i = 0; i < segs.size(); ++i) {
    const long long nt = (segs[i].units + kLmTile - 1) / kLmTile;
    std::vector<int2>& t = segs[i].unit == 16 ? t16 : t8;
    if (i > (size_t)INT_MAX || nt > INT_MAX || t.size() + (size_t)nt > (size_t)INT_MAX) return LINS_E_CAPACITY;
    for (long long k = 0; k < nt; ++k) t.push_back(make_int2((int)i, (int)k));
  }
  tb.o_segs = align64(sizeof c.base), tb.o_t16 = align64(tb.o_segs + segs.size() * sizeof(lins_snapshot_segment));
  tb.o_t8 = align64(tb.o_t16 + t16.size() * sizeof(int2)), tb.bytes = align64(tb.o_t8 + t8.size() * sizeof(int2));
  tb.n16 = (int)t16.size(), tb.n8 = (int)t8.size();
  auto& sn = ctx->snap;
  BUF_TRY(ctx, sn.h_tab.grow(tb.bytes));
  BUF_TRY(ctx, sn.d_tab.grow(tb.bytes));
  BUF_TRY(ctx, sn.h_stage.grow((size_t)stg_bytes));
  BUF_TRY(ctx, sn.d_stage.grow((size_t)stg_bytes));
  std::memcpy(sn.h_tab, c.base, sizeof c.base);
  if (!segs.empty()) std::memcpy(sn.h_tab + tb.o_segs, segs.data(), segs.size() * sizeof(lins_snapshot_segment));
  if (!t16.empty()) std::memcpy(sn.h_tab + tb.o_t16, t16.data(), t16.size() * sizeof(int2));
  if (!t8.empty()) std::memcpy(sn.h_tab + tb.o_t8, t8.data(), t8.size() * sizeof(int2));
  return LINS_OK;
}

int table_run(lins_ctx* ctx, const Table& tb, uint64_t stg_bytes, bool pack) {
  auto& sn = ctx->snap;
  hipStream_t st = ctx->stream;
  const lins_snapshot_segment* d_segs = (const lins_snapshot_segment*)(sn.d_tab + tb.o_segs);
  void* const* d_bases = (void* const*)sn.d_tab.get();
  if (!pack && stg_bytes) HIP_TRY(ctx, hipMemcpyAsync(sn.d_stage, sn.h_stage, (size_t)stg_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(sn.d_tab, sn.h_tab, tb.bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, st));
  if (pack) {
    launch_snap_pack(st, 16, tb.n16, d_segs, (const int2*)(sn.d_tab + tb.o_t16), d_bases, sn.d_stage);
    launch_snap_pack(st, 8, tb.n8, d_segs, (const int2*)(sn.d_tab + tb.o_t8), d_bases, sn.d_stage);
  } else {
    launch_snap_unpack(st, 16, tb.n16, d_segs, (const int2*)(sn.d_tab + tb.o_t16), d_bases, sn.d_stage);
    launch_snap_unpack(st, 8, tb.n8, d_segs, (const int2*)(sn.d_tab + tb.o_t8), d_bases, sn.d_stage);
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, st));
  if (pack && stg_bytes) HIP_TRY(ctx, hipMemcpyAsync(sn.h_stage, sn.d_stage, (size_t)stg_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(pack ? &sn.pack_ms : &sn.unpack_ms, ctx->ev0, ctx->ev1));
  return LINS_OK;
}

int describe_all(lins_ctx* ctx, const SnapContext& c, int n, const int32_t* streams, std::vector<SnapStream>& ss, std::vector<uint64_t>& total,
                 std::vector<uint64_t>& dev_at) {
  ss.assign((size_t)n, SnapStream{}), total.assign((size_t)n, 0), dev_at.assign((size_t)n, 0);
  for (int k = 0; k < n; ++k) {
    SnapStream& s = ss[k];
    if (int rc = streams_snapshot_describe(ctx, streams[k], s)) return rc;
    if (c.modules & LINS_SNAP_MAP_POSE)
      if (int rc = streams_map_snapshot_describe(ctx, streams[k], s)) return rc;
    if (c.modules & LINS_SNAP_RING)
      if (int rc = local_map_snapshot_describe(ctx, streams[k], s)) return rc;
    if (c.modules & LINS_SNAP_ARCHIVE)
      if (int rc = archive_snapshot_describe(ctx, streams[k], s)) return rc;
    if (c.modules & LINS_SNAP_GRAPH)
      if (int rc = pose_graph_snapshot_describe(ctx, streams[k], s)) return rc;
    s.bind();
    if (lins_snap::layout(s.modules, s.counts, nullptr, &total[k], &dev_at[k])) return LINS_E_STATE;
  }
  return LINS_OK;
}

int entry_checks(lins_ctx* ctx, int n, const int32_t* streams) {
  if (!ctx || n < 0 || (n && !streams)) return LINS_E_ARG;
  if (ctx->st.n <= 0 || ctx->st.failed) return LINS_E_STATE;
  return streams_list_check(ctx, n, streams);
}

}  // namespace

extern "C" {

int lins_streams_snapshot_size(lins_ctx* ctx, int n, const int32_t* streams, uint64_t* bytes) {
  if (int rc = entry_checks(ctx, n, streams)) return rc;
  if (n && !bytes) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  const SnapContext c = context_of(ctx);
  std::vector<SnapStream> ss;
  std::vector<uint64_t> total, dev_at;
  if (int rc = describe_all(ctx, c, n, streams, ss, total, dev_at)) return rc;
  std::copy(total.begin(), total.end(), bytes);
  return LINS_OK;
}

int lins_streams_snapshot(lins_ctx* ctx, int n, const int32_t* streams, void* const* blobs, const uint64_t* caps, uint64_t* bytes) {
  if (int rc = entry_checks(ctx, n, streams)) return rc;
  if (n && (!blobs || !caps)) return LINS_E_ARG;
  for (int k = 0; k < n; ++k)
    if (!blobs[k]) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  if (int rc = ctx_quiesce(ctx)) return rc;
  const SnapContext c = context_of(ctx);
  std::vector<SnapStream> ss;
  std::vector<uint64_t> total, dev_at;
  if (int rc = describe_all(ctx, c, n, streams, ss, total, dev_at)) return rc;
  bool fits = true;
  for (int k = 0; k < n; ++k) {
    if (bytes) bytes[k] = total[k];
    fits = fits && caps[k] >= total[k];
  }
  if (!fits) return LINS_E_CAPACITY;
  std::vector<lins_snapshot_segment> segs;
  std::vector<uint64_t> stg_at((size_t)n);
  uint64_t stg_bytes = 0;
  for (int k = 0; k < n; ++k) {
    stg_at[k] = stg_bytes, stg_bytes += total[k] - dev_at[k];
    if (lins_snap::plan(ss[k].modules, ss[k].counts, ss[k].place, stg_at[k], segs)) return LINS_E_STATE;
  }
  Table tb;
  if (int rc = table_build(ctx, c, segs, stg_bytes, tb)) return rc;
  if (int rc = table_run(ctx, tb, stg_bytes, true)) return rc;
  ctx->snap.bytes = stg_bytes, ctx->snap.segments = (int)segs.size();
  for (int k = 0; k < n; ++k) {
    char* b = (char*)blobs[k];
    lins_snapshot_dirent dir[LINS_SNAP_SECTIONS];
    lins_snap::layout(ss[k].modules, ss[k].counts, dir, nullptr);
    std::memset(b, 0, (size_t)dev_at[k]);
    for (int sec = 0; sec < LINS_SNAP_FIRST_DEVICE_SEC; ++sec)
      if (!ss[k].host[sec].empty()) std::memcpy(b + dir[sec].offset, ss[k].host[sec].data(), std::min<size_t>(ss[k].host[sec].size(), dir[sec].bytes));
    if (total[k] > dev_at[k]) std::memcpy(b + dev_at[k], ctx->snap.h_stage + stg_at[k], (size_t)(total[k] - dev_at[k]));
    if (lins_snap::seal(b, caps[k], ss[k].modules, ss[k].counts, c.facts)) return LINS_E_STATE;
  }
  return LINS_OK;
}

int lins_streams_restore(lins_ctx* ctx, int n, const int32_t* streams, const void* const* blobs, const uint64_t* bytes) {
  if (int rc = entry_checks(ctx, n, streams)) return rc;
  if (n && (!blobs || !bytes)) return LINS_E_ARG;
  for (int k = 0; k < n; ++k)
    if (!blobs[k]) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  if (int rc = ctx_quiesce(ctx)) return rc;
  SnapContext c = context_of(ctx);
  // (the filter's rows and the odometry records are allocated on first use: a context always has room for them)
  const uint32_t offered = c.modules | LINS_SNAP_FILTER | LINS_SNAP_ODOM;
  std::vector<SnapView> vs((size_t)n);
  long long arena_claimed = 0;
  uint32_t carried = 0;
  for (int k = 0; k < n; ++k) {
    SnapView& v = vs[k];
    v.blob = (const char*)blobs[k];
    if (int rc = lins_snap::check(blobs[k], bytes[k], &c.facts, nullptr, &v.info)) return rc;
    std::memcpy(v.dir, v.blob + sizeof v.info, sizeof v.dir);
    // the slot is what init / release leave in every module of this context, carried by the blob or not
    lins_snapshot_limits lim;
    std::memset(&lim, 0, sizeof lim);
    lim.modules = offered;
    if (int rc = streams_restore_check(ctx, streams[k], lim)) return rc;
    if (c.modules & LINS_SNAP_MAP_POSE)
      if (int rc = streams_map_restore_check(ctx, streams[k], lim)) return rc;
    if (c.modules & LINS_SNAP_RING)
      if (int rc = local_map_restore_check(ctx, streams[k], lim)) return rc;
    if (c.modules & LINS_SNAP_ARCHIVE)
      if (int rc = archive_restore_check(ctx, streams[k], lim)) return rc;
    if (c.modules & LINS_SNAP_GRAPH)
      if (int rc = pose_graph_restore_check(ctx, streams[k], lim)) return rc;
    lim.archive_points -= arena_claimed;  // (the entries in front of this one of the same call)
    if (int rc = lins_snap::limits_check(v.blob, v.info, v.dir, lim)) return rc;
    arena_claimed += v.info.counts.archive_points;
    carried |= v.info.modules;
  }
  if (int rc = streams_restore_prepare(ctx, carried)) return rc;
  c = context_of(ctx);
  long long arena_at = 0;
  if (c.modules & LINS_SNAP_ARCHIVE) lins_archive_usage(ctx, &arena_at, nullptr);
  std::vector<SnapStream> ss((size_t)n);
  std::vector<lins_snapshot_segment> segs;
  std::vector<uint64_t> stg_at((size_t)n), dev_at((size_t)n);
  uint64_t stg_bytes = 0;
  for (int k = 0; k < n; ++k) {
    SnapStream& s = ss[k];
    const SnapView& v = vs[k];
    s.modules = v.info.modules, s.counts = v.info.counts;
    streams_restore_place(ctx, streams[k], v, s);
    if (s.modules & LINS_SNAP_RING) local_map_restore_place(ctx, streams[k], v, s);
    if (s.modules & LINS_SNAP_ARCHIVE) archive_restore_place(ctx, streams[k], v, s, &arena_at);
    if (s.modules & LINS_SNAP_GRAPH) pose_graph_restore_place(ctx, streams[k], v, s);
    s.bind();
    dev_at[k] = v.dir[LINS_SNAP_FIRST_DEVICE_SEC].offset;
    stg_at[k] = stg_bytes, stg_bytes += v.info.total_bytes - dev_at[k];
    if (lins_snap::plan(s.modules, s.counts, s.place, stg_at[k], segs)) return LINS_E_STATE;
  }
  Table tb;
  if (int rc = table_build(ctx, c, segs, stg_bytes, tb)) return rc;
  for (int k = 0; k < n; ++k)
    if (vs[k].info.total_bytes > dev_at[k]) std::memcpy(ctx->snap.h_stage + stg_at[k], vs[k].blob + dev_at[k], (size_t)(vs[k].info.total_bytes - dev_at[k]));
  if (int rc = table_run(ctx, tb, stg_bytes, false)) return rc;
  ctx->snap.bytes = stg_bytes, ctx->snap.segments = (int)segs.size();
  for (int k = 0; k < n; ++k) {
    const SnapView& v = vs[k];
    streams_restore_apply(ctx, streams[k], v);
    if (v.info.modules & LINS_SNAP_MAP_POSE) streams_map_restore_apply(ctx, streams[k], v);
    if (v.info.modules & LINS_SNAP_RING) local_map_restore_apply(ctx, streams[k], v);
    if (v.info.modules & LINS_SNAP_ARCHIVE) archive_restore_apply(ctx, streams[k], v, ss[k]);
    if (v.info.modules & LINS_SNAP_GRAPH)
      if (int rc = pose_graph_restore_apply(ctx, streams[k], v)) return rc;
  }
  return LINS_OK;
}

int lins_streams_migrate(lins_ctx* src, int src_stream, lins_ctx* dst, int dst_stream) {
  if (!src || !dst || (src == dst && src_stream == dst_stream)) return LINS_E_ARG;
  const int32_t s = src_stream, d = dst_stream;
  if (int rc = entry_checks(dst, 1, &d)) return rc;
  uint64_t need = 0;
  if (int rc = lins_streams_snapshot_size(src, 1, &s, &need)) return rc;
  std::vector<uint64_t> mem((size_t)(need + 7) / 8);
  void* blob = mem.data();
  if (int rc = lins_streams_snapshot(src, 1, &s, &blob, &need, nullptr)) return rc;  // (reads only)
  const void* cblob = blob;
  if (int rc = lins_streams_restore(dst, 1, &d, &cblob, &need)) return rc;  // a refusal: both contexts are as they were
  return lins_streams_retire(src, 1, &s);
}

int lins_snapshot_info_get(const void* blob, uint64_t bytes, lins_snapshot_info* out) {
  if (!out) return LINS_E_ARG;
  return lins_snap::check(blob, bytes, nullptr, nullptr, out);
}

int lins_last_snapshot_stats(lins_ctx* ctx, float* pack_ms, float* unpack_ms, uint64_t* bytes, int32_t* segments) {
  if (!ctx) return LINS_E_ARG;
  if (pack_ms) *pack_ms = ctx->snap.pack_ms;
  if (unpack_ms) *unpack_ms = ctx->snap.unpack_ms;
  if (bytes) *bytes = ctx->snap.bytes;
  if (segments) *segments = ctx->snap.segments;
  return LINS_OK;
}

}  // extern "C"
