// snapshot.h — what the files behind include/lins_snapshot.h share, in the manner of lifecycle.h: every module exposes
//   context   its context-wide facts, what its slots offer, and its device buffers as the plan names them
//   describe  (snapshot) the counts, the host-only sections and the places of the device pieces of one slot — reads only
//   check     (restore) LINS_E_STATE unless the slot is what init / release leave; the slot's limits
//   place     (restore) where the blob's device pieces will lie — changes nothing
//   apply     (restore) the host fields, behind the unpack kernel — cannot refuse
// in the module's own file beside its *_release_apply, so that lins_streams_restore asks every module and the format's
// check for every entry of the call before a kernel is launched or a field written.  Context quiesced by the caller.
#pragma once
#include <vector>

#include "host/snapshot_format.h"
#include "lifecycle.h"

namespace lins {

struct SnapStream {  // one entry of a snapshot / restore call
  uint32_t modules = 0;
  lins_snapshot_counts counts{};
  lins_snapshot_place place{};
  std::vector<int64_t> ring_off, ar_off;
  std::vector<int32_t> ring_n, ar_n;
  std::vector<char> host[LINS_SNAP_FIRST_DEVICE_SEC];  // (snapshot) the host-only sections
  void bind() { place.ring_off = ring_off.data(), place.ring_n = ring_n.data(), place.ar_off = ar_off.data(), place.ar_n = ar_n.data(); }
  template <class T>
  T* host_section(int sec, size_t count) {
    host[sec].assign(count * sizeof(T), 0);
    return (T*)host[sec].data();
  }
};

struct SnapView {  // a checked blob
  const char* blob = nullptr;
  lins_snapshot_info info;
  lins_snapshot_dirent dir[LINS_SNAP_SECTIONS];
  const char* sec(int id) const { return blob + dir[id].offset; }
};

struct SnapContext {
  lins_snapshot_facts facts;
  uint32_t modules = 0;                      // initialised modules
  void* base[LINS_SNAP_BUFFERS] = {};        // device buffers (null: none)
  int64_t units[LINS_SNAP_BUFFERS] = {};     // their sizes in units
};

// lins_lifecycle_capi.hip: ctx->st — resident scan, outlier cloud, filter, bootstrap, odometry record
void streams_snapshot_context(lins_ctx* ctx, SnapContext& c);
int streams_snapshot_describe(lins_ctx* ctx, int stream, SnapStream& s);
int streams_restore_check(lins_ctx* ctx, int stream, lins_snapshot_limits& lim);
int streams_restore_prepare(lins_ctx* ctx, uint32_t modules);  // the lazily allocated rows a blob's modules need
void streams_restore_place(lins_ctx* ctx, int stream, const SnapView& v, SnapStream& s);
void streams_restore_apply(lins_ctx* ctx, int stream, const SnapView& v);
// lins_capi_streams.hip: a feature slot's resident clouds (points into the streams' arena; caps of the two clouds)
void streams_scan_place(int stream, int slot, int64_t off[2], int32_t caps[2], int64_t* slot_points);
// lins_streams_map_capi.hip
void streams_map_snapshot_context(lins_ctx* ctx, SnapContext& c);
int streams_map_snapshot_describe(lins_ctx* ctx, int stream, SnapStream& s);
int streams_map_restore_check(lins_ctx* ctx, int stream, lins_snapshot_limits& lim);
void streams_map_restore_apply(lins_ctx* ctx, int stream, const SnapView& v);
// lins_local_map_capi.hip
void local_map_snapshot_context(lins_ctx* ctx, SnapContext& c);
int local_map_snapshot_describe(lins_ctx* ctx, int slot, SnapStream& s);
int local_map_restore_check(lins_ctx* ctx, int slot, lins_snapshot_limits& lim);
void local_map_restore_place(lins_ctx* ctx, int slot, const SnapView& v, SnapStream& s);
void local_map_restore_apply(lins_ctx* ctx, int slot, const SnapView& v);
// lins_archive_capi.hip (arena_at: where this entry's frames are appended; advanced)
void archive_snapshot_context(lins_ctx* ctx, SnapContext& c);
int archive_snapshot_describe(lins_ctx* ctx, int slot, SnapStream& s);
int archive_restore_check(lins_ctx* ctx, int slot, lins_snapshot_limits& lim);
void archive_restore_place(lins_ctx* ctx, int slot, const SnapView& v, SnapStream& s, long long* arena_at);
void archive_restore_apply(lins_ctx* ctx, int slot, const SnapView& v, const SnapStream& s);
// lins_pose_graph_capi.hip
void pose_graph_snapshot_context(lins_ctx* ctx, SnapContext& c);
int pose_graph_snapshot_describe(lins_ctx* ctx, int slot, SnapStream& s);
int pose_graph_restore_check(lins_ctx* ctx, int slot, lins_snapshot_limits& lim);
void pose_graph_restore_place(lins_ctx* ctx, int slot, const SnapView& v, SnapStream& s);
int pose_graph_restore_apply(lins_ctx* ctx, int slot, const SnapView& v);  // (uploads the measurements: HIP errors)

}  // namespace lins
