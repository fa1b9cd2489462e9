// lins_archive_capi.hip — C ABI of the key-frame archive (include/lins_map.h lins_archive_*): every key frame of a slot
// in one bump-allocated device arena, the host's list of frames (offset, counts, pose, trigonometry, time), the
// selection of frames (host/keyframe_select.h — the same inline code liblins_host.so exports), and the packing of an
// assembly into the jobs of archive_kernels.hip / local_map_kernels.hip.  Slots are released, and the arena compacted
// behind them, by lins_archive_release_slots (include/lins_lifecycle.h; archive_release_apply below).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lins_lifecycle.h"
#include "../../include/lins_map.h"
#include "host/arena_reclaim.h"
#include "host/keyframe_select.h"
#include "host/team_select.h"
#include "keyframe_archive.h"
#include "keypose_select_math.h"
#include "lifecycle.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "local_map.h"
#include "place.h"
#include "snapshot.h"

using namespace lins;
using lins_hostmap::cloud_ok;
using lins_hostmap::pose_ok;

namespace {

struct Archive {
  int n_slots = 0, max_frames = 0, chunk = kArScanChunk;
  long long max_points = 0, used = 0;
  DevBuf<float4> d_arena;
  std::vector<std::vector<ArFrame>> frames;  // [slot][id]
  // assembly arenas (grown, never shrunk)
  DevBuf<float4> d_stage, d_out;
  DevBuf<unsigned> d_ka, d_kb;  // (d_ka, d_kb, d_va, d_vb, d_starts: one group, d_ka answers)
  DevBuf<int> d_va, d_vb, d_starts, d_hist, d_tilecnt, d_csum;
  DevBuf<char> d_tab;  // (bytes)
  PinBuf<char> h_tab, h_states;
  // the last assembly
  bool built = false;
  unsigned long long serial = 0;  // assemblies started so far
  std::vector<long long> off;
  std::vector<lins_submap_info> info;
  std::vector<char> filtered;  // per entry: a VoxelGrid output (its info carries the 1 m box)
  float ms = 0.f;
  uint64_t points_in = 0;
  // the key-pose selection on the device (lins_keyposes_*): the mirror of the slots' key poses and times, frame id of slot
  // s at s * max_frames + id, current below stale_from[s]; one table up, one block of results down (pinned staging)
  DevBuf<float4> d_kp_pose;
  DevBuf<double> d_kp_time;
  std::vector<int> stale_from;  // [slot]
  DevBuf<char> d_kp_up, d_kp_down;  // (bytes)
  PinBuf<char> h_kp_up, h_kp_down;
  DevBuf<int> d_kp_scratch;
  int kp_mode = LINS_KEYPOSES_HOST, kp_host = 0;
  float kp_ms = 0.f;
  uint64_t kp_hits = 0;
  // the team selection (lins_keyposes_team_select_batch): the same mirror and staging; the last call
  int ts_host = 0;
  float ts_ms = 0.f;
  uint64_t ts_hits = 0;
  // the arena's compaction (lins_archive_release_slots): points per pass, the staging buffer of that many points
  // (allocated by the first staged pass), one table up (segments | blocks; pinned staging), the last compaction
  long long reclaim_chunk = kArReclaimChunk;
  DevBuf<float4> d_reclaim;
  DevBuf<char> d_rc_tab;  // (bytes)
  PinBuf<char> h_rc_tab;
  float rc_ms = 0.f;
  uint64_t rc_moved = 0;
  int rc_staged = 0, rc_direct = 0;
  // place recognition's descriptors (place.h, lins_place_*): a second derived mirror, current below place.described[s]
  PlaceStore place;
};

void archive_free(void* p) { delete (Archive*)p; }

Archive* archive_of(lins_ctx* ctx) {
  void** slot = map_slot(ctx, kSlotArchive, archive_free);
  if (!*slot) *slot = new Archive();
  return (Archive*)*slot;
}

void set_pose(ArFrame& f, const lins_key_pose& p) {  // updateTransformPointCloudSinCos (LM:612-624), as the local map's set_pose
  f.pose = p;
  const float t[9] = {std::cos(p.roll), std::sin(p.roll), std::cos(p.pitch), std::sin(p.pitch), std::cos(p.yaw), std::sin(p.yaw), p.x, p.y, p.z};
  std::memcpy(f.t, t, sizeof t);
}

size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// the mirror of the slot's key poses is out of date from frame `id` on (brought up by the next lins_keyposes_* call)
void stale_at(Archive* m, int slot, int id) { m->stale_from[slot] = std::min(m->stale_from[slot], id); }

// the slot's frames are other frames from now on: both mirrors start over (a descriptor depends on a frame's points only,
// so a changed pose — stale_at — or a moved block leaves it)
void mirrors_drop(Archive* m, int slot) {
  m->stale_from[slot] = 0;
  if (m->place.on) m->place.described[slot] = 0, m->place.team.drop_slot(slot);
}

std::vector<lins_key_pose> poses_of(const std::vector<ArFrame>& fr) {
  std::vector<lins_key_pose> p(fr.size());
  for (size_t i = 0; i < fr.size(); ++i) p[i] = fr[i].pose;
  return p;
}

}  // namespace

namespace lins {
int archive_view(lins_ctx* ctx, ArchiveView* v) {
  Archive* m = archive_of(ctx);
  if (!m->built) return LINS_E_STATE;
  v->d_out = m->d_out, v->n = (int)m->info.size(), v->off = m->off.data(), v->info = m->info.data(), v->filtered = m->filtered.data();
  v->serial = m->serial;
  return LINS_OK;
}
int archive_store(lins_ctx* ctx, ArchiveStore* v) {
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  v->d_arena = m->d_arena, v->n_slots = m->n_slots, v->chunk = m->chunk, v->frames = &m->frames;
  return LINS_OK;
}

int archive_slots(lins_ctx* ctx) { return archive_of(ctx)->n_slots; }

int archive_team_select_host(lins_ctx* ctx, int n_targets, const int32_t* slots, const float centre[3], float radius, float pose_leaf,
                             std::vector<int32_t>& pairs) {
  Archive* m = archive_of(ctx);
  pairs.clear();
  if (!m->n_slots) return LINS_E_STATE;
  if (n_targets < 0 || !lins_select::query_ok(centre, radius) || !lins_team_select::leaf_ok(pose_leaf)) return LINS_E_ARG;
  std::vector<std::vector<lins_key_pose>> keep((size_t)n_targets);
  std::vector<const lins_key_pose*> ptr((size_t)n_targets);
  std::vector<int32_t> cnt((size_t)n_targets);
  for (int t = 0; t < n_targets; ++t) {
    if (slots[t] < 0 || slots[t] >= m->n_slots) return LINS_E_ARG;
    keep[t] = poses_of(m->frames[slots[t]]);
    ptr[t] = keep[t].data(), cnt[t] = (int32_t)keep[t].size();
  }
  std::vector<lins_team_select::Pair> sel;
  const int rc = lins_team_select::select(n_targets, slots, ptr.data(), cnt.data(), centre, radius, pose_leaf, sel, nullptr);
  if (rc == lins_team_select::kDuplicate) return LINS_E_ARG;
  if (rc == lins_team_select::kTooManyCells) return LINS_E_CAPACITY;
  for (const lins_team_select::Pair& p : sel) pairs.push_back(p.slot), pairs.push_back(p.id);
  return LINS_OK;
}

ConsensusStore* archive_consensus(lins_ctx* ctx) { return &archive_of(ctx)->place.team.consensus; }

int archive_place(lins_ctx* ctx, ArchivePlace* v) {
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  v->store = &m->place, v->d_arena = m->d_arena, v->n_slots = m->n_slots, v->max_frames = m->max_frames, v->frames = &m->frames;
  return LINS_OK;
}

// The frames of the slots named go, the arena closes up behind them (host/arena_reclaim.h: the plan; archive_kernels.hip
// ar_reclaim_*: its passes).  One table upload in front, every pass queued back to back, one synchronisation behind;
// the host's records change only after that synchronisation.  Arguments checked by the caller, context quiesced.
int archive_release_apply(lins_ctx* ctx, int n, const int32_t* slots, long long* released) {
  Archive* m = archive_of(ctx);
  m->rc_ms = 0.f, m->rc_moved = 0, m->rc_staged = m->rc_direct = 0;
  if (released) *released = 0;
  if (n == 0) return LINS_OK;
  std::vector<char> drop((size_t)m->n_slots, 0);
  for (int k = 0; k < n; ++k) drop[slots[k]] = 1;
  // the arena's blocks in offset order: one per frame (pushes are appended, so a slot's frames ascend already)
  struct Ref {
    int slot, id;
  };
  std::vector<Ref> refs;
  for (int s = 0; s < m->n_slots; ++s)
    for (int i = 0; i < (int)m->frames[s].size(); ++i) refs.push_back(Ref{s, i});
  auto total_of = [](const ArFrame& f) { return (long long)f.n[0] + f.n[1] + f.n[2]; };
  std::sort(refs.begin(), refs.end(), [&](const Ref& a, const Ref& b) {  // (an empty frame shares its offset with the next one: it goes first)
    const ArFrame &fa = m->frames[a.slot][a.id], &fb = m->frames[b.slot][b.id];
    return fa.off != fb.off ? fa.off < fb.off : (total_of(fa) != 0) < (total_of(fb) != 0);
  });
  std::vector<lins_arena_block> blocks(refs.size());
  long long freed = 0;
  for (size_t i = 0; i < refs.size(); ++i) {
    const ArFrame& f = m->frames[refs[i].slot][refs[i].id];
    blocks[i] = lins_arena_block{f.off, (long long)f.n[0] + f.n[1] + f.n[2], drop[refs[i].slot] ? 0 : 1, 0};
    if (drop[refs[i].slot]) freed += blocks[i].n;
  }
  if (!lins_reclaim::blocks_ok((int)blocks.size(), blocks.data())) return LINS_E_STATE;  // (the records are the archive's own)
  std::vector<lins_arena_segment> plan;
  const int n_passes = lins_reclaim::plan((int)blocks.size(), blocks.data(), m->reclaim_chunk, plan);
  if (!plan.empty()) {
    // the table: segments | (segment, tile) entries, pass p's entries at [first[p], first[p + 1])
    std::vector<ArMove> segs(plan.size());
    std::vector<int2> tiles;
    std::vector<size_t> first((size_t)n_passes + 1, 0);
    std::vector<char> direct((size_t)n_passes, 0);
    long long stg = 0, need_stage = 0;
    uint64_t moved = 0;
    for (size_t i = 0; i < plan.size(); ++i) {
      const lins_arena_segment& g = plan[i];
      if (i == 0 || plan[i - 1].pass != g.pass) stg = 0, first[g.pass] = tiles.size(), direct[g.pass] = (char)g.direct;
      if (g.src < g.dst || g.dst < 0 || g.n < 1 || g.src + g.n > m->used || stg + g.n > m->reclaim_chunk) return LINS_E_STATE;
      segs[i] = ArMove{g.src, g.dst, g.n, stg};
      stg += g.n, moved += (uint64_t)g.n;
      if (!g.direct) need_stage = std::max(need_stage, stg);
      const long long nt = (g.n + kLmTile - 1) / kLmTile;
      if (i > (size_t)INT_MAX || nt > INT_MAX || tiles.size() + (size_t)nt > (size_t)INT_MAX) return LINS_E_CAPACITY;
      for (long long t = 0; t < nt; ++t) tiles.push_back(make_int2((int)i, (int)t));
    }
    first[n_passes] = tiles.size();
    const size_t o_tiles = align64(segs.size() * sizeof(ArMove)), tab_bytes = align64(o_tiles + tiles.size() * sizeof(int2));
    BUF_TRY(ctx, m->h_rc_tab.grow(tab_bytes));
    BUF_TRY(ctx, m->d_rc_tab.grow(tab_bytes));
    if (need_stage) BUF_TRY(ctx, m->d_reclaim.grow((size_t)std::min(m->reclaim_chunk, m->max_points)));
    std::memcpy(m->h_rc_tab, segs.data(), segs.size() * sizeof(ArMove));
    std::memcpy(m->h_rc_tab + o_tiles, tiles.data(), tiles.size() * sizeof(int2));
    hipStream_t st = ctx_stream(ctx);
    hipEvent_t e0, e1;
    ctx_events(ctx, &e0, &e1);
    HIP_TRY(ctx, hipMemcpyAsync(m->d_rc_tab, m->h_rc_tab, tab_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipEventRecord(e0, st));
    const ArMove* d_segs = (const ArMove*)m->d_rc_tab.get();
    const int2* d_tiles = (const int2*)(m->d_rc_tab + o_tiles);
    for (int p = 0; p < n_passes; ++p) {
      const int cnt = (int)(first[p + 1] - first[p]);
      if (direct[p]) {
        launch_ar_reclaim_move(st, cnt, d_segs, d_tiles + first[p], m->d_arena);
      } else {
        launch_ar_reclaim_gather(st, cnt, d_segs, d_tiles + first[p], m->d_arena, m->d_reclaim);
        launch_ar_reclaim_scatter(st, cnt, d_segs, d_tiles + first[p], m->d_reclaim, m->d_arena);
      }
      (direct[p] ? m->rc_direct : m->rc_staged) += 1;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(e1, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    HIP_TRY(ctx, hipEventElapsedTime(&m->rc_ms, e0, e1));
    m->rc_moved = moved;
  }
  const std::vector<long long> to = lins_reclaim::new_offsets((int)blocks.size(), blocks.data());
  for (size_t i = 0; i < refs.size(); ++i)
    if (blocks[i].keep) m->frames[refs[i].slot][refs[i].id].off = to[i];
  for (int k = 0; k < n; ++k) m->frames[slots[k]].clear(), mirrors_drop(m, slots[k]);
  m->used -= freed;
  if (released) *released = freed;
  return LINS_OK;
}

// ---- snapshot.h: every frame of the slot in id order.  A restore appends them at the arena's `used`, one after the
// other, so ids survive; the key-pose mirror is brought up by the next lins_keyposes_* call (stale_from = 0).
void archive_snapshot_context(lins_ctx* ctx, SnapContext& c) {
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return;
  c.modules |= LINS_SNAP_ARCHIVE;
  c.base[LINS_SNAP_BUF_ARENA] = m->d_arena.get(), c.units[LINS_SNAP_BUF_ARENA] = m->max_points;
}

int archive_snapshot_describe(lins_ctx* ctx, int slot, SnapStream& s) {
  Archive* m = archive_of(ctx);
  const std::vector<ArFrame>& fr = m->frames[slot];
  s.modules |= LINS_SNAP_ARCHIVE;
  s.counts.archive_frames = (int32_t)fr.size(), s.counts.archive_points = 0;
  lins_snapshot_frame* out = s.host_section<lins_snapshot_frame>(LINS_SNAP_SEC_AR_META, fr.size());
  s.ar_off.resize(fr.size()), s.ar_n.resize(fr.size());
  for (size_t i = 0; i < fr.size(); ++i) {
    const ArFrame& f = fr[i];
    std::memcpy(out[i].n, f.n, sizeof f.n);
    const float pose[6] = {f.pose.x, f.pose.y, f.pose.z, f.pose.roll, f.pose.pitch, f.pose.yaw};
    std::memcpy(out[i].pose, pose, sizeof pose);
    std::memcpy(out[i].t, f.t, sizeof f.t);
    out[i].time = f.time;
    s.ar_off[i] = f.off, s.ar_n[i] = f.n[0] + f.n[1] + f.n[2];
    s.counts.archive_points += s.ar_n[i];
  }
  return LINS_OK;
}

int archive_restore_check(lins_ctx* ctx, int slot, lins_snapshot_limits& lim) {
  Archive* m = archive_of(ctx);
  if (!m->frames[slot].empty()) return LINS_E_STATE;
  lim.archive_frames = m->max_frames, lim.archive_points = m->max_points - m->used;
  return LINS_OK;
}

void archive_restore_place(lins_ctx* ctx, int slot, const SnapView& v, SnapStream& s, long long* arena_at) {
  const int cnt = v.info.counts.archive_frames;
  s.ar_off.resize(cnt), s.ar_n.resize(cnt);
  for (int i = 0; i < cnt; ++i) {
    lins_snapshot_frame f;
    std::memcpy(&f, v.sec(LINS_SNAP_SEC_AR_META) + (size_t)i * sizeof f, sizeof f);
    s.ar_off[i] = *arena_at, s.ar_n[i] = f.n[0] + f.n[1] + f.n[2];
    *arena_at += s.ar_n[i];
  }
}

void archive_restore_apply(lins_ctx* ctx, int slot, const SnapView& v, const SnapStream& s) {
  Archive* m = archive_of(ctx);
  const int cnt = v.info.counts.archive_frames;
  std::vector<ArFrame>& fr = m->frames[slot];
  fr.assign((size_t)cnt, ArFrame{});
  for (int i = 0; i < cnt; ++i) {
    lins_snapshot_frame f;
    std::memcpy(&f, v.sec(LINS_SNAP_SEC_AR_META) + (size_t)i * sizeof f, sizeof f);
    fr[i].off = s.ar_off[i], fr[i].time = f.time;
    std::memcpy(fr[i].n, f.n, sizeof f.n);
    fr[i].pose = lins_key_pose{f.pose[0], f.pose[1], f.pose[2], f.pose[3], f.pose[4], f.pose[5]};
    std::memcpy(fr[i].t, f.t, sizeof f.t);
  }
  m->used += v.info.counts.archive_points;
  mirrors_drop(m, slot);
}
}  // namespace lins

extern "C" {

int lins_archive_init(lins_ctx* ctx, int n_slots, int max_frames_per_slot, long long max_points_total) {
  if (!ctx || n_slots < 1 || max_frames_per_slot < 1 || max_points_total < 1 || max_points_total > (1ll << 40)) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  Archive* m = archive_of(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));  // (a push_scans copy may still write the old arena)
  m->d_arena.reset(), m->d_kp_pose.reset(), m->d_kp_time.reset();
  m->n_slots = 0, m->built = false, m->used = 0;
  m->frames.clear();
  m->place.on = false, m->place.described.clear(), m->place.d_D.reset(), m->place.d_rec.reset();  // (sized by lins_place_init)
  m->place.team.drop();
  BUF_TRY(ctx, m->d_arena.grow((size_t)max_points_total));
  BUF_TRY(ctx, m->d_kp_pose.grow((size_t)n_slots * max_frames_per_slot));
  BUF_TRY(ctx, m->d_kp_time.grow((size_t)n_slots * max_frames_per_slot));
  m->n_slots = n_slots, m->max_frames = max_frames_per_slot, m->max_points = max_points_total;
  m->frames.assign(n_slots, {});
  m->stale_from.assign(n_slots, 0);
  return LINS_OK;
}

int lins_archive_push(lins_ctx* ctx, int slot, const lins_keyframe* f, double time) {
  if (!ctx || !f) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots) return LINS_E_ARG;
  const lins_point* c[3] = {f->corner, f->surf, f->outlier};
  const int n[3] = {f->n_corner, f->n_surf, f->n_outlier};
  for (int k = 0; k < 3; ++k) {
    if (n[k] < 0 || (n[k] && !c[k])) return LINS_E_ARG;
    if (!cloud_ok(c[k], n[k])) return LINS_E_INPUT;
  }
  if (!pose_ok(f->pose) || !std::isfinite(time)) return LINS_E_INPUT;
  const long long total = (long long)n[0] + n[1] + n[2];
  if (m->used + total > m->max_points || (int)m->frames[slot].size() >= m->max_frames) return LINS_E_CAPACITY;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  ArFrame fr{};
  fr.off = m->used, fr.time = time;
  float4* dst = m->d_arena + fr.off;
  for (int k = 0; k < 3; ++k) {
    fr.n[k] = n[k];
    if (n[k]) HIP_TRY(ctx, hipMemcpyAsync(dst, c[k], (size_t)n[k] * sizeof(float4), hipMemcpyHostToDevice, st));
    dst += n[k];
  }
  set_pose(fr, f->pose);
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (the caller's clouds may go once this returns)
  m->used += total;
  m->frames[slot].push_back(fr);
  stale_at(m, slot, (int)m->frames[slot].size() - 1);
  return (int)m->frames[slot].size() - 1;
}

int lins_archive_push_scans(lins_ctx* ctx, int n, const int32_t* entries, const lins_key_pose* poses, const double* times, int32_t* ids_out) {
  if (!ctx || n < 0 || (n && (!entries || !poses || !times))) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  LocalMapView v;
  if (int rc = local_map_view(ctx, &v)) return rc;
  long long total = 0;
  std::vector<int> added(m->n_slots, 0);
  for (int i = 0; i < n; ++i) {
    const int e = entries[i];
    if (e < 0 || e >= v.n || v.slots[e] >= m->n_slots) return LINS_E_ARG;
    const lins_local_map_sizes& z = v.sizes[e];
    if (z.status) return LINS_E_STATE;
    if (!pose_ok(poses[i]) || !std::isfinite(times[i])) return LINS_E_INPUT;
    total += (long long)z.n[LINS_LOCAL_SCAN_CORNER] + z.n[LINS_LOCAL_SCAN_SURF] + z.n[LINS_LOCAL_SCAN_OUTLIER];
    if ((int)m->frames[v.slots[e]].size() + ++added[v.slots[e]] > m->max_frames) return LINS_E_CAPACITY;
  }
  if (m->used + total > m->max_points) return LINS_E_CAPACITY;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  for (int i = 0; i < n; ++i) {  // saveKeyFramesAndFactor (LM:1758-1763): cornerDS, surfDS, outlierDS
    const int e = entries[i], s = v.slots[e];
    ArFrame fr{};
    fr.off = m->used, fr.time = times[i];
    float4* dst = m->d_arena + fr.off;
    for (int q = 0; q < 3; ++q) {
      const int c = LINS_LOCAL_SCAN_CORNER + q, cnt = v.sizes[e].n[c];
      fr.n[q] = cnt;
      if (cnt) HIP_TRY(ctx, hipMemcpyAsync(dst, v.d_out + v.off[6 * e + c], (size_t)cnt * sizeof(float4), hipMemcpyDeviceToDevice, st));
      dst += cnt;
    }
    set_pose(fr, poses[i]);
    m->used += (long long)fr.n[0] + fr.n[1] + fr.n[2];
    m->frames[s].push_back(fr);
    stale_at(m, s, (int)m->frames[s].size() - 1);
    if (ids_out) ids_out[i] = (int32_t)m->frames[s].size() - 1;
  }
  return LINS_OK;
}

int lins_archive_set_poses(lins_ctx* ctx, int slot, int first_id, int n, const lins_key_pose* poses) {
  if (!ctx || n < 0 || (n && !poses)) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots || first_id < 0 || (long long)first_id + n > (long long)m->frames[slot].size()) return LINS_E_ARG;
  for (int i = 0; i < n; ++i)
    if (!pose_ok(poses[i])) return LINS_E_INPUT;
  for (int i = 0; i < n; ++i) set_pose(m->frames[slot][first_id + i], poses[i]);
  if (n) stale_at(m, slot, first_id);
  return LINS_OK;
}

int lins_archive_count(lins_ctx* ctx, int slot) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots) return LINS_E_ARG;
  return (int)m->frames[slot].size();
}

int lins_archive_select_radius(lins_ctx* ctx, int slot, const float centre[3], float radius, float pose_leaf, int32_t* ids, int cap) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots || cap < 0 || !lins_select::query_ok(centre, radius) || !(pose_leaf > 0.f)) return LINS_E_ARG;
  const std::vector<lins_key_pose> poses = poses_of(m->frames[slot]);
  std::vector<int> sel;
  if (!lins_select::select_radius(poses.data(), (int)poses.size(), centre, radius, pose_leaf, sel)) return LINS_E_CAPACITY;
  if ((int)sel.size() > cap) return LINS_E_CAPACITY;
  if (!sel.empty() && !ids) return LINS_E_ARG;
  for (size_t i = 0; i < sel.size(); ++i) ids[i] = sel[i];
  return (int)sel.size();
}

int lins_archive_find_loop(lins_ctx* ctx, int slot, const float centre[3], float radius, double now, double min_gap_s, int32_t* closest) {
  if (!ctx || !closest) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots || !lins_select::query_ok(centre, radius)) return LINS_E_ARG;
  const std::vector<lins_key_pose> poses = poses_of(m->frames[slot]);
  std::vector<double> times(poses.size());
  for (size_t i = 0; i < times.size(); ++i) times[i] = m->frames[slot][i].time;
  *closest = lins_select::find_loop(poses.data(), times.data(), (int)poses.size(), centre, radius, now, min_gap_s);
  return LINS_OK;
}

int lins_archive_set_scan_chunk(lins_ctx* ctx, int chunk_tiles) {
  if (!ctx || chunk_tiles < 0) return LINS_E_ARG;
  archive_of(ctx)->chunk = chunk_tiles ? chunk_tiles : kArScanChunk;
  return LINS_OK;
}

int lins_archive_assemble(lins_ctx* ctx, int n, const lins_submap_spec* specs, lins_submap_info* out) {
  if (!ctx || n < 0 || (n && !specs)) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  const int all = LINS_SUBMAP_CORNER | LINS_SUBMAP_SURF | LINS_SUBMAP_OUTLIER;
  std::vector<long long> cap(n, 0);
  for (int k = 0; k < n; ++k) {
    const lins_submap_spec& sp = specs[k];
    if (sp.slot < 0 || sp.slot >= m->n_slots || sp.n_ids < 0 || (sp.n_ids && !sp.ids) || sp.clouds <= 0 || (sp.clouds & ~all) ||
        (sp.flags & ~LINS_SUBMAP_DROP_NEGATIVE) || !(sp.leaf >= 0.f) || !std::isfinite(sp.leaf) ||
        ((sp.flags & LINS_SUBMAP_DROP_NEGATIVE) && sp.leaf != 0.f))
      return LINS_E_ARG;
    const std::vector<ArFrame>& fr = m->frames[sp.slot];
    for (int i = 0; i < sp.n_ids; ++i) {
      if (sp.ids[i] < 0 || sp.ids[i] >= (int)fr.size()) return LINS_E_ARG;
      for (int q = 0; q < 3; ++q)
        if (sp.clouds & (1 << q)) cap[k] += fr[sp.ids[i]].n[q];
    }
  }
  for (int k = 0; k < n; ++k)
    if (cap[k] > INT_MAX / 2) return LINS_E_CAPACITY;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  m->built = false, m->serial += 1;
  // jobs: VoxelGrid jobs first — those whose scans are split, then the others — then the leaf == 0 jobs, the split ones last
  const int chunk = m->chunk;
  auto tiles_of = [&](int k) { return (cap[k] + kLmTile - 1) / kLmTile; };
  auto cls = [&](int k) {
    const bool vg = specs[k].leaf > 0.f, split = tiles_of(k) > chunk;
    return vg ? (split ? 0 : 1) : (split ? 3 : 2);
  };
  std::vector<int> spec_of, job_of(n);
  int bound[5] = {0, 0, 0, 0, 0};  // jobs of class c: [bound[c], bound[c + 1])
  for (int c = 0; c < 4; ++c) {
    for (int k = 0; k < n; ++k)
      if (cls(k) == c) job_of[k] = (int)spec_of.size(), spec_of.push_back(k);
    bound[c + 1] = (int)spec_of.size();
  }
  const int nv = bound[2];
  std::vector<LmJob> jobs(n);
  std::vector<LmState> states(n);
  std::vector<int> jflags(n, 0);
  std::vector<int2> tiles;
  std::vector<ArChunk> chunks;
  std::vector<ArSplit> splits;
  size_t stage_total = 0, sort_total = 0, tiles_total = 0, vg_tiles = 0, out_total = 0;
  int n_hist_chunks = 0;
  for (int j = 0; j < n; ++j) {
    const int k = spec_of[j];
    LmJob& jb = jobs[j];
    jb.off_in = (long long)stage_total, stage_total += (size_t)cap[k];
    jb.off_out = (long long)out_total, out_total += (size_t)cap[k];
    jb.cap = (int)cap[k];
    jb.ntiles = (int)tiles_of(k);
    jb.tile0 = (int)tiles_total, tiles_total += (size_t)jb.ntiles;
    jb.inv = specs[k].leaf > 0.f ? 1.0f / specs[k].leaf : 0.f;
    jb.out_after = jb.src_a = jb.src_b = jb.feed = jb.feed_after = -1, jb.map = j < nv ? 1 : 0, jb.pad = 0;
    jflags[j] = specs[k].flags;
    if (j < nv) sort_total = stage_total, vg_tiles = tiles_total;
    for (int t = 0; t < jb.ntiles; ++t) tiles.push_back(make_int2(j, t));
    LmState& st = states[j];
    std::memset(&st, 0, sizeof st);
    for (int a = 0; a < 3; ++a)
      st.mn[a] = lm_enc(INFINITY), st.mx[a] = lm_enc(-INFINITY), st.bmin[a] = INT_MAX, st.bmax[a] = INT_MIN;
    st.n = jb.cap;
  }
  if (tiles_total > (size_t)INT_MAX / 256) return LINS_E_CAPACITY;
  for (int pass = 0; pass < 2; ++pass) {  // the split jobs' chunks: the VoxelGrid jobs' first (the histogram scans use those alone)
    for (int j = pass ? bound[3] : 0; j < (pass ? bound[4] : bound[1]); ++j) {
      ArSplit s{j, (int)chunks.size(), (jobs[j].ntiles + chunk - 1) / chunk, 0};
      for (int c = 0; c < s.nc; ++c) chunks.push_back(ArChunk{j, c, s.c0, 0});
      splits.push_back(s);
    }
    if (!pass) n_hist_chunks = (int)chunks.size();
  }
  // the chosen clouds: one segment per run of chosen clouds of a frame (they lie one after the other in the arena and
  // share the frame's pose), blocks of kLmTile points
  std::vector<LmSeg> segs;
  std::vector<int2> blocks;
  uint64_t pts_in = 0;
  for (int j = 0; j < n; ++j) {
    const lins_submap_spec& sp = specs[spec_of[j]];
    long long at = jobs[j].off_in;
    for (int i = 0; i < sp.n_ids; ++i) {
      const ArFrame& f = m->frames[sp.slot][sp.ids[i]];
      long long src = f.off;
      for (int q = 0; q < 3;) {
        if (!(sp.clouds & (1 << q))) {
          src += f.n[q++];
          continue;
        }
        LmSeg g{};
        g.src = src, g.dst = at, g.job = j;
        for (; q < 3 && (sp.clouds & (1 << q)); ++q) g.n += f.n[q];
        std::memcpy(g.t, f.t, sizeof g.t);
        if (g.n) {
          for (int b = 0; b < (g.n + kLmTile - 1) / kLmTile; ++b) blocks.push_back(make_int2((int)segs.size(), b));
          segs.push_back(g);
        }
        src += g.n, at += g.n, pts_in += (uint64_t)g.n;
      }
    }
  }
  // one table upload: jobs | states | segments | blocks | tiles | job flags | chunks | splits
  const size_t o_jobs = 0, o_states = align64(o_jobs + n * sizeof(LmJob)), o_segs = align64(o_states + n * sizeof(LmState)),
               o_blocks = align64(o_segs + segs.size() * sizeof(LmSeg)), o_tiles = align64(o_blocks + blocks.size() * sizeof(int2)),
               o_flags = align64(o_tiles + tiles.size() * sizeof(int2)), o_chunks = align64(o_flags + n * sizeof(int)),
               o_splits = align64(o_chunks + chunks.size() * sizeof(ArChunk)), tab_bytes = align64(o_splits + splits.size() * sizeof(ArSplit));
  BUF_TRY(ctx, m->h_tab.grow(tab_bytes));
  BUF_TRY(ctx, m->h_states.grow(n * sizeof(LmState)));
  auto put = [&](size_t o, const void* p, size_t bytes) {
    if (bytes) std::memcpy(m->h_tab + o, p, bytes);
  };
  put(o_jobs, jobs.data(), n * sizeof(LmJob)), put(o_states, states.data(), n * sizeof(LmState));
  put(o_segs, segs.data(), segs.size() * sizeof(LmSeg)), put(o_blocks, blocks.data(), blocks.size() * sizeof(int2));
  put(o_tiles, tiles.data(), tiles.size() * sizeof(int2)), put(o_flags, jflags.data(), n * sizeof(int));
  put(o_chunks, chunks.data(), chunks.size() * sizeof(ArChunk)), put(o_splits, splits.data(), splits.size() * sizeof(ArSplit));
  BUF_TRY(ctx, m->d_tab.grow(tab_bytes));
  BUF_TRY(ctx, m->d_stage.grow(stage_total));
  BUF_TRY(ctx, m->d_out.grow(out_total));
  BUF_TRY(ctx, m->d_hist.grow(vg_tiles * 256));
  BUF_TRY(ctx, m->d_tilecnt.grow(tiles_total));
  BUF_TRY(ctx, m->d_csum.grow(chunks.size()));
  // the sort's scratch: the extent of the VoxelGrid jobs' staging
  BUF_TRY(ctx, grow_all(m->d_ka, sort_total, m->d_kb, sort_total, m->d_va, sort_total, m->d_vb, sort_total, m->d_starts, sort_total));
  hipStream_t st = ctx_stream(ctx);
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  if (tab_bytes) HIP_TRY(ctx, hipMemcpyAsync(m->d_tab, m->h_tab, tab_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(e0, st));
  const LmJob* d_jobs = (const LmJob*)(m->d_tab + o_jobs);
  LmState* d_states = (LmState*)(m->d_tab + o_states);
  const int2* d_tiles = (const int2*)(m->d_tab + o_tiles);
  const int* d_flags = (const int*)(m->d_tab + o_flags);
  const ArChunk* d_chunks = (const ArChunk*)(m->d_tab + o_chunks);
  const ArSplit* d_splits = (const ArSplit*)(m->d_tab + o_splits);
  const int vt = (int)vg_tiles, ct = (int)(tiles_total - vg_tiles);
  launch_ar_gather(st, (int)blocks.size(), (const LmSeg*)(m->d_tab + o_segs), (const int2*)(m->d_tab + o_blocks), m->d_arena, m->d_stage, d_states);
  // the VoxelGrid jobs: the local-map build's kernels; the scans of the jobs [0, bound[1]) over many workgroups
  launch_lm_setup(st, 0, nv, d_jobs, d_states);
  launch_lm_keys(st, vt, d_tiles, d_jobs, d_states, m->d_stage, m->d_ka, m->d_va);
  for (int p = 0; p < kLmPasses && vt; ++p) {
    unsigned *kin = (p & 1) ? m->d_kb : m->d_ka, *kout = (p & 1) ? m->d_ka : m->d_kb;
    int *vin = (p & 1) ? m->d_vb : m->d_va, *vout = (p & 1) ? m->d_va : m->d_vb;
    launch_lm_hist(st, p, vt, d_tiles, d_jobs, d_states, kin, m->d_hist);
    launch_lm_scan(st, p, bound[1], nv - bound[1], d_jobs, d_states, m->d_hist);
    launch_ar_scan(st, 256, p, chunk, n_hist_chunks, d_chunks, bound[1], d_splits, d_jobs, d_states, m->d_hist, m->d_csum);
    launch_lm_scatter(st, p, vt, d_tiles, d_jobs, d_states, m->d_hist, kin, vin, kout, vout);
  }
  launch_lm_heads(st, vt, d_tiles, d_jobs, d_states, m->d_ka, m->d_kb, m->d_tilecnt);
  // the leaf == 0 jobs: keep counts per tile; then one scan of the per-tile counts for both kinds
  launch_ar_keep(st, nv, n - nv, ct, d_tiles + vt, d_jobs, d_states, d_flags, m->d_stage, m->d_tilecnt);
  launch_lm_heads_scan(st, bound[1], bound[3] - bound[1], d_jobs, d_states, m->d_tilecnt);
  launch_ar_scan(st, 1, -1, chunk, (int)chunks.size(), d_chunks, (int)splits.size(), d_splits, d_jobs, d_states, m->d_tilecnt, m->d_csum);
  launch_lm_starts(st, vt, d_tiles, d_jobs, d_states, m->d_ka, m->d_kb, m->d_tilecnt, m->d_starts);
  launch_lm_sum(st, vt, d_tiles, d_jobs, d_states, m->d_va, m->d_vb, m->d_starts, m->d_stage, m->d_out);
  launch_ar_compact(st, ct, d_tiles + vt, d_jobs, d_states, d_flags, m->d_stage, m->d_tilecnt, m->d_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(e1, st));
  if (n) HIP_TRY(ctx, hipMemcpyAsync(m->h_states, d_states, n * sizeof(LmState), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&m->ms, e0, e1));
  m->points_in = pts_in;
  const LmState* S = (const LmState*)m->h_states.get();
  m->off.assign(n, 0);
  m->info.assign(n, lins_submap_info{});
  m->filtered.assign(n, 0);
  for (int k = 0; k < n; ++k) {
    const int j = job_of[k];
    lins_submap_info& z = m->info[k];
    z.status = S[j].status, z.frames = specs[k].n_ids, z.points_in = (uint64_t)cap[k];
    z.n = z.status ? 0 : S[j].nvox;
    m->off[k] = jobs[j].off_out;
    m->filtered[k] = j < nv;
    const bool box = j < nv && z.n > 0;
    for (int a = 0; a < 3; ++a) z.box_min[a] = box ? S[j].bmin[a] : 0, z.box_dim[a] = box ? S[j].bmax[a] - S[j].bmin[a] + 1 : 1;
    if (out) out[k] = z;
  }
  m->built = true;
  return LINS_OK;
}

int lins_archive_download(lins_ctx* ctx, int entry, lins_point* out, int cap) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->built) return LINS_E_STATE;
  if (entry < 0 || entry >= (int)m->info.size()) return LINS_E_ARG;
  const int cnt = m->info[entry].n;
  if (cnt > cap) return LINS_E_CAPACITY;
  if (cnt && !out) return LINS_E_ARG;
  if (!cnt) return 0;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(out, m->d_out + m->off[entry], (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return cnt;
}

// ---- include/lins_lifecycle.h: the archive's part
int lins_archive_usage(lins_ctx* ctx, long long* used, long long* capacity) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (used) *used = m->used;
  if (capacity) *capacity = m->max_points;
  return LINS_OK;
}

int lins_archive_release_slots(lins_ctx* ctx, int n, const int32_t* slots, long long* released) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (int rc = release_list_check(n, slots, m->n_slots)) return rc;
  if (int rc = ctx_quiesce(ctx)) return rc;
  return archive_release_apply(ctx, n, slots, released);
}

int lins_archive_set_reclaim_chunk(lins_ctx* ctx, long long chunk_points) {
  if (!ctx || chunk_points < 0) return LINS_E_ARG;
  archive_of(ctx)->reclaim_chunk = chunk_points ? chunk_points : kArReclaimChunk;
  return LINS_OK;
}

int lins_last_reclaim_stats(lins_ctx* ctx, float* ms, uint64_t* points_moved, int32_t* staged_passes, int32_t* direct_passes) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (ms) *ms = m->rc_ms;
  if (points_moved) *points_moved = m->rc_moved;
  if (staged_passes) *staged_passes = m->rc_staged;
  if (direct_passes) *direct_passes = m->rc_direct;
  return LINS_OK;
}

int lins_last_archive_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* points_in) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (kernel_ms) *kernel_ms = m->ms;
  if (points_in) *points_in = m->points_in;
  return LINS_OK;
}

}  // extern "C"

// ---- key-pose selection on the device (include/lins_map.h lins_keyposes_*) ------------------------------------------------
namespace {

enum KpKind { kKpSelect, kKpLoop, kKpSurround };

// One batched selection: the whole call's refusals, then one upload (entries | stale mirror records | lists), one chain
// of launches, one download (results | ids or lists or candidates) and one synchronisation; the entries the kernel hands
// back (KpOut::host) are served by host/keyframe_select.h here.  q(k): entry k's query; lq: the loop queries or null.
int kp_batch(lins_ctx* ctx, KpKind kind, int n, const lins_keyposes_query* qs, const lins_keyposes_loop_query* lq, int32_t* ids, int stride,
             int32_t* n_list, int32_t* closest, lins_keyposes_result* results) {
  if (!ctx || n < 0 || (n && !qs && !lq)) return LINS_E_ARG;
  if (kind != kKpLoop && (stride < 0 || (n && (!results || (stride && !ids))))) return LINS_E_ARG;
  if (kind == kKpLoop && n && !closest) return LINS_E_ARG;
  if (kind == kKpSurround && n && !n_list) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  auto q = [&](int k) -> const lins_keyposes_query& { return lq ? lq[k].q : qs[k]; };
  for (int k = 0; k < n; ++k) {
    const lins_keyposes_query& a = q(k);
    if (a.slot < 0 || a.slot >= m->n_slots || !lins_select::query_ok(a.centre, a.radius)) return LINS_E_ARG;
    if (kind != kKpLoop && (!(a.pose_leaf > 0.f) || !std::isfinite(1.0f / a.pose_leaf))) return LINS_E_ARG;
    if (kind == kKpLoop && (!std::isfinite(lq[k].now) || std::isnan(lq[k].min_gap_s))) return LINS_E_INPUT;
    if (kind == kKpSurround) {
      const int nf = (int)m->frames[a.slot].size();
      if (n_list[k] < 0 || n_list[k] > stride) return LINS_E_ARG;
      for (int i = 0; i < n_list[k]; ++i)
        if (ids[(size_t)k * stride + i] < 0 || ids[(size_t)k * stride + i] >= nf) return LINS_E_ARG;
    }
  }
  m->kp_ms = 0.f, m->kp_host = 0, m->kp_hits = 0;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  // the table: entries | stale records of the slots named | (surround) the lists
  std::vector<KpEntry> entries((size_t)n);
  std::vector<KpStale> stale;
  long long scratch_total = 0;
  for (int k = 0; k < n; ++k) {
    const lins_keyposes_query& a = q(k);
    const std::vector<ArFrame>& fr = m->frames[a.slot];
    KpEntry& e = entries[k];
    std::memset(&e, 0, sizeof e);
    e.base = (long long)a.slot * m->max_frames, e.nf = (int)fr.size();
    std::memcpy(e.c, a.centre, sizeof e.c);
    e.r2 = a.radius * a.radius;
    e.inv = kind == kKpLoop ? 0.f : 1.0f / a.pose_leaf;
    e.stride = stride;
    if (kind == kKpLoop) e.now = lq[k].now, e.gap = lq[k].min_gap_s;
    if (kind == kKpSurround) e.n_list = n_list[k], e.mark_off = scratch_total, scratch_total += 2ll * e.nf;
    for (int i = m->stale_from[a.slot]; i < e.nf; ++i)
      stale.push_back(KpStale{fr[i].time, fr[i].pose.x, fr[i].pose.y, fr[i].pose.z, 0, e.base + i});
    m->stale_from[a.slot] = e.nf;  // (a slot named again in this call adds nothing)
  }
  const size_t out_ints = kind == kKpLoop ? (size_t)n : (size_t)n * stride;
  const size_t o_stale = align64(n * sizeof(KpEntry)), o_lists = align64(o_stale + stale.size() * sizeof(KpStale)),
               up_bytes = align64(o_lists + (kind == kKpSurround ? out_ints * sizeof(int) : 0));
  const size_t o_ints = align64(n * sizeof(KpOut)), down_bytes = align64(o_ints + out_ints * sizeof(int));
  auto grow_staging = [&]() -> int {
    BUF_TRY(ctx, m->h_kp_up.grow(up_bytes));
    BUF_TRY(ctx, m->d_kp_up.grow(up_bytes));
    BUF_TRY(ctx, m->h_kp_down.grow(down_bytes));
    BUF_TRY(ctx, m->d_kp_down.grow(down_bytes));
    BUF_TRY(ctx, m->d_kp_scratch.grow((size_t)scratch_total));
    return LINS_OK;
  };
  if (const int rc = grow_staging()) {
    std::fill(m->stale_from.begin(), m->stale_from.end(), 0);  // (the records packed above did not go up)
    return rc;
  }
  std::memcpy(m->h_kp_up, entries.data(), n * sizeof(KpEntry));
  if (!stale.empty()) std::memcpy(m->h_kp_up + o_stale, stale.data(), stale.size() * sizeof(KpStale));
  if (kind == kKpSurround && out_ints) std::memcpy(m->h_kp_up + o_lists, ids, out_ints * sizeof(int));
  hipStream_t st = ctx_stream(ctx);
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  const KpEntry* d_entries = (const KpEntry*)m->d_kp_up.get();
  KpOut* d_out = (KpOut*)m->d_kp_down.get();
  int* d_ints = (int*)(m->d_kp_down + o_ints);
  hipError_t err = hipMemcpyAsync(m->d_kp_up, m->h_kp_up, up_bytes, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipEventRecord(e0, st);
  if (err == hipSuccess) {
    launch_kp_refresh(st, (int)stale.size(), (const KpStale*)(m->d_kp_up + o_stale), m->d_kp_pose, m->d_kp_time);
    if (kind == kKpSelect) launch_kp_select(st, n, d_entries, m->d_kp_pose, d_ints, d_out);
    if (kind == kKpSurround) launch_kp_surround(st, n, d_entries, m->d_kp_pose, (const int*)(m->d_kp_up + o_lists), d_ints, m->d_kp_scratch, d_out);
    if (kind == kKpLoop) launch_kp_find_loop(st, n, d_entries, m->d_kp_pose, m->d_kp_time, d_ints);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipEventRecord(e1, st);
  if (err == hipSuccess) err = hipMemcpyAsync(m->h_kp_down, m->d_kp_down, down_bytes, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) {
    std::fill(m->stale_from.begin(), m->stale_from.end(), 0);  // (what of the mirror was written is not known)
    return ctx_fail_hip(ctx, err, "lins_keyposes batch");
  }
  HIP_TRY(ctx, hipEventElapsedTime(&m->kp_ms, e0, e1));
  const KpOut* O = (const KpOut*)m->h_kp_down.get();
  const int* I = (const int*)(m->h_kp_down + o_ints);
  if (kind == kKpLoop) {
    for (int k = 0; k < n; ++k) closest[k] = I[k];
    return LINS_OK;
  }
  for (int k = 0; k < n; ++k) {
    const lins_keyposes_query& a = q(k);
    lins_keyposes_result& r = results[k];
    r = lins_keyposes_result{O[k].n, O[k].hits, O[k].status, O[k].host};
    m->kp_hits += (uint64_t)O[k].hits;
    int32_t* mine = ids + (size_t)k * stride;
    if (!O[k].host) {
      if (r.status) continue;
      const int cnt = kind == kKpSelect ? O[k].n : O[k].n_list;
      if (cnt) std::memcpy(mine, I + (size_t)k * stride, (size_t)cnt * sizeof(int));
      if (kind == kKpSurround) n_list[k] = cnt;
      continue;
    }
    m->kp_host += 1;  // the host text, with the same bits
    const std::vector<lins_key_pose> poses = poses_of(m->frames[a.slot]);
    std::vector<int> sel;
    r.n = 0;
    if (!lins_select::select_radius(poses.data(), (int)poses.size(), a.centre, a.radius, a.pose_leaf, sel)) {
      r.status = LINS_E_CAPACITY;
      continue;
    }
    if (kind == kKpSelect) {
      if ((int)sel.size() > stride) {
        r.status = LINS_E_CAPACITY;
        continue;
      }
      std::copy(sel.begin(), sel.end(), mine);
    } else {
      std::vector<int> list(mine, mine + n_list[k]);
      lins_select::surround_update(list, sel);
      if ((int)list.size() > stride) {
        r.status = LINS_E_CAPACITY;
        continue;
      }
      std::copy(list.begin(), list.end(), mine);
      n_list[k] = (int32_t)list.size();
    }
    r.n = (int32_t)sel.size();
  }
  return LINS_OK;
}

// The team selection, batched: the conventions of kp_batch (the whole call's refusals, one upload: entries | targets |
// stale mirror records of every slot named, the refresh and one workgroup per entry, one download, one synchronisation);
// the entries the kernel hands back are served by host/team_select.h here, with the same bits.
int ts_batch(lins_ctx* ctx, int n, const lins_keyposes_team_query* qs, const int32_t* table, int n_table, int32_t* pairs, int stride,
             lins_keyposes_result* results) {
  if (!ctx || n < 0 || n_table < 0 || stride < 0 || (n_table && !table) || (n && (!qs || !results || (stride && !pairs)))) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  for (int t = 0; t < n_table; ++t)
    if (table[t] < 0 || table[t] >= m->n_slots) return LINS_E_ARG;
  std::vector<std::vector<int>> order((size_t)n);  // entry k's targets in ascending slot order (positions in its range)
  size_t n_rec = 0;
  for (int k = 0; k < n; ++k) {
    const lins_keyposes_team_query& a = qs[k];
    if (!lins_select::query_ok(a.centre, a.radius) || !lins_team_select::leaf_ok(a.pose_leaf)) return LINS_E_ARG;
    if (a.n_targets < 0 || a.first_target < 0 || (long long)a.first_target + a.n_targets > n_table) return LINS_E_ARG;
    if (!lins_team_select::order_targets(a.n_targets, table + a.first_target, order[k])) return LINS_E_ARG;
    n_rec += (size_t)a.n_targets;
  }
  if (n_rec > (size_t)INT_MAX || (stride && (size_t)n > (size_t)INT_MAX / 2 / (size_t)stride)) return LINS_E_CAPACITY;
  m->ts_ms = 0.f, m->ts_host = 0, m->ts_hits = 0;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  std::vector<TsEntry> entries((size_t)n);
  std::vector<TsTarget> recs;
  std::vector<KpStale> stale;
  recs.reserve(n_rec);
  for (int k = 0; k < n; ++k) {
    const lins_keyposes_team_query& a = qs[k];
    TsEntry& e = entries[k];
    std::memset(&e, 0, sizeof e);
    std::memcpy(e.c, a.centre, sizeof e.c);
    e.r2 = a.radius * a.radius, e.inv = 1.0f / a.pose_leaf;
    e.n_targets = a.n_targets, e.t0 = (int)recs.size(), e.stride = stride;
    long long total = 0;
    for (int t : order[k]) {
      const int slot = table[a.first_target + t];
      const std::vector<ArFrame>& fr = m->frames[slot];
      const long long base = (long long)slot * m->max_frames;
      recs.push_back(TsTarget{base, (int)std::min<long long>(total, INT_MAX), slot});
      total += (long long)fr.size();
      for (int i = m->stale_from[slot]; i < (int)fr.size(); ++i)
        stale.push_back(KpStale{fr[i].time, fr[i].pose.x, fr[i].pose.y, fr[i].pose.z, 0, base + i});
      m->stale_from[slot] = (int)fr.size();  // (a slot named again in this call adds nothing)
    }
    e.host = total > INT_MAX;  // (a place is an int; the records of such an entry are not read)
    e.total = e.host ? 0 : (int)total;
  }
  const size_t out_ints = (size_t)n * stride * 2;
  const size_t o_recs = align64(n * sizeof(TsEntry)), o_stale = align64(o_recs + recs.size() * sizeof(TsTarget)),
               up_bytes = align64(o_stale + stale.size() * sizeof(KpStale));
  const size_t o_ints = align64(n * sizeof(KpOut)), down_bytes = align64(o_ints + out_ints * sizeof(int));
  auto grow_staging = [&]() -> int {
    BUF_TRY(ctx, m->h_kp_up.grow(up_bytes));
    BUF_TRY(ctx, m->d_kp_up.grow(up_bytes));
    BUF_TRY(ctx, m->h_kp_down.grow(down_bytes));
    BUF_TRY(ctx, m->d_kp_down.grow(down_bytes));
    return LINS_OK;
  };
  if (const int rc = grow_staging()) {
    std::fill(m->stale_from.begin(), m->stale_from.end(), 0);  // (the records packed above did not go up)
    return rc;
  }
  std::memcpy(m->h_kp_up, entries.data(), n * sizeof(TsEntry));
  if (!recs.empty()) std::memcpy(m->h_kp_up + o_recs, recs.data(), recs.size() * sizeof(TsTarget));
  if (!stale.empty()) std::memcpy(m->h_kp_up + o_stale, stale.data(), stale.size() * sizeof(KpStale));
  hipStream_t st = ctx_stream(ctx);
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  KpOut* d_out = (KpOut*)m->d_kp_down.get();
  hipError_t err = hipMemcpyAsync(m->d_kp_up, m->h_kp_up, up_bytes, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipEventRecord(e0, st);
  if (err == hipSuccess) {
    launch_kp_refresh(st, (int)stale.size(), (const KpStale*)(m->d_kp_up + o_stale), m->d_kp_pose, m->d_kp_time);
    launch_team_select(st, n, (const TsEntry*)m->d_kp_up.get(), (const TsTarget*)(m->d_kp_up + o_recs), m->d_kp_pose,
                       (int2*)(m->d_kp_down + o_ints), d_out);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipEventRecord(e1, st);
  if (err == hipSuccess) err = hipMemcpyAsync(m->h_kp_down, m->d_kp_down, down_bytes, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) {
    std::fill(m->stale_from.begin(), m->stale_from.end(), 0);  // (what of the mirror was written is not known)
    return ctx_fail_hip(ctx, err, "lins_keyposes_team_select_batch");
  }
  HIP_TRY(ctx, hipEventElapsedTime(&m->ts_ms, e0, e1));
  const KpOut* O = (const KpOut*)m->h_kp_down.get();
  const int* I = (const int*)(m->h_kp_down + o_ints);
  for (int k = 0; k < n; ++k) {
    const lins_keyposes_team_query& a = qs[k];
    lins_keyposes_result& r = results[k];
    r = lins_keyposes_result{O[k].n, O[k].hits, O[k].status, O[k].host};
    int32_t* mine = pairs + (size_t)k * stride * 2;
    if (!O[k].host) {
      m->ts_hits += (uint64_t)O[k].hits;
      if (!r.status && r.n) std::memcpy(mine, I + (size_t)k * stride * 2, (size_t)r.n * 2 * sizeof(int));
      continue;
    }
    m->ts_host += 1;  // the host text, with the same bits
    std::vector<std::vector<lins_key_pose>> keep((size_t)a.n_targets);
    std::vector<const lins_key_pose*> ptr((size_t)a.n_targets);
    std::vector<int32_t> cnt((size_t)a.n_targets);
    for (int t = 0; t < a.n_targets; ++t) {
      keep[t] = poses_of(m->frames[table[a.first_target + t]]);
      ptr[t] = keep[t].data(), cnt[t] = (int32_t)keep[t].size();
    }
    std::vector<lins_team_select::Pair> sel;
    long long hits = 0;
    const int rc = lins_team_select::select(a.n_targets, table + a.first_target, ptr.data(), cnt.data(), a.centre, a.radius, a.pose_leaf, sel, &hits);
    r.n = 0, r.hits = (int32_t)std::min<long long>(hits, INT_MAX);
    m->ts_hits += (uint64_t)hits;
    if (rc != lins_team_select::kOk || (int)sel.size() > stride) {
      r.status = LINS_E_CAPACITY;
      continue;
    }
    for (size_t i = 0; i < sel.size(); ++i) mine[2 * i] = sel[i].slot, mine[2 * i + 1] = sel[i].id;
    r.n = (int32_t)sel.size();
  }
  return LINS_OK;
}

}  // namespace

extern "C" {

int lins_keyposes_select_batch(lins_ctx* ctx, int n, const lins_keyposes_query* queries, int32_t* ids, int stride, lins_keyposes_result* results) {
  return kp_batch(ctx, kKpSelect, n, queries, nullptr, ids, stride, nullptr, nullptr, results);
}

int lins_keyposes_find_loop_batch(lins_ctx* ctx, int n, const lins_keyposes_loop_query* queries, int32_t* closest) {
  return kp_batch(ctx, kKpLoop, n, nullptr, queries, nullptr, 0, nullptr, closest, nullptr);
}

int lins_keyposes_surround_batch(lins_ctx* ctx, int n, const lins_keyposes_query* queries, int32_t* lists, int stride, int32_t* n_list,
                                 lins_keyposes_result* results) {
  return kp_batch(ctx, kKpSurround, n, queries, nullptr, lists, stride, n_list, nullptr, results);
}

int lins_keyposes_set_mode(lins_ctx* ctx, int mode) {
  if (!ctx || (mode != LINS_KEYPOSES_HOST && mode != LINS_KEYPOSES_DEVICE)) return LINS_E_ARG;
  archive_of(ctx)->kp_mode = mode;
  return LINS_OK;
}

int lins_keyposes_mode(lins_ctx* ctx) { return ctx ? archive_of(ctx)->kp_mode : LINS_E_ARG; }

int lins_keyposes_team_select_batch(lins_ctx* ctx, int n, const lins_keyposes_team_query* queries, const int32_t* targets, int n_table,
                                    int32_t* pairs, int stride, lins_keyposes_result* results) {
  return ts_batch(ctx, n, queries, targets, n_table, pairs, stride, results);
}

int lins_last_keyposes_team_stats(lins_ctx* ctx, float* device_ms, int32_t* host_entries, uint64_t* hits) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (device_ms) *device_ms = m->ts_ms;
  if (host_entries) *host_entries = m->ts_host;
  if (hits) *hits = m->ts_hits;
  return LINS_OK;
}

int lins_last_keyposes_stats(lins_ctx* ctx, float* device_ms, int32_t* host_entries, uint64_t* hits) {
  if (!ctx) return LINS_E_ARG;
  Archive* m = archive_of(ctx);
  if (device_ms) *device_ms = m->kp_ms;
  if (host_entries) *host_entries = m->kp_host;
  if (hits) *hits = m->kp_hits;
  return LINS_OK;
}

}  // extern "C"
