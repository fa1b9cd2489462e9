// lins_streams_map_capi.hip — C ABI of the mapping node's run() for streams (include/lins_streams_map.h
// lins_streams_map_*, lins_map_associate_batch): the per-stream map poses in one device block, the interval gate, and
// the order of LM:1821-1836 around the calls that already exist — the local-map build over the streams' clouds,
// scan-to-map between the two pose kernels (lins_map_capi.hip scan2map_local_resident), the key-frame pushes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/lins_lifecycle.h"
#include "../../include/lins_map.h"
#include "../../include/lins_streams_map.h"
#include "host/keyframe_select.h"
#include "keyframe_archive.h"
#include "lifecycle.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "local_map.h"
#include "snapshot.h"

using namespace lins;

static_assert(sizeof(MapPoseRec) == 8 * lins_snap::kRowMapPose, "the map pose record as the snapshot's plan copies it");

namespace {

struct StreamsMap {
  int n = 0;  // streams (0: lins_streams_map_init has not run)
  double interval = 0.3;
  bool use_archive = false;
  DevBuf<MapPoseRec> d_poses;  // [n]
  std::vector<double> last_time;  // timeLastProcessing per stream
  // one step's batch: entries up, result records down (pinned staging), n entries at most
  DevBuf<MapPoseEntry> d_entries;
  PinBuf<MapPoseEntry> h_entries;
  DevBuf<lins_map_step_result> d_out;
  PinBuf<lins_map_step_result> h_out;
  Event ev[4];  // associate start / end, finish start / end
  float associate_ms = 0.f, finish_ms = 0.f;
  // currentRobotPosPoint per stream (LM:1655-1658): transform[3..5] of its last entry with status OK
  std::vector<float> centre;   // [n][3]
  std::vector<char> stepped;   // [n]
  // lins_streams_map_loop: the step feeds the pose graph; transformLast per stream mirrored on the host
  bool loop = false;
  std::vector<float> last6;    // [n][6]
  // lins_streams_map_surround: the local map is the surrounding key frames of the archive; the list per stream
  bool surround = false;
  float radius = 50.f, pose_leaf = 1.f;
  std::vector<std::vector<int>> lists;  // [n] surroundingExistingKeyPosesID
  // lins_streams_map_team: the local map is the team selection over the slots of the stream's group.  A context setting
  // like the modes above; the selection is a pure function of the key poses and the centre, so nothing persists per
  // stream but the record of the last list (read back by lins_streams_map_team_list, an input to nothing)
  bool team = false;
  float team_radius = 50.f, team_leaf = 1.f;
  std::vector<int32_t> groups;                       // [n] >= 0: the slots of one map frame; -1: the slot alone
  std::vector<std::vector<int32_t>> team_lists;      // [n] (slot, id) pairs of the stream's last build
  // a write-back's batch (lins_pose_graph_apply_batch): n entries at most
  DevBuf<MapPoseFix> d_fix;
  PinBuf<MapPoseFix> h_fix;
  // lins_map_associate_batch's own buffers (grown together, never shrunk; d_ab_poses answers)
  DevBuf<MapPoseRec> d_ab_poses;
  DevBuf<MapPoseEntry> d_ab_entries;
  DevBuf<lins_map_step_result> d_ab_out;
};

void step_buffers_free(StreamsMap* m) {
  m->d_poses.reset(), m->d_entries.reset(), m->d_out.reset(), m->d_fix.reset();
  m->h_entries.reset(), m->h_out.reset(), m->h_fix.reset();
  m->n = 0;
  m->loop = m->surround = m->team = false;
}

void streams_map_free(void* p) { delete (StreamsMap*)p; }

StreamsMap* state_of(lins_ctx* ctx) {
  void** slot = map_slot(ctx, kSlotPose, streams_map_free);
  if (!*slot) *slot = new StreamsMap();
  return (StreamsMap*)*slot;
}

bool finite6(const float* v) {
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

lins_key_pose key_pose_of(const float* t) { return lins_key_pose{t[3], t[4], t[5], t[0], t[1], t[2]}; }  // LM:1721-1732

}  // namespace

namespace lins {
int streams_map_streams(lins_ctx* ctx) { return state_of(ctx)->n; }
const MapPoseRec* streams_map_poses(lins_ctx* ctx) { return state_of(ctx)->d_poses; }

int streams_map_centre(lins_ctx* ctx, int stream, float centre[3]) {
  StreamsMap* m = state_of(ctx);
  if (stream < 0 || stream >= m->n) return LINS_E_ARG;
  if (!m->stepped[stream]) return LINS_E_STATE;
  std::memcpy(centre, &m->centre[3 * (size_t)stream], 3 * sizeof(float));
  return LINS_OK;
}

int streams_map_correct(lins_ctx* ctx, int n, const int32_t* streams, const float* six) {
  StreamsMap* m = state_of(ctx);
  if (n < 0 || n > m->n) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  for (int k = 0; k < n; ++k)
    if (streams[k] < 0 || streams[k] >= m->n || !finite6(six + 6 * k)) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  for (int k = 0; k < n; ++k) {
    MapPoseFix& f = m->h_fix[k];
    f.stream = streams[k], f.pad = 0;
    std::memcpy(f.p, six + 6 * k, sizeof f.p);
  }
  HIP_TRY(ctx, hipMemcpyAsync(m->d_fix, m->h_fix, (size_t)n * sizeof(MapPoseFix), hipMemcpyHostToDevice, st));
  launch_map_pose_correct(st, n, m->d_fix, m->d_poses);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (the next batch refills h_fix)
  if (m->loop)
    for (int k = 0; k < n; ++k) std::memcpy(&m->last6[6 * (size_t)streams[k]], six + 6 * k, 6 * sizeof(float));
  return LINS_OK;
}

// (lifecycle.h) the streams named as lins_streams_map_init leaves them: allocateMemory's map pose (LM:305-409),
// timeLastProcessing = -1 (LM:356), no currentRobotPosPoint, no surrounding key poses; the context's modes stay
int streams_map_release_apply(lins_ctx* ctx, int n, const int32_t* streams) {
  StreamsMap* m = state_of(ctx);
  hipStream_t st = ctx_stream(ctx);
  for (int k = 0; k < n; ++k) {
    const size_t s = (size_t)streams[k];
    HIP_TRY(ctx, hipMemsetAsync(m->d_poses + s, 0, sizeof(MapPoseRec), st));
    m->last_time[s] = -1.0;
    std::fill(m->centre.begin() + 3 * s, m->centre.begin() + 3 * s + 3, 0.f);
    m->stepped[s] = 0;
    std::fill(m->last6.begin() + 6 * s, m->last6.begin() + 6 * s + 6, 0.f);
    m->lists[s].clear();
    m->groups[s] = -1, m->team_lists[s].clear();
  }
  if (n) HIP_TRY(ctx, hipStreamSynchronize(st));
  return LINS_OK;
}

// ---- snapshot.h: the same fields.  The map pose record travels as 14 units of 8 bytes through the kernel.
void streams_map_snapshot_context(lins_ctx* ctx, SnapContext& c) {
  StreamsMap* m = state_of(ctx);
  if (!m->n) return;
  c.modules |= LINS_SNAP_MAP_POSE;
  c.facts.map_interval = m->interval, c.facts.loop = m->loop ? 1 : 0, c.facts.surround = m->surround ? 1 : 0;
  if (m->surround) c.facts.surround_radius = m->radius, c.facts.surround_pose_leaf = m->pose_leaf;
  c.base[LINS_SNAP_BUF_MAP_POSE] = m->d_poses.get(), c.units[LINS_SNAP_BUF_MAP_POSE] = (int64_t)lins_snap::kRowMapPose * m->n;
}

int streams_map_snapshot_describe(lins_ctx* ctx, int stream, SnapStream& s) {
  StreamsMap* m = state_of(ctx);
  const size_t k = (size_t)stream;
  s.modules |= LINS_SNAP_MAP_POSE;
  lins_snapshot_stream_rec* r = (lins_snapshot_stream_rec*)s.host[LINS_SNAP_SEC_STREAM_REC].data();
  r->map_last_time = m->last_time[k], r->stepped = m->stepped[k] ? 1 : 0;
  std::memcpy(r->centre, &m->centre[3 * k], sizeof r->centre);
  std::memcpy(r->last6, &m->last6[6 * k], sizeof r->last6);
  s.counts.surround = (int32_t)m->lists[k].size();
  int32_t* ids = s.host_section<int32_t>(LINS_SNAP_SEC_SURROUND, m->lists[k].size());
  std::copy(m->lists[k].begin(), m->lists[k].end(), ids);
  return LINS_OK;
}

int streams_map_restore_check(lins_ctx* ctx, int stream, lins_snapshot_limits& lim) {
  StreamsMap* m = state_of(ctx);
  const size_t k = (size_t)stream;
  if (m->last_time[k] != -1.0 || m->stepped[k] || !m->lists[k].empty()) return LINS_E_STATE;
  lim.surround_max = 0x7fffffff;  // (the list names key frames: bounded by the archive's frames, which the format checks)
  return LINS_OK;
}

void streams_map_restore_apply(lins_ctx* ctx, int stream, const SnapView& v) {
  StreamsMap* m = state_of(ctx);
  const size_t k = (size_t)stream;
  lins_snapshot_stream_rec r;
  std::memcpy(&r, v.sec(LINS_SNAP_SEC_STREAM_REC), sizeof r);
  m->last_time[k] = r.map_last_time, m->stepped[k] = (char)r.stepped;
  std::memcpy(&m->centre[3 * k], r.centre, sizeof r.centre);
  std::memcpy(&m->last6[6 * k], r.last6, sizeof r.last6);
  m->lists[k].assign((size_t)v.info.counts.surround, 0);
  if (v.info.counts.surround) std::memcpy(m->lists[k].data(), v.sec(LINS_SNAP_SEC_SURROUND), 4 * (size_t)v.info.counts.surround);
}
}  // namespace lins

extern "C" {

int lins_streams_map_release(lins_ctx* ctx, int n, const int32_t* streams) {
  if (!ctx) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (int rc = release_list_check(n, streams, m->n)) return rc;
  if (int rc = ctx_quiesce(ctx)) return rc;
  return streams_map_release_apply(ctx, n, streams);
}

int lins_map_associate_batch(lins_ctx* ctx, int n, const float* bef6, const float* aft6, const float* sum6, float* tobe6) {
  if (!ctx || n < 0 || (n && (!bef6 || !aft6 || !sum6 || !tobe6))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  for (int k = 0; k < n; ++k)
    if (!finite6(bef6 + 6 * k) || !finite6(aft6 + 6 * k) || !finite6(sum6 + 6 * k)) return LINS_E_INPUT;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  StreamsMap* m = state_of(ctx);
  BUF_TRY(ctx, grow_all(m->d_ab_poses, (size_t)n, m->d_ab_entries, (size_t)n, m->d_ab_out, (size_t)n));
  std::vector<MapPoseRec> recs((size_t)n, MapPoseRec{});
  std::vector<MapPoseEntry> ent((size_t)n, MapPoseEntry{});
  std::vector<lins_map_step_result> res((size_t)n);
  for (int k = 0; k < n; ++k) {
    std::memcpy(recs[k].bef, bef6 + 6 * k, sizeof recs[k].bef);
    std::memcpy(recs[k].aft, aft6 + 6 * k, sizeof recs[k].aft);
    std::memcpy(ent[k].sum, sum6 + 6 * k, sizeof ent[k].sum);
    ent[k].stream = k;
  }
  hipStream_t st = ctx_stream(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(m->d_ab_poses, recs.data(), (size_t)n * sizeof(MapPoseRec), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(m->d_ab_entries, ent.data(), (size_t)n * sizeof(MapPoseEntry), hipMemcpyHostToDevice, st));
  launch_map_associate(st, n, m->d_ab_entries, nullptr, m->d_ab_poses, nullptr, m->d_ab_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(res.data(), m->d_ab_out, (size_t)n * sizeof(lins_map_step_result), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int k = 0; k < n; ++k) std::memcpy(tobe6 + 6 * k, res[k].tobe_start, 6 * sizeof(float));
  return LINS_OK;
}

int lins_streams_map_init(lins_ctx* ctx, int n_streams, double process_interval) {
  if (!ctx || n_streams < 1 || !(process_interval >= 0.0) || !std::isfinite(process_interval)) return LINS_E_ARG;
  if (streams_count(ctx) < n_streams || local_map_slots(ctx) < n_streams) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  StreamsMap* m = state_of(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));
  step_buffers_free(m);
  for (Event& e : m->ev) BUF_TRY(ctx, e.create());
  BUF_TRY(ctx, m->d_poses.grow((size_t)n_streams));
  BUF_TRY(ctx, m->d_entries.grow((size_t)n_streams));
  BUF_TRY(ctx, m->d_out.grow((size_t)n_streams));
  BUF_TRY(ctx, m->h_entries.grow((size_t)n_streams));
  BUF_TRY(ctx, m->h_out.grow((size_t)n_streams));
  BUF_TRY(ctx, m->d_fix.grow((size_t)n_streams));
  BUF_TRY(ctx, m->h_fix.grow((size_t)n_streams));
  HIP_TRY(ctx, hipMemsetAsync(m->d_poses, 0, (size_t)n_streams * sizeof(MapPoseRec), ctx_stream(ctx)));  // allocateMemory (LM:305-409)
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));
  m->last_time.assign((size_t)n_streams, -1.0);  // LM:356
  m->centre.assign(3 * (size_t)n_streams, 0.f), m->stepped.assign((size_t)n_streams, 0);
  m->last6.assign(6 * (size_t)n_streams, 0.f);
  m->lists.assign((size_t)n_streams, {});
  m->groups.assign((size_t)n_streams, -1), m->team_lists.assign((size_t)n_streams, {});
  m->interval = process_interval;
  m->use_archive = lins_archive_count(ctx, 0) >= 0;
  m->associate_ms = m->finish_ms = 0.f;
  m->n = n_streams;
  streams_slam_reset(ctx);  // (lins_streams_fuse: no records of an earlier run against the new poses)
  return LINS_OK;
}

int lins_streams_map_get_pose(lins_ctx* ctx, int stream, lins_map_pose_state* out) {
  if (!ctx || !out) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (stream < 0 || stream >= m->n) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  MapPoseRec r;
  HIP_TRY(ctx, hipMemcpyAsync(&r, m->d_poses + stream, sizeof r, hipMemcpyDeviceToHost, ctx_stream(ctx)));
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));
  static_assert(offsetof(lins_map_pose_state, n_frames) == offsetof(MapPoseRec, n_frames), "the record is the state's head");
  std::memcpy(out, &r, sizeof r);
  out->last_time = m->last_time[stream];
  return LINS_OK;
}

int lins_streams_map_set_pose(lins_ctx* ctx, int stream, const lins_map_pose_state* in) {
  if (!ctx || !in) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (stream < 0 || stream >= m->n) return LINS_E_ARG;
  if (!finite6(in->bef) || !finite6(in->aft) || !finite6(in->tobe) || !finite6(in->last) || !std::isfinite(in->prev[0]) ||
      !std::isfinite(in->prev[1]) || !std::isfinite(in->prev[2]) || in->n_frames < 0 || !std::isfinite(in->last_time))
    return LINS_E_INPUT;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  MapPoseRec r;
  std::memcpy(&r, in, sizeof r);
  HIP_TRY(ctx, hipMemcpyAsync(m->d_poses + stream, &r, sizeof r, hipMemcpyHostToDevice, ctx_stream(ctx)));
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));  // (r goes out of scope)
  m->last_time[stream] = in->last_time;
  if (m->loop) std::memcpy(&m->last6[6 * (size_t)stream], in->last, sizeof in->last);
  return LINS_OK;
}

int lins_streams_map_loop(lins_ctx* ctx, int on) {
  if (!ctx) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (!on) {
    m->loop = false;
    return LINS_OK;
  }
  if (m->surround || !m->use_archive || pose_graph_slots(ctx) < m->n) return LINS_E_STATE;
  for (int s = 0; s < m->n; ++s) {
    const int in_archive = lins_archive_count(ctx, s);  // (an archive re-sized below the streams: no such slot)
    if (in_archive < 0 || in_archive != lins_pose_graph_count(ctx, s, nullptr)) return LINS_E_STATE;
  }
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  std::vector<MapPoseRec> recs((size_t)m->n);
  HIP_TRY(ctx, hipMemcpyAsync(recs.data(), m->d_poses, recs.size() * sizeof(MapPoseRec), hipMemcpyDeviceToHost, ctx_stream(ctx)));
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));
  for (int s = 0; s < m->n; ++s) std::memcpy(&m->last6[6 * (size_t)s], recs[s].last, sizeof recs[s].last);
  m->loop = true;
  return LINS_OK;
}

int lins_streams_map_surround(lins_ctx* ctx, int on, float radius, float pose_leaf) {
  if (!ctx) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (!on) {
    m->surround = false;
    return LINS_OK;
  }
  if (!std::isfinite(radius) || radius < 0.f || !(pose_leaf > 0.f) || !std::isfinite(pose_leaf)) return LINS_E_ARG;
  if (m->loop || m->team || !m->use_archive) return LINS_E_STATE;
  for (int s = 0; s < m->n; ++s)
    if (lins_archive_count(ctx, s) < 0) return LINS_E_STATE;  // (an archive re-sized below the streams: no such slot)
  for (std::vector<int>& l : m->lists) l.clear();
  m->surround = true, m->radius = radius, m->pose_leaf = pose_leaf;
  return LINS_OK;
}

int lins_streams_map_surround_list(lins_ctx* ctx, int stream, int32_t* ids, int cap) {
  if (!ctx || cap < 0) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (stream < 0 || stream >= m->n) return LINS_E_ARG;
  const std::vector<int>& l = m->lists[stream];
  if ((int)l.size() > cap) return LINS_E_CAPACITY;
  if (!l.empty() && !ids) return LINS_E_ARG;
  for (size_t i = 0; i < l.size(); ++i) ids[i] = l[i];
  return (int)l.size();
}

int lins_streams_map_team(lins_ctx* ctx, int on, float radius, float pose_leaf) {
  if (!ctx) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (!on) {
    m->team = false;
    return LINS_OK;
  }
  if (!std::isfinite(radius) || radius < 0.f || !(pose_leaf > 0.f) || !std::isfinite(1.0f / pose_leaf)) return LINS_E_ARG;
  if (m->surround || !m->use_archive) return LINS_E_STATE;
  for (int s = 0; s < m->n; ++s)
    if (lins_archive_count(ctx, s) < 0) return LINS_E_STATE;  // (an archive re-sized below the streams: no such slot)
  for (std::vector<int32_t>& l : m->team_lists) l.clear();
  m->team = true, m->team_radius = radius, m->team_leaf = pose_leaf;
  return LINS_OK;
}

int lins_streams_map_team_groups(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* groups) {
  if (!ctx || n < 0 || (n && (!slots || !groups))) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  for (int k = 0; k < n; ++k)
    if (slots[k] < 0 || slots[k] >= m->n || groups[k] < -1) return LINS_E_ARG;
  for (int k = 0; k < n; ++k) m->groups[slots[k]] = groups[k];
  return LINS_OK;
}

int lins_streams_map_team_group(lins_ctx* ctx, int slot, int32_t* group) {
  if (!ctx || !group) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n) return LINS_E_ARG;
  *group = m->groups[slot];
  return LINS_OK;
}

int lins_streams_map_team_list(lins_ctx* ctx, int stream, int32_t* pairs, int cap) {
  if (!ctx || cap < 0) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (stream < 0 || stream >= m->n) return LINS_E_ARG;
  const std::vector<int32_t>& l = m->team_lists[stream];
  if ((int)(l.size() / 2) > cap) return LINS_E_CAPACITY;
  if (!l.empty() && !pairs) return LINS_E_ARG;
  std::copy(l.begin(), l.end(), pairs);
  return (int)(l.size() / 2);
}

int lins_streams_map_step(lins_ctx* ctx, int n, const int32_t* streams, const lins_map_odom* odom, lins_map_step_result* out) {
  if (!ctx || n < 0 || (n && (!streams || !odom || !out))) return LINS_E_ARG;
  return streams_map_step_run(ctx, n, streams, MapStepIn{odom, nullptr, nullptr, nullptr, nullptr}, out);
}

}  // extern "C"

// run() for the entries named: the body of lins_streams_map_step and lins_streams_map_step_resident (local_map.h MapStepIn)
int lins::streams_map_step_run(lins_ctx* ctx, int n, const int32_t* streams, const MapStepIn& in, lins_map_step_result* out) {
  const lins_map_odom* odom = in.odom;
  StreamsMap* m = state_of(ctx);
  if (!m->n) return LINS_E_STATE;
  if (n > m->n) return LINS_E_ARG;
  for (int k = 0; k < n; ++k) {
    if (streams[k] < 0 || streams[k] >= m->n) return LINS_E_ARG;
    for (int i = 0; i < k; ++i)
      if (streams[i] == streams[k]) return LINS_E_ARG;  // (a stream may appear once)
  }
  for (int k = 0; k < n; ++k) {
    if (odom) {
      const lins_map_odom& o = odom[k];
      if (!finite6(o.transform_sum) || !std::isfinite(o.time) || !std::isfinite(o.imu_roll) || !std::isfinite(o.imu_pitch)) return LINS_E_INPUT;
    } else if (!std::isfinite(in.time[k]) || (in.imu && (!std::isfinite(in.imu[k].roll) || !std::isfinite(in.imu[k].pitch))))
      return LINS_E_INPUT;
  }
  auto time_of = [&](int k) { return odom ? odom[k].time : in.time[k]; };
  m->associate_ms = m->finish_ms = 0.f;
  // the interval gate (LM:1821), f64
  std::vector<int> batch;     // positions in the call of the entries that run
  std::vector<int32_t> which;  // ... and their streams = their slots
  std::vector<std::vector<int32_t>> lists;  // surround mode: the list each of them builds its map from
  auto gate = [&](int k) {
    const bool no_record = !odom && !in.h_odom[streams[k]].valid;  // (the stream has no pose to map with: refused, entry alone)
    return no_record ? LINS_E_INPUT : time_of(k) - m->last_time[streams[k]] >= m->interval ? LINS_OK : LINS_MAP_STEP_SKIPPED;
  };
  // LINS_KEYPOSES_DEVICE: the selection and the list rule of every gated entry in one lins_keyposes_surround_batch
  const bool on_device = m->surround && lins_keyposes_mode(ctx) == LINS_KEYPOSES_DEVICE;
  std::vector<int> dev_at(on_device ? (size_t)n : 0, -1);  // position k of the call -> its entry of the batched selection
  std::vector<int32_t> dev_lists, dev_n;
  std::vector<lins_keyposes_result> dev_res;
  int dev_stride = 1;
  if (on_device) {
    std::vector<lins_keyposes_query> qs;
    for (int k = 0; k < n; ++k) {
      if (gate(k)) continue;
      const int s = streams[k], have = lins_archive_count(ctx, s);
      if (have < 0) return LINS_E_STATE;
      dev_at[k] = (int)qs.size();
      qs.push_back(lins_keyposes_query{s, {m->centre[3 * (size_t)s], m->centre[3 * (size_t)s + 1], m->centre[3 * (size_t)s + 2]}, m->radius, m->pose_leaf});
      dev_stride = std::max(dev_stride, have + (have ? (int)m->lists[s].size() : 0));  // (survivors + selection: no longer)
    }
    const int nq = (int)qs.size();
    dev_lists.assign((size_t)nq * dev_stride, 0), dev_n.assign((size_t)nq, 0), dev_res.resize((size_t)nq);
    for (int j = 0; j < nq; ++j) {
      const std::vector<int>& l = m->lists[qs[j].slot];
      if (lins_archive_count(ctx, qs[j].slot) == 0) continue;  // (LM:1202: no key poses, nothing listed)
      dev_n[j] = (int32_t)l.size();
      std::copy(l.begin(), l.end(), dev_lists.begin() + (size_t)j * dev_stride);
    }
    if (int rc = lins_keyposes_surround_batch(ctx, nq, qs.data(), dev_lists.data(), dev_stride, dev_n.data(), dev_res.data())) return rc;
  }
  // team mode: the targets of every gated entry are the slots of its stream's group, the centre the remembered
  // currentRobotPosPoint; one selection for the batch — the batched device call or the host text, the same bits
  std::vector<int> team_at(m->team ? (size_t)n : 0, -1);  // position k of the call -> its entry of the selection
  std::vector<std::vector<int32_t>> team_sel;             // per selection entry: its (slot, id) pairs
  std::vector<int> team_status;
  if (m->team) {
    std::vector<lins_keyposes_team_query> qs;
    std::vector<int32_t> table;
    long long stride = 1;
    for (int k = 0; k < n; ++k) {
      if (gate(k)) continue;
      const int s = streams[k];
      lins_keyposes_team_query q{{m->centre[3 * (size_t)s], m->centre[3 * (size_t)s + 1], m->centre[3 * (size_t)s + 2]}, m->team_radius, m->team_leaf,
                                 0, (int32_t)table.size(), 0};
      long long frames = 0;
      for (int t = 0; t < m->n; ++t) {
        if (t != s && (m->groups[s] < 0 || m->groups[t] != m->groups[s])) continue;
        const int have = lins_archive_count(ctx, t);
        if (have < 0) return LINS_E_STATE;
        table.push_back(t), q.n_targets += 1, frames += have;
      }
      stride = std::max(stride, frames);
      team_at[k] = (int)qs.size();
      qs.push_back(q);
    }
    const int nq = (int)qs.size();
    team_sel.resize((size_t)nq), team_status.assign((size_t)nq, LINS_OK);
    if (nq && lins_keyposes_mode(ctx) == LINS_KEYPOSES_DEVICE) {
      if (stride > INT_MAX / 2 / nq) return LINS_E_CAPACITY;
      std::vector<int32_t> pairs((size_t)nq * (size_t)stride * 2);
      std::vector<lins_keyposes_result> res((size_t)nq);
      if (int rc = lins_keyposes_team_select_batch(ctx, nq, qs.data(), table.data(), (int)table.size(), pairs.data(), (int)stride, res.data())) return rc;
      for (int j = 0; j < nq; ++j) {
        team_status[j] = res[j].status;
        if (!res[j].status) team_sel[j].assign(pairs.begin() + (size_t)j * stride * 2, pairs.begin() + ((size_t)j * stride + res[j].n) * 2);
      }
    } else {
      for (int j = 0; j < nq; ++j)
        if ((team_status[j] = archive_team_select_host(ctx, qs[j].n_targets, table.data() + qs[j].first_target, qs[j].centre, qs[j].radius,
                                                       qs[j].pose_leaf, team_sel[j])) < 0 && team_status[j] != LINS_E_CAPACITY)
          return team_status[j];
    }
  }
  for (int k = 0; k < n; ++k) {
    int refused = gate(k);
    if (!refused && m->team) {
      const int j = team_at[k];
      if (team_status[j] == LINS_E_CAPACITY) {
        refused = LINS_E_CAPACITY;  // (the selection's box: the entry alone)
      } else if (team_status[j]) {
        return team_status[j];
      } else {
        lists.emplace_back(std::move(team_sel[j]));
      }
    } else if (!refused && on_device) {
      const int j = dev_at[k];
      if (dev_res[j].status == LINS_E_CAPACITY) {
        refused = LINS_E_CAPACITY;  // (the selection's box: the entry alone)
      } else if (dev_res[j].status) {
        return dev_res[j].status;
      } else {
        lists.emplace_back(dev_lists.begin() + (size_t)j * dev_stride, dev_lists.begin() + (size_t)j * dev_stride + dev_n[j]);
      }
    } else if (!refused && m->surround) {  // LM:1247-1308: the radius selection around currentRobotPosPoint, then the list rule
      const int s = streams[k], have = lins_archive_count(ctx, s);
      if (have < 0) return LINS_E_STATE;
      std::vector<int32_t> ds((size_t)std::max(have, 1));
      const int nd = have ? lins_archive_select_radius(ctx, s, &m->centre[3 * (size_t)s], m->radius, m->pose_leaf, ds.data(), have) : 0;
      if (nd == LINS_E_CAPACITY) {
        refused = LINS_E_CAPACITY;  // (the selection's box: the entry alone)
      } else if (nd < 0) {
        return nd;
      } else {
        std::vector<int> list = have ? m->lists[s] : std::vector<int>();  // (LM:1202: no key poses, nothing listed)
        lins_select::surround_update(list, std::vector<int>(ds.begin(), ds.begin() + nd));
        lists.emplace_back(list.begin(), list.end());
      }
    }
    if (!refused) {
      batch.push_back(k), which.push_back(streams[k]);
    } else {
      out[k] = lins_map_step_result{};
      out[k].status = refused, out[k].ring_age = -1, out[k].archive_id = -1;
    }
  }
  const int nb = (int)batch.size();
  if (nb == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  for (int j = 0; j < nb; ++j) {
    MapPoseEntry& e = m->h_entries[j];
    if (odom) {
      const lins_map_odom& o = odom[batch[j]];
      std::memcpy(e.sum, o.transform_sum, sizeof e.sum);
      e.imu_roll = o.imu_roll, e.imu_pitch = o.imu_pitch, e.has_imu = o.has_imu != 0;
    } else {  // (transformSum: the kernels read the resident record of the stream)
      std::memset(e.sum, 0, sizeof e.sum);
      const lins_slam_imu none{0.f, 0.f, 0, 0};
      const lins_slam_imu& a = in.imu ? in.imu[batch[j]] : none;
      e.imu_roll = a.roll, e.imu_pitch = a.pitch, e.has_imu = a.has_imu != 0;
    }
    e.stream = which[j];
  }
  HIP_TRY(ctx, hipMemcpyAsync(m->d_entries, m->h_entries, (size_t)nb * sizeof(MapPoseEntry), hipMemcpyHostToDevice, st));
  // extractSurroundingKeyFrames + downsampleCurrentScan over the streams' clouds where they lie
  int rc;
  if (m->team) {
    std::vector<const int32_t*> idp((size_t)nb);
    std::vector<int32_t> idn((size_t)nb);
    std::vector<lins_local_map_sizes> sizes((size_t)nb);
    for (int j = 0; j < nb; ++j) idp[j] = lists[j].data(), idn[j] = (int32_t)(lists[j].size() / 2);
    if ((rc = lins_local_map_build_team_streams(ctx, nb, which.data(), idp.data(), idn.data(), which.data(), sizes.data()))) return rc;
    for (int j = 0; j < nb; ++j)  // (the record of the last build; an input to nothing)
      if (!sizes[j].status) m->team_lists[which[j]] = lists[j];
  } else if (m->surround) {
    std::vector<const int32_t*> idp((size_t)nb);
    std::vector<int32_t> idn((size_t)nb);
    std::vector<lins_local_map_sizes> sizes((size_t)nb);
    for (int j = 0; j < nb; ++j) idp[j] = lists[j].data(), idn[j] = (int32_t)lists[j].size();
    if ((rc = lins_local_map_build_surround_streams(ctx, nb, which.data(), idp.data(), idn.data(), which.data(), sizes.data()))) return rc;
    for (int j = 0; j < nb; ++j)  // (a build entry with a status keeps its list)
      if (!sizes[j].status) m->lists[which[j]].assign(lists[j].begin(), lists[j].end());
  } else if ((rc = lins_local_map_build_streams(ctx, nb, which.data(), which.data(), nullptr))) {
    return rc;
  }
  // transformAssociateToMap, scan2MapOptimization, transformUpdate, the key-frame rule
  hipEvent_t ev[4] = {m->ev[0], m->ev[1], m->ev[2], m->ev[3]};
  if ((rc = scan2map_local_resident(ctx, nb, m->d_entries, m->d_poses, m->d_out, m->h_out, ev, odom ? nullptr : in.d_odom))) return rc;
  HIP_TRY(ctx, hipEventElapsedTime(&m->associate_ms, m->ev[0], m->ev[1]));
  HIP_TRY(ctx, hipEventElapsedTime(&m->finish_ms, m->ev[2], m->ev[3]));
  std::vector<int32_t> key_entries;
  std::vector<lins_key_pose> key_poses;
  std::vector<double> key_times;
  for (int j = 0; j < nb; ++j) {
    const int k = batch[j];
    out[k] = m->h_out[j];
    if (out[k].status == LINS_OK) {
      m->last_time[which[j]] = time_of(k);  // LM:1824
      std::memcpy(&m->centre[3 * (size_t)which[j]], out[k].transform + 3, 3 * sizeof(float));  // LM:1655-1658
      m->stepped[which[j]] = 1;
    }
    if (out[k].key_frame) key_entries.push_back(j), key_poses.push_back(key_pose_of(out[k].key_pose)), key_times.push_back(time_of(k));
  }
  // saveKeyFramesAndFactor's cloud copies (LM:1751-1764), device to device
  const int nk = (int)key_entries.size();
  if (nk && m->loop) {  // every refusal of the graph is asked before a frame is stored anywhere
    for (int i = 0; i < nk; ++i) {
      const int s = which[key_entries[i]];
      int frames_left = 0;
      pose_graph_room(ctx, s, &frames_left, nullptr, nullptr, nullptr);
      if (lins_pose_graph_count(ctx, s, nullptr) != lins_archive_count(ctx, s)) return LINS_E_STATE;
      if (frames_left < 1) return LINS_E_CAPACITY;
    }
  }
  if (nk) {
    if ((rc = lins_local_map_push_scans(ctx, nk, key_entries.data(), key_poses.data()))) return rc;
    std::vector<int32_t> ids((size_t)nk, -1);
    if (m->use_archive && (rc = lins_archive_push_scans(ctx, nk, key_entries.data(), key_poses.data(), key_times.data(), ids.data()))) return rc;
    for (int i = 0; i < nk; ++i) {
      lins_map_step_result& r = out[batch[key_entries[i]]];
      r.ring_age = 0, r.archive_id = ids[i];
      if (m->loop) {  // saveKeyFramesAndFactor's factor (LM:1673-1705): the first frame's key pose is transformTobeMapped, the prior
        float* last = &m->last6[6 * (size_t)which[key_entries[i]]];
        const int id = lins_pose_graph_push(ctx, which[key_entries[i]], last, r.key_pose);
        if (id < 0) return id;
        if (id != ids[i]) return LINS_E_STATE;
        std::memcpy(last, r.key_pose, 6 * sizeof(float));  // mp_key_pose: transformLast = the key pose
      }
    }
  }
  return LINS_OK;
}

extern "C" {

int lins_last_streams_map_ms(lins_ctx* ctx, float* associate_ms, float* finish_ms) {
  if (!ctx) return LINS_E_ARG;
  StreamsMap* m = state_of(ctx);
  if (associate_ms) *associate_ms = m->associate_ms;
  if (finish_ms) *finish_ms = m->finish_ms;
  return LINS_OK;
}

}  // extern "C"
