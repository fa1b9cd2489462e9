// lins_local_map_capi.hip — C ABI of the mapping node's local map on the device (include/lins_map.h lins_local_map_*):
// the key-frame rings, the packing of a build into the VoxelGrid jobs of local_map_kernels.hip, and the view scan-to-map
// reads the built clouds through (LINS_MAP_LOCAL).  A build's map side is the ring of the entry's slot, or — the
// surround builds — a list of frames of the key-frame archive (keyframe_archive.h ArchiveStore).  The rings hold the key frames in the sensor frame; the host keeps
// their counts, poses and trigonometry (std::cos / std::sin of float, once per pose, LM:612-624).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lins_lifecycle.h"
#include "../../include/lins_map.h"
#include "keyframe_archive.h"
#include "lifecycle.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "local_map.h"
#include "snapshot.h"

using namespace lins;

namespace {

struct KeyFrame {
  int n[3];  // corner, surf, outlier (stored one after the other in the frame's block of the ring)
  lins_key_pose pose;
  float t[9];  // ctRoll, stRoll, ctPitch, stPitch, ctYaw, stYaw, tInX, tInY, tInZ
};

struct LocalMap {
  int n_slots = 0, window = 0, max_pts = 0;
  DevBuf<float4> d_frames;  // [slot][window][max_pts]
  std::vector<KeyFrame> meta;  // [slot][window]
  std::vector<int> head, count;
  // build arenas (grown, never shrunk)
  DevBuf<float4> d_stage, d_out;
  DevBuf<unsigned> d_ka, d_kb;  // (d_stage, d_ka, d_kb, d_va, d_vb, d_starts: one group, d_stage answers)
  DevBuf<int> d_va, d_vb, d_starts, d_hist, d_tilecnt, d_csum;  // (d_hist, d_tilecnt: one group, d_hist answers)
  DevBuf<char> d_tab;  // (bytes)
  PinBuf<float4> h_raw;
  PinBuf<char> h_tab, h_states;  // (bytes)
  // the last build
  bool built = false;
  std::vector<int> slots;
  std::vector<long long> off;  // 6 per entry
  std::vector<lins_local_map_sizes> sizes;
  float ms = 0.f, stage_ms = 0.f;  // stage_ms: the staging kernel of lins_local_map_build_streams (inside ms)
  Event ev_stage;
  uint64_t points_in = 0;
};

void local_free(void* p) { delete (LocalMap*)p; }

LocalMap* local_of(lins_ctx* ctx) {
  void** slot = map_slot(ctx, kSlotLocal, local_free);
  if (!*slot) *slot = new LocalMap();
  return (LocalMap*)*slot;
}

bool point_ok(const lins_point& p) {
  return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::fabs(p.x) <= 1e6f && std::fabs(p.y) <= 1e6f &&
         std::fabs(p.z) <= 1e6f;
}
int cloud_check(const lins_point* p, int n) {
  if (n < 0 || (n && !p)) return LINS_E_ARG;
  for (int i = 0; i < n; ++i)
    if (!point_ok(p[i])) return LINS_E_INPUT;
  return LINS_OK;
}
bool pose_ok(const lins_key_pose& p) {
  const float v[6] = {p.x, p.y, p.z, p.roll, p.pitch, p.yaw};
  for (float x : v)
    if (!std::isfinite(x)) return false;
  return std::fabs(p.x) <= 1e6f && std::fabs(p.y) <= 1e6f && std::fabs(p.z) <= 1e6f;
}
void set_pose(KeyFrame& f, const lins_key_pose& p) {  // updateTransformPointCloudSinCos (LM:612-624)
  f.pose = p;
  const float t[9] = {std::cos(p.roll), std::sin(p.roll), std::cos(p.pitch), std::sin(p.pitch), std::cos(p.yaw), std::sin(p.yaw), p.x, p.y, p.z};
  std::memcpy(f.t, t, sizeof t);
}

// the ring position a new key frame of `slot` goes to (a full ring drops its oldest, LM:1226-1240)
int ring_push(LocalMap* m, int slot) {
  int& h = m->head[slot];
  int& c = m->count[slot];
  if (c < m->window) return (h + c++) % m->window;
  const int idx = h;
  h = (h + 1) % m->window;
  return idx;
}
float4* frame_ptr(LocalMap* m, int slot, int idx) { return m->d_frames + ((size_t)slot * m->window + idx) * m->max_pts; }

size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// the map side of a build: the rings (ids null), or per entry the list ids[k][0 .. n_ids[k]) of frames of the archive
// slot slots[k], in list order (ar: the store they lie in)
struct MapSource {
  const int32_t* const* ids = nullptr;  // entry k's list: ids of its own slot, or (pairs) (slot, id) pairs
  const int32_t* n_ids = nullptr;
  bool pairs = false;
  ArchiveStore ar{};
  // the i-th listed frame of entry k, whose own slot is s
  const ArFrame& frame(int k, int s, int i) const {
    return pairs ? (*ar.frames)[ids[k][2 * i]][ids[k][2 * i + 1]] : (*ar.frames)[s][ids[k][i]];
  }
};

}  // namespace

namespace lins {
int local_map_view(lins_ctx* ctx, LocalMapView* v) {
  LocalMap* m = local_of(ctx);
  if (!m->built) return LINS_E_STATE;
  v->d_out = m->d_out, v->n = (int)m->slots.size(), v->off = m->off.data(), v->sizes = m->sizes.data(), v->slots = m->slots.data();
  return LINS_OK;
}
int local_map_slots(lins_ctx* ctx) { return local_of(ctx)->n_slots; }
int local_map_ring(lins_ctx* ctx, int slot, int* window) {
  LocalMap* m = local_of(ctx);
  if (slot < 0 || slot >= m->n_slots) return -1;
  if (window) *window = m->window;
  return m->count[slot];
}
// (lifecycle.h) the rings of the slots named as lins_local_map_init leaves them; the last build's clouds stay
int local_map_release_apply(lins_ctx* ctx, int n, const int32_t* slots) {
  LocalMap* m = local_of(ctx);
  for (int k = 0; k < n; ++k) {
    const int s = slots[k];
    m->head[s] = m->count[s] = 0;
    std::fill(m->meta.begin() + (size_t)s * m->window, m->meta.begin() + (size_t)(s + 1) * m->window, KeyFrame{});
  }
  return LINS_OK;
}

// ---- snapshot.h: the ring in age order, oldest first.  A build reads the ring's frames by age alone ((head + i) %
// window, i = 0 .. count - 1, above), so a ring restored with head = 0 gives the bits of the ring it was taken from.
void local_map_snapshot_context(lins_ctx* ctx, SnapContext& c) {
  LocalMap* m = local_of(ctx);
  if (!m->n_slots) return;
  c.modules |= LINS_SNAP_RING, c.facts.ring_window = m->window;
  c.base[LINS_SNAP_BUF_RING] = m->d_frames.get(), c.units[LINS_SNAP_BUF_RING] = (int64_t)m->n_slots * m->window * m->max_pts;
}

int local_map_snapshot_describe(lins_ctx* ctx, int slot, SnapStream& s) {
  LocalMap* m = local_of(ctx);
  s.modules |= LINS_SNAP_RING;
  const int cnt = m->count[slot];
  s.counts.ring_frames = cnt, s.counts.ring_points = 0;
  lins_snapshot_frame* fr = s.host_section<lins_snapshot_frame>(LINS_SNAP_SEC_RING_META, (size_t)cnt);
  s.ring_off.resize(cnt), s.ring_n.resize(cnt);
  for (int i = 0; i < cnt; ++i) {
    const int idx = (m->head[slot] + i) % m->window;
    const KeyFrame& kf = m->meta[(size_t)slot * m->window + idx];
    std::memcpy(fr[i].n, kf.n, sizeof kf.n);
    const float pose[6] = {kf.pose.x, kf.pose.y, kf.pose.z, kf.pose.roll, kf.pose.pitch, kf.pose.yaw};
    std::memcpy(fr[i].pose, pose, sizeof pose);
    std::memcpy(fr[i].t, kf.t, sizeof kf.t);
    s.ring_off[i] = ((int64_t)slot * m->window + idx) * m->max_pts, s.ring_n[i] = kf.n[0] + kf.n[1] + kf.n[2];
    s.counts.ring_points += s.ring_n[i];
  }
  return LINS_OK;
}

int local_map_restore_check(lins_ctx* ctx, int slot, lins_snapshot_limits& lim) {
  LocalMap* m = local_of(ctx);
  if (m->head[slot] || m->count[slot]) return LINS_E_STATE;
  lim.ring_window = m->window, lim.ring_max_pts = m->max_pts;
  return LINS_OK;
}

void local_map_restore_place(lins_ctx* ctx, int slot, const SnapView& v, SnapStream& s) {
  LocalMap* m = local_of(ctx);
  const int cnt = v.info.counts.ring_frames;
  s.ring_off.resize(cnt), s.ring_n.resize(cnt);
  for (int i = 0; i < cnt; ++i) {
    lins_snapshot_frame f;
    std::memcpy(&f, v.sec(LINS_SNAP_SEC_RING_META) + (size_t)i * sizeof f, sizeof f);
    s.ring_off[i] = ((int64_t)slot * m->window + i) * m->max_pts, s.ring_n[i] = f.n[0] + f.n[1] + f.n[2];
  }
}

void local_map_restore_apply(lins_ctx* ctx, int slot, const SnapView& v) {
  LocalMap* m = local_of(ctx);
  const int cnt = v.info.counts.ring_frames;
  m->head[slot] = 0, m->count[slot] = cnt;
  for (int i = 0; i < cnt; ++i) {
    lins_snapshot_frame f;
    std::memcpy(&f, v.sec(LINS_SNAP_SEC_RING_META) + (size_t)i * sizeof f, sizeof f);
    KeyFrame& kf = m->meta[(size_t)slot * m->window + i];
    std::memcpy(kf.n, f.n, sizeof kf.n);
    kf.pose = lins_key_pose{f.pose[0], f.pose[1], f.pose[2], f.pose[3], f.pose[4], f.pose[5]};
    std::memcpy(kf.t, f.t, sizeof kf.t);
  }
}
}  // namespace lins

extern "C" {

int lins_local_map_release_slot(lins_ctx* ctx, int slot) {
  if (!ctx) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  const int32_t s = slot;
  if (int rc = release_list_check(1, &s, m->n_slots)) return rc;
  if (int rc = ctx_quiesce(ctx)) return rc;  // (a push_scans copy may still read the ring)
  return local_map_release_apply(ctx, 1, &s);
}

int lins_local_map_init(lins_ctx* ctx, int n_slots, int window, int max_points_per_frame) {
  if (!ctx || n_slots < 1 || window < 1 || window > 4096 || max_points_per_frame < 1) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  LocalMap* m = local_of(ctx);
  HIP_TRY(ctx, hipStreamSynchronize(ctx_stream(ctx)));  // (a push_scans copy may still read the old rings)
  m->d_frames.reset();
  m->n_slots = 0, m->built = false;
  BUF_TRY(ctx, m->d_frames.grow((size_t)n_slots * window * max_points_per_frame));
  m->n_slots = n_slots, m->window = window, m->max_pts = max_points_per_frame;
  m->meta.assign((size_t)n_slots * window, KeyFrame{});
  m->head.assign(n_slots, 0), m->count.assign(n_slots, 0);
  return LINS_OK;
}

int lins_local_map_push(lins_ctx* ctx, int slot, const lins_keyframe* f) {
  if (!ctx || !f) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots) return LINS_E_ARG;
  const lins_point* c[3] = {f->corner, f->surf, f->outlier};
  const int n[3] = {f->n_corner, f->n_surf, f->n_outlier};
  for (int k = 0; k < 3; ++k)
    if (int rc = cloud_check(c[k], n[k])) return rc;
  if (!pose_ok(f->pose)) return LINS_E_INPUT;
  if ((long long)n[0] + n[1] + n[2] > m->max_pts) return LINS_E_CAPACITY;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  const int idx = ring_push(m, slot);
  KeyFrame& kf = m->meta[(size_t)slot * m->window + idx];
  float4* dst = frame_ptr(m, slot, idx);
  for (int k = 0; k < 3; ++k) {
    kf.n[k] = n[k];
    if (n[k]) HIP_TRY(ctx, hipMemcpyAsync(dst, c[k], (size_t)n[k] * sizeof(float4), hipMemcpyHostToDevice, st));
    dst += n[k];
  }
  set_pose(kf, f->pose);
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (the caller's clouds may go once this returns)
  return LINS_OK;
}

// The build behind lins_local_map_build (scans: the entries' scan clouds on the host — checked, boxed and packed here,
// one upload) and lins_local_map_build_streams (from: the same clouds where they lie in the streams' arenas — one
// kernel does that work); arguments checked by the caller.  Everything else is the same job table and the same launches.
// msrc: where the two map jobs of an entry read their frames.  Jobs are named by their logical index (stage A: 5 k + cloud,
// stage B: 5 n + k) and stored at ph[logical]: the map jobs of more than the archive's chunk of tiles come first, so that
// one stage launcher splits their scans (launch_lm_stage_split); a ring build has none and ph is the identity.
static int local_map_build_impl(lins_ctx* ctx, LocalMap* m, int n, const int32_t* slots, const lins_local_scan* scans,
                                const StreamMapClouds* from, const MapSource& msrc, lins_local_map_sizes* out) {
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  m->built = false;
  auto scan_n = [&](int k, int q) { return from ? from[k].n[q] : (q == 0 ? scans[k].n_corner : q == 1 ? scans[k].n_surf : scans[k].n_outlier); };
  const int NJ = 6 * n;  // jobs: stage A 5 per entry (5k + cloud), stage B one per entry (5n + k)
  std::vector<LmJob> jobs(NJ);
  std::vector<LmState> states(NJ);
  std::vector<long long> cap(NJ, 0);
  std::vector<int> frames_of(n);
  for (int k = 0; k < n; ++k) {
    const int s = slots[k];
    frames_of[k] = msrc.ids ? msrc.n_ids[k] : m->count[s];
    for (int i = 0; i < frames_of[k]; ++i) {
      const int* fn = msrc.ids ? msrc.frame(k, s, i).n : m->meta[(size_t)s * m->window + (m->head[s] + i) % m->window].n;
      cap[5 * k] += fn[0], cap[5 * k + 1] += (long long)fn[1] + fn[2];
    }
    cap[5 * k + 2] = scan_n(k, 0), cap[5 * k + 3] = scan_n(k, 1), cap[5 * k + 4] = scan_n(k, 2);
    cap[5 * n + k] = (long long)scan_n(k, 1) + scan_n(k, 2);
  }
  for (int j = 0; j < NJ; ++j)
    if (cap[j] > INT_MAX / 2) return LINS_E_CAPACITY;
  std::vector<int> ph(NJ, -1), lg;  // logical -> stored index and back
  const int chunk = msrc.ids ? msrc.ar.chunk : INT_MAX;
  for (int k = 0; k < n && msrc.ids; ++k)
    for (int w = 0; w < 2; ++w)
      if ((cap[5 * k + w] + kLmTile - 1) / kLmTile > chunk) ph[5 * k + w] = (int)lg.size(), lg.push_back(5 * k + w);
  const int n_split = (int)lg.size();
  for (int j = 0; j < NJ; ++j)
    if (ph[j] < 0) ph[j] = (int)lg.size(), lg.push_back(j);
  // staging: the raw scans of all entries first (one upload), then the maps, then stage B
  std::vector<int> order;
  for (int k = 0; k < n; ++k)
    for (int c = 2; c < 5; ++c) order.push_back(5 * k + c);
  size_t raw_total = 0;
  for (int j : order) raw_total += (size_t)cap[j];
  for (int k = 0; k < n; ++k) order.push_back(5 * k), order.push_back(5 * k + 1);
  for (int k = 0; k < n; ++k) order.push_back(5 * n + k);
  size_t stage_total = 0, tiles_total = 0, out_total = 0;
  for (int j : order) jobs[ph[j]].off_in = (long long)stage_total, stage_total += (size_t)cap[j];
  for (int j = 0; j < NJ; ++j) {
    LmJob& jb = jobs[j];
    jb.cap = (int)cap[lg[j]];
    jb.ntiles = (int)((cap[lg[j]] + kLmTile - 1) / kLmTile);
    jb.tile0 = (int)tiles_total, tiles_total += (size_t)jb.ntiles;
    jb.out_after = jb.src_a = jb.src_b = jb.feed = jb.feed_after = -1, jb.map = 0, jb.pad = 0;
    LmState& st = states[j];
    std::memset(&st, 0, sizeof st);
    for (int a = 0; a < 3; ++a)
      st.mn[a] = lm_enc(INFINITY), st.mx[a] = lm_enc(-INFINITY), st.bmin[a] = INT_MAX, st.bmax[a] = INT_MIN;
    st.n = j < 5 * n ? jb.cap : 0;
  }
  if (tiles_total > (size_t)INT_MAX / 256) return LINS_E_CAPACITY;
  std::vector<ArChunk> chunks;  // the split jobs' chunk tables, as lins_archive_assemble builds them
  std::vector<ArSplit> splits;
  for (int j = 0; j < n_split; ++j) {
    ArSplit sp{j, (int)chunks.size(), (jobs[j].ntiles + chunk - 1) / chunk, 0};
    for (int c = 0; c < sp.nc; ++c) chunks.push_back(ArChunk{j, c, sp.c0, 0});
    splits.push_back(sp);
  }
  for (int k = 0; k < n; ++k) {
    const long long c2 = cap[5 * k + 2] + cap[5 * n + k];  // cornerDS, then surfTotalDS right behind it (the query layout)
    const long long ocap[5] = {cap[5 * k], cap[5 * k + 1], c2, cap[5 * k + 3], cap[5 * k + 4]};
    for (int c = 0; c < 5; ++c) {
      LmJob& jb = jobs[ph[5 * k + c]];
      jb.off_out = (long long)out_total, out_total += (size_t)ocap[c];
      jb.inv = 1.0f / (c == 0 || c == 2 ? 0.2f : 0.4f);
    }
    jobs[ph[5 * k]].map = jobs[ph[5 * k + 1]].map = 1;
    LmJob& b = jobs[ph[5 * n + k]];
    b.inv = 1.0f / 0.4f;
    b.off_out = jobs[ph[5 * k + 2]].off_out, b.out_after = ph[5 * k + 2];
    b.src_a = ph[5 * k + 3], b.src_b = ph[5 * k + 4];
    jobs[ph[5 * k + 3]].feed = jobs[ph[5 * k + 4]].feed = ph[5 * n + k];
    jobs[ph[5 * k + 4]].feed_after = ph[5 * k + 3];
  }
  int rc;
  if (scans) BUF_TRY(ctx, m->h_raw.grow(raw_total));
  // raw scans: input contract, f32 box (the min / max the device would fold), packed for one upload
  for (int k = 0; k < n && scans; ++k) {
    const lins_point* c[3] = {scans[k].corner, scans[k].surf, scans[k].outlier};
    const int cn[3] = {scans[k].n_corner, scans[k].n_surf, scans[k].n_outlier};
    for (int q = 0; q < 3; ++q) {
      if ((rc = cloud_check(c[q], cn[q]))) return rc;
      const int j = ph[5 * k + 2 + q];
      float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (int i = 0; i < cn[q]; ++i) {
        const lins_point& p = c[q][i];
        mn[0] = std::min(mn[0], p.x), mn[1] = std::min(mn[1], p.y), mn[2] = std::min(mn[2], p.z);
        mx[0] = std::max(mx[0], p.x), mx[1] = std::max(mx[1], p.y), mx[2] = std::max(mx[2], p.z);
      }
      for (int a = 0; a < 3; ++a) states[j].mn[a] = lm_enc(mn[a]), states[j].mx[a] = lm_enc(mx[a]);
      if (cn[q]) std::memcpy(m->h_raw + jobs[j].off_in, c[q], (size_t)cn[q] * sizeof(float4));
    }
  }
  // ... or staged on the device out of the streams' arenas: one segment per (entry, cloud), blocks of kLmTile points
  std::vector<LmScanSeg> ssegs;
  std::vector<int2> sblocks;
  for (int k = 0; k < n && from; ++k)
    for (int q = 0; q < 3; ++q) {
      const int cnt = from[k].n[q], j = ph[5 * k + 2 + q];
      if (!cnt) continue;
      for (int b = 0; b < (cnt + kLmTile - 1) / kLmTile; ++b) sblocks.push_back(make_int2((int)ssegs.size(), b));
      ssegs.push_back(LmScanSeg{from[k].src[q], jobs[j].off_in, cnt, j});
    }
  // the window's clouds: one segment per (frame, cloud), blocks of kLmTile points
  std::vector<LmSeg> segs;
  std::vector<int2> blocks;
  uint64_t pts_in = raw_total;
  for (int k = 0; k < n; ++k) {
    const int s = slots[k];
    long long at[2] = {jobs[ph[5 * k]].off_in, jobs[ph[5 * k + 1]].off_in};
    // ... or the listed archive frames': corner_i -> corner map; surf_i and outlier_i, one behind the other in the arena
    // and under one pose, -> surf map as one segment (LM:1310-1314)
    for (int i = 0; i < frames_of[k] && msrc.ids; ++i) {
      const ArFrame& f = msrc.frame(k, s, i);
      const long long from_off[2] = {f.off, f.off + f.n[0]};
      const int cnt[2] = {f.n[0], f.n[1] + f.n[2]};
      for (int w = 0; w < 2; ++w) {
        if (cnt[w]) {
          LmSeg g{};
          g.src = from_off[w], g.dst = at[w], g.n = cnt[w], g.job = ph[5 * k + w];
          std::memcpy(g.t, f.t, sizeof g.t);
          for (int b = 0; b < (cnt[w] + kLmTile - 1) / kLmTile; ++b) blocks.push_back(make_int2((int)segs.size(), b));
          segs.push_back(g);
        }
        at[w] += cnt[w], pts_in += (uint64_t)cnt[w];
      }
    }
    for (int i = 0; i < m->count[s] && !msrc.ids; ++i) {
      const int idx = (m->head[s] + i) % m->window;
      const KeyFrame& f = m->meta[(size_t)s * m->window + idx];
      long long src = (long long)(frame_ptr(m, s, idx) - m->d_frames);
      for (int q = 0; q < 3; ++q) {  // LM:1242-1246: corner_i -> corner map; surf_i, outlier_i -> surf map
        const int w = q == 0 ? 0 : 1;
        if (f.n[q]) {
          LmSeg g{};
          g.src = src, g.dst = at[w], g.n = f.n[q], g.job = ph[5 * k + w];
          std::memcpy(g.t, f.t, sizeof g.t);
          for (int b = 0; b < (f.n[q] + kLmTile - 1) / kLmTile; ++b) blocks.push_back(make_int2((int)segs.size(), b));
          segs.push_back(g);
        }
        src += f.n[q], at[w] += f.n[q], pts_in += (uint64_t)f.n[q];
      }
    }
  }
  std::vector<int2> tiles;
  tiles.reserve(tiles_total);
  for (int j = 0; j < NJ; ++j)
    for (int t = 0; t < jobs[j].ntiles; ++t) tiles.push_back(make_int2(j, t));
  const int tiles_a = n ? jobs[5 * n].tile0 : 0;  // stage A's tiles come first (stage B's jobs are stored where they are named)
  const int tiles_b = (int)tiles_total - tiles_a;
  // one table upload: jobs | states | segments | blocks | tiles | scan segments | scan blocks | chunks | splits
  const size_t o_jobs = 0, o_states = align64(o_jobs + NJ * sizeof(LmJob)), o_segs = align64(o_states + NJ * sizeof(LmState)),
               o_blocks = align64(o_segs + segs.size() * sizeof(LmSeg)), o_tiles = align64(o_blocks + blocks.size() * sizeof(int2)),
               o_ssegs = align64(o_tiles + tiles.size() * sizeof(int2)), o_sblocks = align64(o_ssegs + ssegs.size() * sizeof(LmScanSeg)),
               o_chunks = align64(o_sblocks + sblocks.size() * sizeof(int2)), o_splits = align64(o_chunks + chunks.size() * sizeof(ArChunk)),
               tab_bytes = align64(o_splits + splits.size() * sizeof(ArSplit));
  BUF_TRY(ctx, m->h_tab.grow(tab_bytes));
  BUF_TRY(ctx, m->h_states.grow(NJ * sizeof(LmState)));
  std::memcpy(m->h_tab + o_jobs, jobs.data(), NJ * sizeof(LmJob));
  std::memcpy(m->h_tab + o_states, states.data(), NJ * sizeof(LmState));
  if (!segs.empty()) std::memcpy(m->h_tab + o_segs, segs.data(), segs.size() * sizeof(LmSeg));
  if (!blocks.empty()) std::memcpy(m->h_tab + o_blocks, blocks.data(), blocks.size() * sizeof(int2));
  if (!tiles.empty()) std::memcpy(m->h_tab + o_tiles, tiles.data(), tiles.size() * sizeof(int2));
  if (!ssegs.empty()) std::memcpy(m->h_tab + o_ssegs, ssegs.data(), ssegs.size() * sizeof(LmScanSeg));
  if (!sblocks.empty()) std::memcpy(m->h_tab + o_sblocks, sblocks.data(), sblocks.size() * sizeof(int2));
  if (!chunks.empty()) std::memcpy(m->h_tab + o_chunks, chunks.data(), chunks.size() * sizeof(ArChunk));
  if (!splits.empty()) std::memcpy(m->h_tab + o_splits, splits.data(), splits.size() * sizeof(ArSplit));
  if (from) BUF_TRY(ctx, m->ev_stage.create());
  BUF_TRY(ctx, m->d_tab.grow(tab_bytes));
  // the staging arena and the sort's scratch: same extent
  BUF_TRY(ctx, grow_all(m->d_stage, stage_total, m->d_ka, stage_total, m->d_kb, stage_total, m->d_va, stage_total, m->d_vb, stage_total, m->d_starts, stage_total));
  BUF_TRY(ctx, grow_all(m->d_hist, tiles_total * 256, m->d_tilecnt, tiles_total));
  BUF_TRY(ctx, m->d_out.grow(out_total));
  if (!chunks.empty()) BUF_TRY(ctx, m->d_csum.grow(chunks.size()));
  hipStream_t st = ctx_stream(ctx);
  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  if (raw_total && scans) HIP_TRY(ctx, hipMemcpyAsync(m->d_stage, m->h_raw, raw_total * sizeof(float4), hipMemcpyHostToDevice, st));
  if (tab_bytes) HIP_TRY(ctx, hipMemcpyAsync(m->d_tab, m->h_tab, tab_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(e0, st));
  const LmJob* d_jobs = (const LmJob*)(m->d_tab + o_jobs);
  LmState* d_states = (LmState*)(m->d_tab + o_states);
  const int2* d_tiles = (const int2*)(m->d_tab + o_tiles);
  if (from) {
    launch_lm_stage_scans(st, (int)sblocks.size(), (const LmScanSeg*)(m->d_tab + o_ssegs), (const int2*)(m->d_tab + o_sblocks), m->d_stage, d_states);
    HIP_TRY(ctx, hipEventRecord(m->ev_stage, st));
  }
  if (msrc.ids)
    launch_ar_gather(st, (int)blocks.size(), (const LmSeg*)(m->d_tab + o_segs), (const int2*)(m->d_tab + o_blocks), msrc.ar.d_arena, m->d_stage, d_states);
  else
    launch_lm_transform(st, (int)blocks.size(), (const LmSeg*)(m->d_tab + o_segs), (const int2*)(m->d_tab + o_blocks), m->d_frames, m->d_stage, d_states);
  launch_lm_stage_split(st, 0, n_split, 5 * n, tiles_a, d_tiles, d_jobs, d_states, m->d_stage, m->d_ka, m->d_kb, m->d_va, m->d_vb, m->d_hist,
                        m->d_tilecnt, m->d_starts, m->d_out, chunk, (int)chunks.size(), (const ArChunk*)(m->d_tab + o_chunks),
                        (const ArSplit*)(m->d_tab + o_splits), m->d_csum);
  launch_lm_stage(st, 5 * n, n, tiles_b, d_tiles + tiles_a, d_jobs, d_states, m->d_stage, m->d_ka, m->d_kb, m->d_va, m->d_vb,
                  m->d_hist, m->d_tilecnt, m->d_starts, m->d_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(e1, st));
  if (NJ) HIP_TRY(ctx, hipMemcpyAsync(m->h_states, d_states, NJ * sizeof(LmState), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&m->ms, e0, e1));
  m->stage_ms = 0.f;
  if (from) HIP_TRY(ctx, hipEventElapsedTime(&m->stage_ms, e0, m->ev_stage));
  m->points_in = pts_in;
  const LmState* S = (const LmState*)m->h_states.get();
  m->slots.assign(slots, slots + n);
  m->off.assign((size_t)6 * n, 0);
  m->sizes.assign(n, lins_local_map_sizes{});
  for (int k = 0; k < n; ++k) {
    lins_local_map_sizes& z = m->sizes[k];
    const int js[6] = {ph[5 * k], ph[5 * k + 1], ph[5 * k + 2], ph[5 * k + 3], ph[5 * k + 4], ph[5 * n + k]};
    int status = LINS_OK;
    for (int j : js)
      if (S[j].status == LINS_E_INPUT || (S[j].status && !status)) status = S[j].status;
    z.status = status, z.frames = frames_of[k];
    for (int c = 0; c < 6; ++c) {
      z.n[c] = status ? 0 : S[js[c]].nvox;
      m->off[6 * k + c] = c < 5 ? jobs[js[c]].off_out : jobs[js[2]].off_out + S[js[2]].nvox;
    }
    for (int w = 0; w < 2; ++w)
      for (int a = 0; a < 3; ++a) {
        const bool any = z.n[w] > 0;
        z.box_min[w][a] = any ? S[js[w]].bmin[a] : 0;
        z.box_dim[w][a] = any ? S[js[w]].bmax[a] - S[js[w]].bmin[a] + 1 : 1;
      }
    if (out) out[k] = z;
  }
  m->built = true;
  return LINS_OK;
}

int lins_local_map_build(lins_ctx* ctx, int n, const int32_t* slots, const lins_local_scan* scans, lins_local_map_sizes* out) {
  if (!ctx || n < 0 || (n && (!slots || !scans))) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  for (int k = 0; k < n; ++k) {
    if (slots[k] < 0 || slots[k] >= m->n_slots) return LINS_E_ARG;
    const lins_local_scan& s = scans[k];
    if (s.n_corner < 0 || s.n_surf < 0 || s.n_outlier < 0 || (s.n_corner && !s.corner) || (s.n_surf && !s.surf) ||
        (s.n_outlier && !s.outlier))
      return LINS_E_ARG;
  }
  static const lins_local_scan none{};
  return local_map_build_impl(ctx, m, n, slots, n ? scans : &none, nullptr, MapSource{}, out);
}

int lins_local_map_build_streams(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* streams, lins_local_map_sizes* out) {
  if (!ctx || n < 0 || (n && (!slots || !streams))) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  std::vector<StreamMapClouds> from((size_t)std::max(n, 1));
  for (int k = 0; k < n; ++k) {
    if (slots[k] < 0 || slots[k] >= m->n_slots) return LINS_E_ARG;
    for (int i = 0; i < k; ++i)
      if (streams[i] == streams[k]) return LINS_E_ARG;  // (a stream may appear once)
  }
  for (int k = 0; k < n; ++k)
    if (int rc = streams_map_clouds(ctx, streams[k], &from[k])) return rc;
  return local_map_build_impl(ctx, m, n, slots, nullptr, from.data(), MapSource{}, out);
}

// the surround builds' own arguments: both stores there, every slot in both, every id a frame of its slot
static int surround_source(lins_ctx* ctx, LocalMap* m, int n, const int32_t* slots, const int32_t* const* ids, const int32_t* n_ids, MapSource* src) {
  if (!m->n_slots) return LINS_E_STATE;
  if (int rc = archive_store(ctx, &src->ar)) return rc;
  for (int k = 0; k < n; ++k) {
    if (slots[k] < 0 || slots[k] >= m->n_slots || slots[k] >= src->ar.n_slots || n_ids[k] < 0 || (n_ids[k] && !ids[k])) return LINS_E_ARG;
    const int have = (int)(*src->ar.frames)[slots[k]].size();
    for (int i = 0; i < n_ids[k]; ++i)
      if (ids[k][i] < 0 || ids[k][i] >= have) return LINS_E_ARG;
  }
  src->ids = ids, src->n_ids = n_ids;
  return LINS_OK;
}

int lins_local_map_build_surround(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* const* ids, const int32_t* n_ids,
                                  const lins_local_scan* scans, lins_local_map_sizes* out) {
  if (!ctx || n < 0 || (n && (!slots || !ids || !n_ids || !scans))) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  MapSource src;
  if (int rc = surround_source(ctx, m, n, slots, ids, n_ids, &src)) return rc;
  for (int k = 0; k < n; ++k) {
    const lins_local_scan& s = scans[k];
    if (s.n_corner < 0 || s.n_surf < 0 || s.n_outlier < 0 || (s.n_corner && !s.corner) || (s.n_surf && !s.surf) ||
        (s.n_outlier && !s.outlier))
      return LINS_E_ARG;
  }
  static const lins_local_scan none{};
  return local_map_build_impl(ctx, m, n, slots, n ? scans : &none, nullptr, src, out);
}

int lins_local_map_build_surround_streams(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* const* ids, const int32_t* n_ids,
                                          const int32_t* streams, lins_local_map_sizes* out) {
  if (!ctx || n < 0 || (n && (!slots || !ids || !n_ids || !streams))) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  MapSource src;
  if (int rc = surround_source(ctx, m, n, slots, ids, n_ids, &src)) return rc;
  std::vector<StreamMapClouds> from((size_t)std::max(n, 1));
  for (int k = 0; k < n; ++k)
    for (int i = 0; i < k; ++i)
      if (streams[i] == streams[k]) return LINS_E_ARG;  // (a stream may appear once)
  for (int k = 0; k < n; ++k)
    if (int rc = streams_map_clouds(ctx, streams[k], &from[k])) return rc;
  return local_map_build_impl(ctx, m, n, slots, nullptr, from.data(), src, out);
}

// the team builds' own arguments: as surround_source, each list entry naming its own archive slot
static int team_source(lins_ctx* ctx, LocalMap* m, int n, const int32_t* slots, const int32_t* const* pairs, const int32_t* n_pairs, MapSource* src) {
  if (!m->n_slots) return LINS_E_STATE;
  if (int rc = archive_store(ctx, &src->ar)) return rc;
  for (int k = 0; k < n; ++k) {
    if (slots[k] < 0 || slots[k] >= m->n_slots || slots[k] >= src->ar.n_slots || n_pairs[k] < 0 || (n_pairs[k] && !pairs[k])) return LINS_E_ARG;
    for (int i = 0; i < n_pairs[k]; ++i) {
      const int32_t slot = pairs[k][2 * i], id = pairs[k][2 * i + 1];
      if (slot < 0 || slot >= src->ar.n_slots || id < 0 || id >= (int)(*src->ar.frames)[slot].size()) return LINS_E_ARG;
    }
  }
  src->ids = pairs, src->n_ids = n_pairs, src->pairs = true;
  return LINS_OK;
}

int lins_local_map_build_team(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* const* pairs, const int32_t* n_pairs,
                              const lins_local_scan* scans, lins_local_map_sizes* out) {
  if (!ctx || n < 0 || (n && (!slots || !pairs || !n_pairs || !scans))) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  MapSource src;
  if (int rc = team_source(ctx, m, n, slots, pairs, n_pairs, &src)) return rc;
  for (int k = 0; k < n; ++k) {
    const lins_local_scan& s = scans[k];
    if (s.n_corner < 0 || s.n_surf < 0 || s.n_outlier < 0 || (s.n_corner && !s.corner) || (s.n_surf && !s.surf) ||
        (s.n_outlier && !s.outlier))
      return LINS_E_ARG;
  }
  static const lins_local_scan none{};
  return local_map_build_impl(ctx, m, n, slots, n ? scans : &none, nullptr, src, out);
}

int lins_local_map_build_team_streams(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* const* pairs, const int32_t* n_pairs,
                                      const int32_t* streams, lins_local_map_sizes* out) {
  if (!ctx || n < 0 || (n && (!slots || !pairs || !n_pairs || !streams))) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  MapSource src;
  if (int rc = team_source(ctx, m, n, slots, pairs, n_pairs, &src)) return rc;
  std::vector<StreamMapClouds> from((size_t)std::max(n, 1));
  for (int k = 0; k < n; ++k)
    for (int i = 0; i < k; ++i)
      if (streams[i] == streams[k]) return LINS_E_ARG;  // (a stream may appear once)
  for (int k = 0; k < n; ++k)
    if (int rc = streams_map_clouds(ctx, streams[k], &from[k])) return rc;
  return local_map_build_impl(ctx, m, n, slots, nullptr, from.data(), src, out);
}

int lins_last_local_map_stage_ms(lins_ctx* ctx, float* stage_ms) {
  if (!ctx || !stage_ms) return LINS_E_ARG;
  *stage_ms = local_of(ctx)->stage_ms;
  return LINS_OK;
}

int lins_local_map_push_scans(lins_ctx* ctx, int n, const int32_t* entries, const lins_key_pose* poses) {
  if (!ctx || n < 0 || (n && (!entries || !poses))) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  if (!m->built) return LINS_E_STATE;
  for (int i = 0; i < n; ++i) {
    const int e = entries[i];
    if (e < 0 || e >= (int)m->slots.size()) return LINS_E_ARG;
    const lins_local_map_sizes& z = m->sizes[e];
    if (z.status) return LINS_E_STATE;
    if (!pose_ok(poses[i])) return LINS_E_INPUT;
    if ((long long)z.n[LINS_LOCAL_SCAN_CORNER] + z.n[LINS_LOCAL_SCAN_SURF] + z.n[LINS_LOCAL_SCAN_OUTLIER] > m->max_pts)
      return LINS_E_CAPACITY;
  }
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  for (int i = 0; i < n; ++i) {  // saveKeyFramesAndFactor (LM:1758-1763): cornerDS, surfDS, outlierDS
    const int e = entries[i], s = m->slots[e];
    const int idx = ring_push(m, s);
    KeyFrame& kf = m->meta[(size_t)s * m->window + idx];
    float4* dst = frame_ptr(m, s, idx);
    for (int q = 0; q < 3; ++q) {
      const int c = LINS_LOCAL_SCAN_CORNER + q, cnt = m->sizes[e].n[c];
      kf.n[q] = cnt;
      if (cnt) HIP_TRY(ctx, hipMemcpyAsync(dst, m->d_out + m->off[6 * e + c], (size_t)cnt * sizeof(float4), hipMemcpyDeviceToDevice, st));
      dst += cnt;
    }
    set_pose(kf, poses[i]);
  }
  return LINS_OK;
}

int lins_local_map_set_pose(lins_ctx* ctx, int slot, int age, const lins_key_pose* pose) {
  if (!ctx || !pose) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot < 0 || slot >= m->n_slots || age < 0 || age >= m->count[slot]) return LINS_E_ARG;
  if (!pose_ok(*pose)) return LINS_E_INPUT;
  const int idx = (m->head[slot] + m->count[slot] - 1 - age) % m->window;
  set_pose(m->meta[(size_t)slot * m->window + idx], *pose);
  return LINS_OK;
}

int lins_local_map_download(lins_ctx* ctx, int entry, int which, lins_point* out, int cap) {
  if (!ctx) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  if (!m->built) return LINS_E_STATE;
  if (entry < 0 || entry >= (int)m->slots.size() || which < 0 || which > 5) return LINS_E_ARG;
  const int cnt = m->sizes[entry].n[which];
  if (cnt > cap) return LINS_E_CAPACITY;
  if (cnt && !out) return LINS_E_ARG;
  if (!cnt) return 0;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(out, m->d_out + m->off[6 * entry + which], (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return cnt;
}

int lins_last_local_map_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* points_in) {
  if (!ctx) return LINS_E_ARG;
  LocalMap* m = local_of(ctx);
  if (kernel_ms) *kernel_ms = m->ms;
  if (points_in) *points_in = m->points_in;
  return LINS_OK;
}

}  // extern "C"
