// lins_loop_step_capi.hip — C ABI of the loop thread's step (include/lins_map.h lins_loop_step, lins_loop_closed_cloud):
// performLoopClosure + correctPoses (LM:1033-1186, 1767-1795) for n slots in one call.  Host orchestration only: every
// device stage is the batched call that already exists — lins_archive_assemble, lins_loop_icp_batch_from,
// lins_pose_graph_solve, lins_pose_graph_apply_batch — run ONCE over the entries that reach it, so an entry's bits are
// those of the explicit chain for its slot; what is decided between the stages is host/loop_step.h, the text
// liblins_host.so exports.  lins_loop_step and lins_loop_step_place are one function (step): the front end detects by
// pose or by appearance, the assemble-and-align stage in the middle is the one the rendezvous steps share
// (loop_verify.h, laid out by host/verify_plan.h), the back end is close_loops.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lins_map.h"
#include "../../include/lins_streams_map.h"
#include "host/keyframe_select.h"
#include "../../include/lins_place.h"
#include "host/loop_step.h"
#include "host/place_guess.h"
#include "keyframe_archive.h"
#include "lins_ctx_priv.h"
#include "local_map.h"
#include "loop_icp_math.h"
#include "loop_verify.h"
#include "place.h"
#include "pose_graph.h"

using namespace lins;

namespace {

struct Aligned {  // one entry of the last step
  int source = -1;  // its source cloud in the step's assembly (-1: the entry was not aligned)
  double T[16];
};

struct LoopStepMem {
  std::vector<Aligned> last;
  unsigned long long serial = 0;  // the assembly the sources are entries of
  float assemble_ms = 0.f, icp_ms = 0.f, solve_ms = 0.f;
  int candidates = 0, aligned = 0, closed = 0;
};

void loop_step_free(void* p) { delete (LoopStepMem*)p; }

LoopStepMem* mem_of(lins_ctx* ctx) {
  void** slot = map_slot(ctx, kSlotLoopStep, loop_step_free);
  if (!*slot) *slot = new LoopStepMem();
  return (LoopStepMem*)*slot;
}

// the ranges of the calls the parameters are handed to: lins_archive_find_loop, lins_archive_assemble,
// lins_loop_icp_batch_from, lins_pose_graph_solve
bool params_ok(const lins_loop_step_params* p) {
  return lins_verify::params_ok(p) && std::isfinite(p->search_radius) && p->search_radius >= 0.f && lins_pg::params_ok(&p->graph);
}

// entry k's step record: lins_loop_step's results are an array of them, lins_loop_step_place's begin with one
lins_loop_step_result& step_at(void* out, size_t stride, int k) { return *(lins_loop_step_result*)((char*)out + (size_t)k * stride); }

// The whole call's errors of both entry points, before anything is queued; fills slots, streams and (read_centre) centre.
int check_call(lins_ctx* ctx, int n, const lins_loop_step_entry* entries, const lins_loop_step_params* prm, bool read_centre,
               std::vector<int32_t>& slots, std::vector<int32_t>& streams, std::vector<float>& centre) {
  slots.assign(n, 0), streams.assign(n, 0), centre.assign(3 * (size_t)n, 0.f);
  for (int k = 0; k < n; ++k) {
    const lins_loop_step_entry& e = entries[k];
    const int in_archive = lins_archive_count(ctx, e.slot);
    if (in_archive < 0 || e.slot >= pose_graph_slots(ctx) || in_archive != lins_pose_graph_count(ctx, e.slot, nullptr)) return LINS_E_ARG;
    if (e.stream < -1 || e.stream >= streams_map_streams(ctx) || (e.flags & ~LINS_LOOP_CENTRE_STREAM)) return LINS_E_ARG;
    if ((e.flags & LINS_LOOP_CENTRE_STREAM) && e.stream < 0) return LINS_E_ARG;
    for (int i = 0; i < k; ++i)
      if (entries[i].slot == e.slot || (e.stream >= 0 && entries[i].stream == e.stream)) return LINS_E_ARG;
    slots[k] = e.slot, streams[k] = e.stream;
  }
  for (int k = 0; k < n; ++k) {
    const lins_loop_step_entry& e = entries[k];
    if (!read_centre) {
      if (!std::isfinite(e.now)) return LINS_E_INPUT;
      continue;
    }
    if (e.flags & LINS_LOOP_CENTRE_STREAM) {
      if (int rc = streams_map_centre(ctx, e.stream, &centre[3 * (size_t)k])) return rc;  // LINS_E_STATE: has not stepped
    } else {
      std::memcpy(&centre[3 * (size_t)k], e.centre, 3 * sizeof(float));
    }
    if (!lins_select::query_ok(&centre[3 * (size_t)k], prm->search_radius) || !std::isfinite(e.now)) return LINS_E_INPUT;
  }
  std::vector<int32_t> with_frames_slots, with_frames_streams;  // the write-back's refusals (a slot without frames closes nothing)
  for (int k = 0; k < n; ++k)
    if (lins_archive_count(ctx, slots[k]) > 0) with_frames_slots.push_back(slots[k]), with_frames_streams.push_back(streams[k]);
  return pose_graph_apply_check(ctx, (int)with_frames_slots.size(), with_frames_slots.data(), with_frames_streams.data());
}

// lins_archive_find_loop's answer per entry (-1: none, or a slot without frames); LINS_KEYPOSES_DEVICE: the entries that
// have frames in one lins_keyposes_find_loop_batch
int pose_detect(lins_ctx* ctx, int n, const lins_loop_step_entry* entries, const lins_loop_step_params* prm, const std::vector<int32_t>& slots,
                const std::vector<float>& centre, std::vector<int32_t>& closest) {
  closest.assign(n, -1);
  if (lins_keyposes_mode(ctx) == LINS_KEYPOSES_DEVICE) {
    std::vector<int> at;
    std::vector<lins_keyposes_loop_query> qs;
    for (int k = 0; k < n; ++k) {
      if (lins_archive_count(ctx, slots[k]) < 1) continue;
      const float* c = &centre[3 * (size_t)k];
      at.push_back(k);
      qs.push_back(lins_keyposes_loop_query{lins_keyposes_query{slots[k], {c[0], c[1], c[2]}, prm->search_radius, 0.f}, entries[k].now, prm->min_gap_s});
    }
    std::vector<int32_t> found(qs.size(), -1);
    if (int rc = lins_keyposes_find_loop_batch(ctx, (int)qs.size(), qs.data(), found.data())) return rc;
    for (size_t i = 0; i < at.size(); ++i) closest[at[i]] = found[i];
    return LINS_OK;
  }
  for (int k = 0; k < n; ++k) {
    if (lins_archive_count(ctx, slots[k]) < 1) continue;
    if (int rc = lins_archive_find_loop(ctx, slots[k], &centre[3 * (size_t)k], prm->search_radius, entries[k].now, prm->min_gap_s, &closest[k])) return rc;
  }
  return LINS_OK;
}

// The tail both entry points share (LM:1140-1181, 1767-1795).  `judged`: the entries whose step record holds an alignment
// (icp, closest_id) and the outcome LINS_LOOP_REJECTED.  The factor of every accepted one, then the solve and the
// correction of the history, one call each over the slots that gained a loop.
int close_loops(lins_ctx* ctx, LoopStepMem* m, const lins_loop_step_params* prm, const std::vector<int32_t>& slots, const std::vector<int32_t>& streams,
                const std::vector<int>& judged, void* out, size_t stride) {
  std::vector<int> closed;  // entries
  for (int k : judged) {
    lins_loop_step_result& r = step_at(out, stride, k);
    if (!lins_loop::accept(r.icp.converged, r.icp.fitness, prm->max_fitness) || !lins_loop::variance(r.icp.fitness, nullptr)) continue;
    lins_key_pose wrong;
    if (int rc = lins_pose_graph_poses(ctx, slots[k], r.latest_id, 1, &wrong)) return rc;
    lins_loop::pose_from(r.icp.transform, wrong, &r.pose_from);
    if (int rc = lins_pose_graph_add_loop(ctx, slots[k], r.latest_id, r.closest_id, &r.pose_from, r.icp.fitness)) {
      r.status = rc;  // (a pose_from that is not finite)
      continue;
    }
    closed.push_back(k);
  }
  const int ns = (int)closed.size();
  if (ns == 0) return LINS_OK;
  std::vector<int32_t> s_slots(ns), s_streams(ns);
  std::vector<lins_pose_graph_result> solved(ns);
  for (int i = 0; i < ns; ++i) s_slots[i] = slots[closed[i]], s_streams[i] = streams[closed[i]];
  if (int rc = lins_pose_graph_solve(ctx, ns, s_slots.data(), &prm->graph, solved.data())) return rc;
  (void)lins_last_pose_graph_stats(ctx, &m->solve_ms, nullptr);
  for (int i = 0; i < ns; ++i) step_at(out, stride, closed[i]).graph = solved[i];
  if (int rc = lins_pose_graph_apply_batch(ctx, ns, s_slots.data(), s_streams.data())) return rc;
  for (int i = 0; i < ns; ++i) step_at(out, stride, closed[i]).outcome = LINS_LOOP_CLOSED;
  m->closed = ns;
  return LINS_OK;
}

// Both entry points, arguments and parameters checked: check -> detect -> plan -> verify_assemble -> start transforms ->
// verify_align -> choose -> close_loops.  `out`: records `stride` bytes apart that begin with a step record (step_at).
// place == nullptr: lins_loop_step — the records are step records, every entry is detected by pose (one hypothesis) and
// the place store `ap` is not read; else they are lins_loop_place_result.
int step(lins_ctx* ctx, int n, const lins_loop_step_entry* entries, const lins_loop_step_params* prm, const lins_loop_place_params* place,
         const ArchivePlace* ap, void* out, size_t stride) {
  lins_loop_place_result* po = place ? (lins_loop_place_result*)out : nullptr;
  const bool pose_first = !place || place->mode == LINS_LOOP_DETECT_POSE_THEN_PLACE;
  const int K = place ? place->k : 1, min_sep = !place ? 0 : place->min_sep < 0 ? prm->search_num : place->min_sep;
  // ---- the whole call's errors, before anything is queued ----
  std::vector<int32_t> slots, streams, closest(n, -1);
  std::vector<float> centre;
  if (int rc = check_call(ctx, n, entries, prm, pose_first, slots, streams, centre)) return rc;
  if (place && (long long)n * (1 + K) > 2147483647ll) return LINS_E_CAPACITY;  // (specs of one assembly; the n K alignments are fewer)

  LoopStepMem* m = mem_of(ctx);
  m->last.assign(n, Aligned());
  m->assemble_ms = m->icp_ms = m->solve_ms = 0.f, m->candidates = m->aligned = m->closed = 0;
  // ---- detect: the pose search where the mode asks for it, then one top-K search over the entries it left empty-handed ----
  if (pose_first)
    if (int rc = pose_detect(ctx, n, entries, prm, slots, centre, closest)) return rc;
  std::vector<int> asking;  // entries of the place search
  std::vector<lins_place_query> qs;
  for (int k = 0; k < n; ++k) {
    lins_loop_step_result& r = step_at(out, stride, k);
    std::memset((void*)&r, 0, stride);
    r.outcome = LINS_LOOP_NONE, r.latest_id = lins_archive_count(ctx, slots[k]) - 1, r.closest_id = -1;
    if (!po) continue;
    po[k].chosen = -1;
    for (int j = 0; j < LINS_PLACE_MAX_K; ++j) po[k].cand[j].id = -1, po[k].cand[j].distance = 1.f;
    if (r.latest_id < 0 || closest[k] >= 0) continue;  // (detect 0: lins_loop_step's entry)
    po[k].detect = 1;
    asking.push_back(k);
    qs.push_back(lins_place_query{slots[k], r.latest_id, slots[k], 0, entries[k].now, prm->min_gap_s});
  }
  std::vector<lins_place_result> found(qs.size() * (size_t)K);
  std::vector<int32_t> filled(qs.size(), 0);
  if (!qs.empty())
    if (int rc = lins_place_topk_batch(ctx, (int)qs.size(), qs.data(), K, min_sep, found.data(), filled.data())) return rc;
  std::vector<int> at_query(n, -1);
  for (size_t i = 0; i < asking.size(); ++i) at_query[asking[i]] = (int)i;
  // ---- plan: per candidate entry the latest frame against one history window per rank ----
  Verify v;
  for (int k = 0; k < n; ++k) {
    lins_loop_step_result& r = step_at(out, stride, k);
    if (r.latest_id < 0) continue;
    int loops_left = 0, last_latest = -1, last_closest = -1, what = LINS_LOOP_NONE, nc = 0;
    int32_t ids[LINS_PLACE_MAX_K];  // the frames that go to the alignment
    pose_graph_room(ctx, slots[k], nullptr, &loops_left, &last_latest, &last_closest);
    if (!po || !po[k].detect) {
      r.closest_id = closest[k];
      what = lins_loop::candidate(r.latest_id, r.closest_id, last_latest, last_closest);
      if (what == lins_loop::kAlign) ids[nc++] = r.closest_id;
      if (po && nc) po[k].cand[0].id = r.closest_id;
    } else {
      const lins_place_result* f = &found[(size_t)at_query[k] * K];
      for (int j = 0; j < filled[at_query[k]]; ++j) {
        if (f[j].distance > place->max_distance) continue;
        const int w = lins_loop::candidate(r.latest_id, f[j].id, last_latest, last_closest);
        if (w == LINS_LOOP_REPEAT) what = LINS_LOOP_REPEAT;
        if (w == lins_loop::kAlign) po[k].cand[nc] = f[j], ids[nc++] = f[j].id;
      }
      if (nc) what = lins_loop::kAlign;
    }
    if (what != lins_loop::kAlign) {
      r.outcome = what;
    } else if (loops_left < 1) {
      r.status = LINS_E_CAPACITY;
      for (int j = 0; po && j < LINS_PLACE_MAX_K; ++j) po[k].cand[j] = lins_place_result{-1, 0, 1.f, 0, 0, 0};
    } else {
      if (po) po[k].n_candidates = nc;
      v.entry(k, slots[k]);
      for (int j = 0; j < nc; ++j) v.hyp(r.latest_id, slots[k], ids[j], r.latest_id);
    }
  }
  m->candidates = v.n();
  if (v.n() == 0) return LINS_OK;
  // ---- assemble ----
  if (int rc = verify_assemble(ctx, v, prm->search_num, prm->history_leaf)) return rc;
  (void)lins_last_archive_stats(ctx, &m->assemble_ms, nullptr);
  ArchiveView av{};
  if (int rc = archive_view(ctx, &av)) return rc;
  m->serial = av.serial;
  // ---- start transforms: the appearance's guess, or the identity (lins_loop_icp_batch's start) ----
  std::vector<double> T0(16 * v.hyps.size(), 0.0);
  for (int i = 0; i < v.n(); ++i) {
    const int k = v.of[i], x0 = v.hyp0[i];
    const bool detect = po && po[k].detect;
    lins_loop_step_result& r = step_at(out, stride, k);
    r.latest = v.infos[v.src_spec[x0]];
    if (!detect) r.history = v.infos[v.tgt_spec[x0]];
    if (v.status[i]) {  // (nothing is aligned for it)
      r.status = v.status[i];
      continue;
    }
    for (int x = x0; x < v.hyp0[i + 1]; ++x) {
      double* T = &T0[16 * (size_t)x];
      if (detect) {
        const std::vector<ArFrame>& fr = (*ap->frames)[slots[k]];
        const lins_place_result& c = po[k].cand[x - x0];
        lins_place::guess(fr[r.latest_id].pose, fr[c.id].pose, c.shift, ap->store->prm.up_axis, T);
      } else {
        T[0] = T[5] = T[10] = T[15] = 1.0;
      }
    }
  }
  // ---- align ----
  if (int rc = verify_align(ctx, v, T0.data(), &prm->icp)) return rc;
  if (!v.n_ran) return LINS_OK;
  (void)lins_last_loop_icp_stats(ctx, &m->icp_ms, nullptr);
  // ---- choose: the best accepted fit of every entry goes on to the tail ----
  std::vector<int> judged;  // entries
  for (int i = 0; i < v.n(); ++i) {
    if (v.status[i]) continue;
    const int k = v.of[i], x0 = v.hyp0[i], nc = v.hyp0[i + 1] - x0;
    const bool detect = po && po[k].detect;
    const lins_loop_icp_result* icp = &v.icp[x0];
    lins_loop_step_result& r = step_at(out, stride, k);
    int32_t conv[LINS_PLACE_MAX_K];
    double fit[LINS_PLACE_MAX_K];
    if (po) std::memcpy(po[k].icp, icp, nc * sizeof icp[0]);
    const lins_verify::IcpSummary s = lins_verify::icp_summary(icp, nc, conv, fit);
    if (!detect) r.icp = icp[0];
    if (!s.ran) {
      r.status = s.status;
      continue;
    }
    m->aligned += 1;
    r.outcome = LINS_LOOP_REJECTED;
    const int chosen = lins_loop::choose(nc, conv, fit, prm->max_fitness);
    if (po) po[k].chosen = chosen;
    if (detect) {
      if (chosen < 0) continue;
      r.closest_id = po[k].cand[chosen].id, r.history = v.infos[v.tgt_spec[x0 + chosen]], r.icp = icp[chosen];
    }
    m->last[k].source = v.src_spec[x0];
    std::memcpy(m->last[k].T, r.icp.transform, sizeof r.icp.transform);
    judged.push_back(k);
  }
  return close_loops(ctx, m, prm, slots, streams, judged, out, stride);
}

}  // namespace

extern "C" {

void lins_loop_step_default_params(lins_loop_step_params* p) {
  if (!p) return;
  p->search_radius = 5.f, p->max_fitness = 0.3f, p->history_leaf = 0.4f, p->search_num = 25, p->min_gap_s = 30.0;
  lins_licp::default_params(&p->icp);
  lins_pg::default_params(&p->graph);
}

int lins_loop_step(lins_ctx* ctx, int n, const lins_loop_step_entry* entries, const lins_loop_step_params* prm, lins_loop_step_result* out) {
  if (!ctx || n < 0 || (n && (!entries || !out))) return LINS_E_ARG;
  if (lins_archive_count(ctx, 0) == LINS_E_STATE || !pose_graph_slots(ctx)) return LINS_E_STATE;
  if (!params_ok(prm)) return LINS_E_ARG;
  return step(ctx, n, entries, prm, nullptr, nullptr, out, sizeof *out);
}

void lins_loop_place_default_params(lins_loop_place_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->mode = LINS_LOOP_DETECT_PLACE, p->k = 4, p->min_sep = -1, p->max_distance = 1.f;
}

// (include/lins_place.h) lins_loop_step with the candidates found by appearance: every stage is ONE batched call
int lins_loop_step_place(lins_ctx* ctx, int n, const lins_loop_step_entry* entries, const lins_loop_step_params* prm,
                         const lins_loop_place_params* place, lins_loop_place_result* out) {
  if (!ctx || n < 0 || (n && (!entries || !out))) return LINS_E_ARG;
  if (lins_archive_count(ctx, 0) == LINS_E_STATE || !pose_graph_slots(ctx)) return LINS_E_STATE;
  ArchivePlace ap;
  if (archive_place(ctx, &ap) || !ap.store->on) return LINS_E_STATE;
  if (!params_ok(prm) || !place) return LINS_E_ARG;
  if ((place->mode != LINS_LOOP_DETECT_PLACE && place->mode != LINS_LOOP_DETECT_POSE_THEN_PLACE) || place->k < 1 || place->k > LINS_PLACE_MAX_K ||
      place->min_sep < -1 || std::isnan(place->max_distance))
    return LINS_E_ARG;
  return step(ctx, n, entries, prm, place, &ap, out, sizeof *out);
}

int lins_loop_closed_cloud(lins_ctx* ctx, int entry, lins_point* out, int cap) {
  if (!ctx) return LINS_E_ARG;
  LoopStepMem* m = mem_of(ctx);
  if (entry < 0 || entry >= (int)m->last.size() || m->last[entry].source < 0) return LINS_E_ARG;
  ArchiveView av{};
  if (int rc = archive_view(ctx, &av)) return rc;
  if (av.serial != m->serial || m->last[entry].source >= av.n) return LINS_E_STATE;  // (another assembly since the step)
  const int cnt = lins_archive_download(ctx, m->last[entry].source, out, cap);
  if (cnt <= 0) return cnt;
  float M[12];
  lins_licp::make_move(m->last[entry].T, M);
  for (int i = 0; i < cnt; ++i) {  // step 1 of the ICP's contract at the final T; intensity stays
    float x, y, z;
    lins_licp::move_point(M, out[i].x, out[i].y, out[i].z, x, y, z);
    out[i].x = x, out[i].y = y, out[i].z = z;
  }
  return cnt;
}

int lins_last_loop_step_stats(lins_ctx* ctx, float* assemble_ms, float* icp_ms, float* solve_ms, int32_t* candidates, int32_t* aligned,
                              int32_t* closed) {
  if (!ctx) return LINS_E_ARG;
  LoopStepMem* m = mem_of(ctx);
  if (assemble_ms) *assemble_ms = m->assemble_ms;
  if (icp_ms) *icp_ms = m->icp_ms;
  if (solve_ms) *solve_ms = m->solve_ms;
  if (candidates) *candidates = m->candidates;
  if (aligned) *aligned = m->aligned;
  if (closed) *closed = m->closed;
  return LINS_OK;
}

}  // extern "C"
