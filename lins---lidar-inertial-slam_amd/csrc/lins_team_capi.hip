// lins_team_capi.hip — C ABI of the team search (include/lins_team.h): host orchestration around team_kernels.hip.
// The ring keys live in the place store (place.h TeamStore), allocated by the first call here.  A call has the stale
// frames of every slot it names described by lins_place_sync, then packs ONE table — the frames without a key | the
// queries | the targets —, uploads it, queues the key launch, the shortlist launches and the pair launch, downloads the
// n * M shortlist keys and the n * M row keys and synchronises once; select_team takes the ranks here.  The marks "keyed
// below id" move only after that synchronisation.
// lins_rendezvous_step is host orchestration only, as lins_loop_step_place is: every device stage is a batched call that
// exists, run ONCE over the entries that reach it.  lins_rendezvous_window_step is the same composition over the last
// frames of every entry, with one more stage: lins_rendezvous_consensus_batch (rendezvous_consensus_kernels.hip; its
// staging is place.h ConsensusStore) decides which alignments agree.  The two share their checks (rendezvous_check,
// assembly_room) and, with the loop thread's steps, the assemble-and-align stage in the middle (loop_verify.h, laid out
// by host/verify_plan.h); each keeps its own detect filter and its own decision.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lins_team.h"
#include "host/loop_step.h"
#include "host/place_guess.h"
#include "host/place_math.h"
#include "host/rendezvous_consensus.h"
#include "keyframe_archive.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "local_map.h"
#include "loop_verify.h"
#include "place.h"

using namespace lins;
using namespace lins_place;

namespace {

size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// the store, switched on, of an archive whose slots a shortlist key holds
int store_of(lins_ctx* ctx, ArchivePlace* A) {
  if (int rc = archive_place(ctx, A)) return rc;
  if (!A->store->on) return LINS_E_STATE;
  return A->n_slots > kMaxTeamSlots ? LINS_E_CAPACITY : LINS_OK;
}

// the mirror, sized for the archive (the first call after lins_place_init allocates it)
int keys_ready(lins_ctx* ctx, const ArchivePlace& A) {
  TeamStore& t = A.store->team;
  if (!t.keyed.empty()) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  BUF_TRY(ctx, t.d_key.grow((size_t)A.n_slots * A.max_frames * 2));
  t.keyed.assign(A.n_slots, 0);
  return LINS_OK;
}

// Describes and keys the stale frames of `slots` and of the queries' slots, then answers the n queries.  Arguments
// checked by the caller.
int run(lins_ctx* ctx, const ArchivePlace& A, int n, const lins_place_team_query* qs, int n_targets, const int32_t* slots,
        const lins_place_team_params& prm, lins_place_team_result* results, int32_t* counts) {
  TeamStore& t = A.store->team;
  t.key_ms = t.shortlist_ms = t.pair_ms = 0.f, t.scanned = 0, t.built = 0;
  const std::vector<std::vector<ArFrame>>& frames = *A.frames;
  std::vector<int32_t> named(slots, slots + n_targets);
  for (int k = 0; k < n; ++k) named.push_back(qs[k].query_slot);
  std::vector<int> mark = t.keyed.empty() ? std::vector<int>((size_t)A.n_slots, 0) : t.keyed;  // as they will stand after this call
  std::vector<TmStale> stale;
  for (int32_t s : named) {
    const std::vector<ArFrame>& fr = frames[s];
    for (int i = mark[s]; i < (int)fr.size(); ++i) stale.push_back(TmStale{(long long)s * A.max_frames + i, fr[i].time});
    mark[s] = (int)fr.size();  // (a slot named again in this call adds nothing)
  }
  if (stale.size() > (size_t)INT_MAX) return LINS_E_CAPACITY;
  std::vector<TmTarget> targets((size_t)n_targets);
  long long total = 0;
  for (int k = 0; k < n_targets; ++k) {
    targets[k] = TmTarget{(long long)slots[k] * A.max_frames, total, slots[k], (int)frames[slots[k]].size()};
    total += targets[k].nf;
  }
  const int M = prm.shortlist, chunk = t.chunk;
  const long long n_chunks = (total + chunk - 1) / chunk;
  if ((long long)n * n_chunks > INT_MAX || n_chunks * M > INT_MAX) return LINS_E_CAPACITY;
  if (stale.empty() && n == 0) return LINS_OK;
  // (every refusal is behind us: from here on only a HIP error ends the call)
  if (int rc = lins_place_sync(ctx, (int)named.size(), named.data())) return rc;
  if (int rc = keys_ready(ctx, A)) return rc;
  std::vector<TmQuery> queries((size_t)n);
  for (int k = 0; k < n; ++k)
    queries[k] = TmQuery{(long long)qs[k].query_slot * A.max_frames + qs[k].query_id, qs[k].now, qs[k].min_gap_s, qs[k].query_slot, qs[k].query_id};
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  // up: stale | queries | targets.  down: the shortlists | the rows, and behind them (never downloaded) the chunks' lists
  const size_t o_queries = align64(stale.size() * sizeof(TmStale)), o_targets = align64(o_queries + (size_t)n * sizeof(TmQuery)),
               up_bytes = align64(o_targets + (size_t)n_targets * sizeof(TmTarget));
  const size_t o_row = align64((size_t)n * M * 8), o_lists = align64(o_row + (size_t)n * M * 8), down_bytes = o_lists,
               down_cap = align64(o_lists + (size_t)n * (size_t)n_chunks * M * 8);
  BUF_TRY(ctx, t.h_up.grow(up_bytes));
  BUF_TRY(ctx, t.d_up.grow(up_bytes));
  BUF_TRY(ctx, t.h_down.grow(down_bytes));
  BUF_TRY(ctx, t.d_down.grow(down_cap));
  for (int i = 0; i < 4; ++i) BUF_TRY(ctx, t.ev[i].create());
  if (!stale.empty()) std::memcpy(t.h_up, stale.data(), stale.size() * sizeof(TmStale));
  if (n) std::memcpy(t.h_up + o_queries, queries.data(), (size_t)n * sizeof(TmQuery));
  if (n_targets) std::memcpy(t.h_up + o_targets, targets.data(), (size_t)n_targets * sizeof(TmTarget));
  hipStream_t st = ctx_stream(ctx);
  const TmQuery* d_queries = (const TmQuery*)(t.d_up + o_queries);
  unsigned long long* d_short = (unsigned long long*)t.d_down.get();
  unsigned long long* d_row = (unsigned long long*)(t.d_down + o_row);
  HIP_TRY(ctx, hipMemcpyAsync(t.d_up, t.h_up, up_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(t.ev[0], st));
  launch_team_keys(st, (int)stale.size(), (const TmStale*)t.d_up.get(), A.store->d_D, t.d_key);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(t.ev[1], st));
  launch_team_shortlist(st, n, d_queries, n_targets, (const TmTarget*)(t.d_up + o_targets), total, chunk, (int)n_chunks, M, t.d_key,
                        (unsigned long long*)(t.d_down + o_lists), d_short);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(t.ev[2], st));
  launch_team_pairs(st, n, d_queries, M, A.max_frames, d_short, A.store->d_rec, d_row);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(t.ev[3], st));
  if (n) HIP_TRY(ctx, hipMemcpyAsync(t.h_down, t.d_down, down_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&t.key_ms, t.ev[0], t.ev[1]));
  HIP_TRY(ctx, hipEventElapsedTime(&t.shortlist_ms, t.ev[1], t.ev[2]));
  HIP_TRY(ctx, hipEventElapsedTime(&t.pair_ms, t.ev[2], t.ev[3]));
  t.keyed = mark;
  t.built = (int)stale.size(), t.scanned = (uint64_t)n * (uint64_t)total;
  const unsigned long long* S = (const unsigned long long*)t.h_down.get();
  const unsigned long long* R = (const unsigned long long*)(t.h_down + o_row);
  for (int k = 0; k < n; ++k) {
    // admissible candidates: every frame of another slot; of the query's own, those the gate admits
    long long admissible = 0;
    for (int j = 0; j < n_targets; ++j) {
      const std::vector<ArFrame>& fr = frames[slots[j]];
      if (slots[j] != qs[k].query_slot) {
        admissible += (long long)fr.size();
        continue;
      }
      for (int c = 0; c < (int)fr.size(); ++c)
        if (team_admits(slots[j], c, fr[c].time, qs[k].query_slot, qs[k].query_id, qs[k].now, qs[k].min_gap_s)) admissible += 1;
    }
    int pos[kMaxK];
    const int filled = select_team(R + (size_t)k * M, S + (size_t)k * M, M, prm.k, prm.min_sep, pos);
    team_results(R + (size_t)k * M, S + (size_t)k * M, pos, prm.k, (int)(admissible > INT_MAX ? INT_MAX : admissible), results + (size_t)k * prm.k);
    counts[k] = filled;
  }
  return LINS_OK;
}

int slots_check(const ArchivePlace& A, int n_targets, const int32_t* slots) {
  if (n_targets < 0 || (n_targets && !slots)) return LINS_E_ARG;
  std::vector<char> seen((size_t)A.n_slots, 0);
  for (int k = 0; k < n_targets; ++k) {
    if (slots[k] < 0 || slots[k] >= A.n_slots || seen[slots[k]]) return LINS_E_ARG;
    seen[slots[k]] = 1;
  }
  return LINS_OK;
}

// ---- what the two rendezvous steps share in front of their detect stages ----
// The whole call's errors, before anything is queued; *tp: the team search's parameters, min_sep resolved.
int rendezvous_check(const ArchivePlace& A, int n, const lins_rendezvous_entry* entries, int n_targets, const int32_t* target_slots,
                     const lins_loop_step_params* prm, const lins_rendezvous_params* team, lins_place_team_params* tp) {
  if (!lins_verify::params_ok(prm) || !team) return LINS_E_ARG;
  *tp = team->team;
  if (tp->min_sep < -1 || std::isnan(team->max_distance)) return LINS_E_ARG;
  if (tp->min_sep < 0) tp->min_sep = prm->search_num;
  if (!team_params_ok(tp)) return LINS_E_ARG;
  if (int rc = slots_check(A, n_targets, target_slots)) return rc;
  for (int k = 0; k < n; ++k) {
    if (entries[k].slot < 0 || entries[k].slot >= A.n_slots) return LINS_E_ARG;
    for (int i = 0; i < k; ++i)
      if (entries[i].slot == entries[k].slot) return LINS_E_ARG;
  }
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(entries[k].now)) return LINS_E_INPUT;
  return LINS_OK;
}

// the frames of a slot with `count` frames that ask, of a window of W: latest - j * stride, while it exists
int queries_of(int count, int W, int stride) {
  int nq = 0;
  while (nq < W && (long long)(count - 1) - (long long)nq * stride >= 0) ++nq;
  return nq;
}

// What lins_archive_assemble refuses (a submap of more than INT_MAX / 2 points, more than INT_MAX / 256 tiles in a call),
// asked of the most the assembly can be given — the ranks are not known yet: K windows a query, every window as large as
// the largest target slot's whole history.  So the assembly behind the detect stage cannot refuse.  (lins_rendezvous_step:
// a window of one.)
int assembly_room(const std::vector<std::vector<ArFrame>>& frames, int n, const lins_rendezvous_entry* entries, int n_targets,
                  const int32_t* target_slots, int K, int W, int stride) {
  if ((long long)n * W * (1 + K) > 2147483647ll) return LINS_E_CAPACITY;
  auto both = [](const ArFrame& f) { return (long long)f.n[0] + f.n[1]; };  // corner | surf
  long long widest = 0, tiles = 0;
  for (int t = 0; t < n_targets; ++t) {
    long long sum = 0;
    for (const ArFrame& f : frames[target_slots[t]]) sum += both(f);
    widest = std::max(widest, sum);
  }
  if (widest > INT_MAX / 2) return LINS_E_CAPACITY;
  for (int k = 0; k < n; ++k) {
    const std::vector<ArFrame>& fr = frames[entries[k].slot];
    const int nq = queries_of((int)fr.size(), W, stride);
    for (int j = 0; j < nq; ++j)
      tiles += (both(fr[fr.size() - 1 - (size_t)j * stride]) + kLmTile - 1) / kLmTile + (long long)K * ((widest + kLmTile - 1) / kLmTile);
    if (tiles > INT_MAX / 256) return LINS_E_CAPACITY;
  }
  return LINS_OK;
}

// a result record before anything is known of its entry
template <class R>
R& blank(R& o) {
  std::memset(&o, 0, sizeof o);
  o.outcome = LINS_RENDEZVOUS_NONE, o.target_slot = o.target_id = -1;
  return o;
}

}  // namespace

extern "C" {

void lins_place_team_default_params(lins_place_team_params* p) {
  if (p) team_default_params(p);
}

int lins_place_team_topk_batch(lins_ctx* ctx, int n, const lins_place_team_query* queries, int n_targets, const int32_t* target_slots,
                               const lins_place_team_params* prm, lins_place_team_result* results, int32_t* counts) {
  if (!ctx || n < 0 || (n && (!queries || !results || !counts))) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  if (!team_params_ok(prm)) return LINS_E_ARG;
  if (int rc = slots_check(A, n_targets, target_slots)) return rc;
  for (int k = 0; k < n; ++k) {
    const lins_place_team_query& q = queries[k];
    if (q.query_slot < 0 || q.query_slot >= A.n_slots || q.query_id < 0 || q.query_id >= (int)(*A.frames)[q.query_slot].size()) return LINS_E_ARG;
  }
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(queries[k].now) || std::isnan(queries[k].min_gap_s)) return LINS_E_INPUT;
  return run(ctx, A, n, queries, n_targets, target_slots, *prm, results, counts);
}

int lins_place_team_key(lins_ctx* ctx, int slot, int id, uint8_t* occ, uint32_t* sumsq, double* time) {
  if (!ctx || !occ || !sumsq || !time) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  if (slot < 0 || slot >= A.n_slots || id < 0 || id >= (int)(*A.frames)[slot].size()) return LINS_E_ARG;
  const int32_t s = slot;
  lins_place_team_params prm;
  team_default_params(&prm);
  if (int rc = run(ctx, A, 0, nullptr, 1, &s, prm, nullptr, nullptr)) return rc;
  RingKey key;
  hipStream_t st = ctx_stream(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(&key, A.store->team.d_key + ((size_t)slot * A.max_frames + id) * 2, sizeof key, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  std::memcpy(occ, key.occ, sizeof key.occ);
  *sumsq = key.sumsq, *time = key.time;
  return LINS_OK;
}

int lins_place_team_set_chunk(lins_ctx* ctx, int chunk) {
  if (!ctx || chunk < 0) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = archive_place(ctx, &A)) return rc;
  A.store->team.chunk = chunk && chunk < kTmChunk ? chunk : kTmChunk;
  return LINS_OK;
}

int lins_last_place_team_stats(lins_ctx* ctx, float* key_ms, float* shortlist_ms, float* pair_ms, int32_t* frames_keyed, uint64_t* scanned) {
  if (!ctx) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = archive_place(ctx, &A)) return rc;
  const TeamStore& t = A.store->team;
  if (key_ms) *key_ms = t.key_ms;
  if (shortlist_ms) *shortlist_ms = t.shortlist_ms;
  if (pair_ms) *pair_ms = t.pair_ms;
  if (frames_keyed) *frames_keyed = t.built;
  if (scanned) *scanned = t.scanned;
  return LINS_OK;
}

void lins_rendezvous_default_params(lins_rendezvous_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  team_default_params(&p->team);
  p->team.min_sep = -1, p->max_distance = 1.f;
}

int lins_rendezvous_step(lins_ctx* ctx, int n, const lins_rendezvous_entry* entries, int n_targets, const int32_t* target_slots,
                         const lins_loop_step_params* prm, const lins_rendezvous_params* team, lins_rendezvous_result* out) {
  if (!ctx || n < 0 || (n && (!entries || !out))) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  // ---- the whole call's errors, before anything is queued ----
  lins_place_team_params tp;
  if (int rc = rendezvous_check(A, n, entries, n_targets, target_slots, prm, team, &tp)) return rc;
  const int K = tp.k;
  const std::vector<std::vector<ArFrame>>& frames = *A.frames;
  if (int rc = assembly_room(frames, n, entries, n_targets, target_slots, K, 1, 1)) return rc;
  // ---- detect: one team search over the entries that have a frame ----
  std::vector<int> asking;
  std::vector<lins_place_team_query> qs;
  for (int k = 0; k < n; ++k) {
    lins_rendezvous_result& o = blank(out[k]);
    o.latest_id = (int)frames[entries[k].slot].size() - 1, o.chosen = -1;
    for (int j = 0; j < LINS_PLACE_MAX_K; ++j) o.cand[j].slot = o.cand[j].id = o.cand[j].dk = -1, o.cand[j].distance = 1.f;
    if (o.latest_id < 0) continue;
    asking.push_back(k);
    qs.push_back(lins_place_team_query{entries[k].slot, o.latest_id, entries[k].now, prm->min_gap_s});
  }
  if (asking.empty()) return LINS_OK;
  std::vector<lins_place_team_result> found(qs.size() * (size_t)K);
  std::vector<int32_t> filled(qs.size(), 0);
  if (int rc = run(ctx, A, (int)qs.size(), qs.data(), n_targets, target_slots, tp, found.data(), filled.data())) return rc;
  // ---- plan: per entry its latest frame against one window per rank, from the rank's own slot ----
  Verify v;
  for (size_t a = 0; a < asking.size(); ++a) {
    lins_rendezvous_result& o = out[asking[a]];
    for (int j = 0; j < filled[a]; ++j)
      if (!(found[a * K + j].distance > team->max_distance)) o.cand[o.n_candidates++] = found[a * K + j];
    if (o.n_candidates) v.entry(asking[a], entries[asking[a]].slot);
    for (int j = 0; j < o.n_candidates; ++j) v.hyp(o.latest_id, o.cand[j].slot, o.cand[j].id, (int)frames[o.cand[j].slot].size() - 1);
  }
  if (v.n() == 0) return LINS_OK;
  // ---- assemble ----
  if (int rc = verify_assemble(ctx, v, prm->search_num, prm->history_leaf)) return rc;
  // ---- start transforms: the appearance's guess between the two maps ----
  std::vector<double> T0(16 * v.hyps.size(), 0.0);
  for (int i = 0; i < v.n(); ++i) {
    lins_rendezvous_result& o = out[v.of[i]];
    const int x0 = v.hyp0[i];
    o.latest = v.infos[v.src_spec[x0]];
    for (int j = 0; j < o.n_candidates; ++j) o.target[j] = v.infos[v.tgt_spec[x0 + j]];
    o.status = v.status[i];  // (not zero: nothing is aligned for it)
    for (int j = 0; j < o.n_candidates && !o.status; ++j)
      lins_place::guess_team(frames[v.slots[i]][o.latest_id].pose, frames[o.cand[j].slot][o.cand[j].id].pose, o.cand[j].shift, A.store->prm.up_axis,
                             &T0[16 * (size_t)(x0 + j)]);
  }
  // ---- align ----
  if (int rc = verify_align(ctx, v, T0.data(), &prm->icp)) return rc;
  if (!v.n_ran) return LINS_OK;
  // ---- choose ----
  for (int i = 0; i < v.n(); ++i) {
    if (v.status[i]) continue;
    lins_rendezvous_result& o = out[v.of[i]];
    int32_t conv[LINS_PLACE_MAX_K];
    double fit[LINS_PLACE_MAX_K];
    std::memcpy(o.icp, &v.icp[v.hyp0[i]], o.n_candidates * sizeof o.icp[0]);
    const lins_verify::IcpSummary s = lins_verify::icp_summary(o.icp, o.n_candidates, conv, fit);
    if (!s.ran) {
      o.status = s.status;
      continue;
    }
    o.outcome = LINS_RENDEZVOUS_REJECTED;
    o.chosen = lins_loop::choose(o.n_candidates, conv, fit, prm->max_fitness);
    if (o.chosen < 0) continue;
    o.outcome = LINS_RENDEZVOUS_FOUND, o.target_slot = o.cand[o.chosen].slot, o.target_id = o.cand[o.chosen].id;
    std::memcpy(o.X, o.icp[o.chosen].transform, sizeof o.X);
  }
  return LINS_OK;
}

// ---- rendezvous over a window ----
void lins_rendezvous_consensus_default_params(lins_consensus_params* p) {
  if (p) lins_consensus::default_params(p);
}

int lins_rendezvous_consensus_batch(lins_ctx* ctx, int n, const lins_consensus_hyp* hypotheses, const int32_t* offsets,
                                    const lins_consensus_params* prm, lins_consensus_result* results) {
  using namespace lins_consensus;
  if (!ctx || n < 0 || !bars_ok(prm) || (n && (!offsets || !results))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  if (offsets[0] != 0) return LINS_E_ARG;
  for (int e = 0; e < n; ++e)
    if (offsets[e + 1] < offsets[e] || offsets[e + 1] - offsets[e] > kMaxHyp) return LINS_E_ARG;
  const int total = offsets[n];
  if (total && !hypotheses) return LINS_E_ARG;
  int input = LINS_OK;  // (an argument error in any table comes before an input error in an earlier one)
  for (int e = 0; e < n; ++e) {
    const int rc = table_check(hypotheses + offsets[e], offsets[e + 1] - offsets[e]);
    if (rc == LINS_E_ARG) return rc;
    if (rc && !input) input = rc;
  }
  if (input) return input;
  // (every refusal is behind us)
  ConsensusStore& c = *archive_consensus(ctx);
  c.kernel_ms = 0.f;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  const size_t o_off = align64((size_t)total * sizeof(lins_consensus_hyp)), up_bytes = align64(o_off + ((size_t)n + 1) * sizeof(int32_t)),
               down_bytes = (size_t)n * sizeof(lins_consensus_result);
  BUF_TRY(ctx, c.h_up.grow(up_bytes));
  BUF_TRY(ctx, c.d_up.grow(up_bytes));
  BUF_TRY(ctx, c.h_down.grow(down_bytes));
  BUF_TRY(ctx, c.d_down.grow(down_bytes));
  for (int i = 0; i < 2; ++i) BUF_TRY(ctx, c.ev[i].create());
  if (total) std::memcpy(c.h_up, hypotheses, (size_t)total * sizeof(lins_consensus_hyp));
  std::memcpy(c.h_up + o_off, offsets, ((size_t)n + 1) * sizeof(int32_t));
  hipStream_t st = ctx_stream(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(c.d_up, c.h_up, up_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(c.ev[0], st));
  launch_rendezvous_consensus(st, n, (const lins_consensus_hyp*)c.d_up.get(), (const int*)(c.d_up + o_off), prm->max_translation,
                              prm->min_cos_rotation, (lins_consensus_result*)c.d_down.get());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(c.ev[1], st));
  HIP_TRY(ctx, hipMemcpyAsync(c.h_down, c.d_down, down_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&c.kernel_ms, c.ev[0], c.ev[1]));
  std::memcpy(results, c.h_down, down_bytes);
  return LINS_OK;
}

int lins_last_rendezvous_consensus_stats(lins_ctx* ctx, float* kernel_ms) {
  if (!ctx) return LINS_E_ARG;
  if (kernel_ms) *kernel_ms = archive_consensus(ctx)->kernel_ms;
  return LINS_OK;
}

int lins_last_rendezvous_window_stats(lins_ctx* ctx, float* detect_ms, float* assemble_ms, float* align_ms, float* consensus_ms, float* total_ms) {
  if (!ctx) return LINS_E_ARG;
  const float* t = archive_consensus(ctx)->stage_ms;
  float* const dst[5] = {detect_ms, assemble_ms, align_ms, consensus_ms, total_ms};
  for (int i = 0; i < 5; ++i)
    if (dst[i]) *dst[i] = t[i];
  return LINS_OK;
}

int lins_rendezvous_window_step(lins_ctx* ctx, int n, const lins_rendezvous_entry* entries, int n_targets, const int32_t* target_slots,
                                const lins_loop_step_params* prm, const lins_rendezvous_params* team, const lins_consensus_params* consensus,
                                lins_rendezvous_window_result* out, lins_rendezvous_hypothesis* hyp) {
  using clock = std::chrono::steady_clock;
  if (!ctx || n < 0 || (n && (!entries || !out || !hyp))) return LINS_E_ARG;
  ArchivePlace A;
  if (int rc = store_of(ctx, &A)) return rc;
  // ---- the whole call's errors, before anything is queued (the window's, and lins_rendezvous_step's) ----
  if (!lins_consensus::params_ok(consensus)) return LINS_E_ARG;
  lins_place_team_params tp;
  if (int rc = rendezvous_check(A, n, entries, n_targets, target_slots, prm, team, &tp)) return rc;
  const int K = tp.k, W = consensus->window, stride = consensus->stride;
  static_assert(LINS_RENDEZVOUS_MAX_WINDOW * LINS_PLACE_MAX_K == LINS_RENDEZVOUS_MAX_HYP, "an entry's hypotheses fill one consensus table at the most");
  const std::vector<std::vector<ArFrame>>& frames = *A.frames;
  if (int rc = assembly_room(frames, n, entries, n_targets, target_slots, K, W, stride)) return rc;
  ConsensusStore& cs = *archive_consensus(ctx);
  for (float& t : cs.stage_ms) t = 0.f;
  const clock::time_point t_begin = clock::now();
  clock::time_point t_stage = t_begin;
  auto lap = [&](int stage) {
    const clock::time_point now = clock::now();
    cs.stage_ms[stage] = std::chrono::duration<float, std::milli>(now - t_stage).count();
    cs.stage_ms[4] = std::chrono::duration<float, std::milli>(now - t_begin).count();
    t_stage = now;
  };
  // ---- queries and detect: one team search over every (entry, query) ----
  struct Ask {
    int entry, query;
  };
  std::vector<Ask> asks;
  std::vector<lins_place_team_query> qs;
  const size_t per_entry = (size_t)W * K;
  for (int k = 0; k < n; ++k) {
    lins_rendezvous_window_result& o = blank(out[k]);
    std::memset(hyp + k * per_entry, 0, per_entry * sizeof *hyp);
    o.winner = -1;
    const int count = (int)frames[entries[k].slot].size();
    o.n_queries = queries_of(count, W, stride);
    for (int j = 0; j < LINS_RENDEZVOUS_MAX_WINDOW; ++j) o.query_id[j] = j < o.n_queries ? count - 1 - j * stride : -1;
    for (int j = 0; j < o.n_queries; ++j) {
      asks.push_back(Ask{k, j});
      qs.push_back(lins_place_team_query{entries[k].slot, o.query_id[j], entries[k].now, prm->min_gap_s});
    }
  }
  if (asks.empty()) return LINS_OK;
  std::vector<lins_place_team_result> found(qs.size() * (size_t)K);
  std::vector<int32_t> filled(qs.size(), 0);
  if (int rc = run(ctx, A, (int)qs.size(), qs.data(), n_targets, target_slots, tp, found.data(), filled.data())) return rc;
  lap(0);
  for (size_t a = 0; a < asks.size(); ++a) {
    lins_rendezvous_window_result& o = out[asks[a].entry];
    lins_rendezvous_hypothesis* h = hyp + asks[a].entry * per_entry;
    for (int j = 0; j < filled[a]; ++j) {
      const lins_place_team_result& r = found[a * K + j];
      if (r.distance > team->max_distance || r.slot == entries[asks[a].entry].slot) continue;
      lins_rendezvous_hypothesis& x = h[o.n_hypotheses++];
      x.query = asks[a].query, x.rank = o.n_ranks[asks[a].query]++, x.cand = r;
    }
  }
  // ---- plan: per hypothesis its query's frame against the window around the rank, from the rank's own slot ----
  Verify v;
  for (int k = 0; k < n; ++k) {
    const lins_rendezvous_hypothesis* h = hyp + k * per_entry;
    if (out[k].n_hypotheses) v.entry(k, entries[k].slot);
    for (int x = 0; x < out[k].n_hypotheses; ++x)
      v.hyp(out[k].query_id[h[x].query], h[x].cand.slot, h[x].cand.id, (int)frames[h[x].cand.slot].size() - 1);
  }
  if (v.n() == 0) return LINS_OK;
  // ---- assemble ----
  if (int rc = verify_assemble(ctx, v, prm->search_num, prm->history_leaf)) return rc;
  lap(1);
  // ---- start transforms: the appearance's guess between the two maps ----
  std::vector<double> T0(16 * v.hyps.size(), 0.0);
  for (int i = 0; i < v.n(); ++i) {
    const int k = v.of[i];
    lins_rendezvous_window_result& o = out[k];
    lins_rendezvous_hypothesis* h = hyp + k * per_entry;
    for (int x = 0; x < o.n_hypotheses; ++x) {
      o.source[h[x].query] = v.infos[v.src_spec[v.hyp0[i] + x]];
      h[x].target = v.infos[v.tgt_spec[v.hyp0[i] + x]];
    }
    o.status = v.status[i];  // (not zero: nothing is aligned for it)
    for (int x = 0; x < o.n_hypotheses && !o.status; ++x)
      lins_place::guess_team(frames[entries[k].slot][o.query_id[h[x].query]].pose, frames[h[x].cand.slot][h[x].cand.id].pose, h[x].cand.shift,
                             A.store->prm.up_axis, &T0[16 * (size_t)(v.hyp0[i] + x)]);
  }
  // ---- align ----
  if (int rc = verify_align(ctx, v, T0.data(), &prm->icp)) return rc;
  if (!v.n_ran) return LINS_OK;
  lap(2);
  // ---- consensus: one table per entry that was aligned, one launch ----
  std::vector<int> judged;  // entries
  std::vector<lins_consensus_hyp> table;
  std::vector<int32_t> offsets(1, 0);
  for (int i = 0; i < v.n(); ++i) {
    if (v.status[i]) continue;
    const int k = v.of[i];
    lins_rendezvous_window_result& o = out[k];
    lins_rendezvous_hypothesis* h = hyp + k * per_entry;
    const lins_verify::IcpSummary s = lins_verify::icp_summary(&v.icp[v.hyp0[i]], o.n_hypotheses, nullptr, nullptr);
    for (int x = 0; x < o.n_hypotheses; ++x) {
      const lins_loop_icp_result& r = h[x].icp = v.icp[v.hyp0[i] + x];
      bool finite = lins_consensus::finite64(r.fitness) && r.fitness >= 0.0;
      for (int j = 0; j < 16; ++j) finite = finite && lins_consensus::finite64(r.transform[j]);
      h[x].admissible = !r.status && finite && lins_loop::accept(r.converged, r.fitness, prm->max_fitness) ? 1 : 0;
    }
    if (!s.ran) {
      o.status = s.status;
      continue;
    }
    judged.push_back(k);
    for (int x = 0; x < o.n_hypotheses; ++x) {
      lins_consensus_hyp c;
      std::memset(&c, 0, sizeof c);
      const lins_key_pose& p = frames[entries[k].slot][o.query_id[h[x].query]].pose;
      if (h[x].admissible) std::memcpy(c.X, h[x].icp.transform, sizeof c.X), c.fitness = h[x].icp.fitness;
      c.p[0] = (double)p.x, c.p[1] = (double)p.y, c.p[2] = (double)p.z;
      c.query = h[x].query, c.rank = h[x].rank, c.target_slot = h[x].cand.slot, c.admissible = h[x].admissible;
      table.push_back(c);
    }
    offsets.push_back((int32_t)table.size());
  }
  if (judged.empty()) return LINS_OK;
  std::vector<lins_consensus_result> verdict(judged.size());
  if (int rc = lins_rendezvous_consensus_batch(ctx, (int)judged.size(), table.data(), offsets.data(), consensus, verdict.data())) return rc;
  // ---- outcome ----
  for (size_t a = 0; a < judged.size(); ++a) {
    lins_rendezvous_window_result& o = out[judged[a]];
    lins_rendezvous_hypothesis* h = hyp + judged[a] * per_entry;
    const lins_consensus_result& w = verdict[a];
    o.winner = w.winner, o.support = w.support, o.n_admissible = w.n_admissible;
    std::memcpy(o.members, w.members, sizeof o.members);
    for (int x = 0; x < o.n_hypotheses; ++x) h[x].member = (int32_t)((w.members[x >> 5] >> (x & 31)) & 1u);
    o.outcome = w.winner < 0 ? LINS_RENDEZVOUS_REJECTED : (w.support < consensus->min_support ? LINS_RENDEZVOUS_UNCONFIRMED : LINS_RENDEZVOUS_FOUND);
    if (o.outcome != LINS_RENDEZVOUS_FOUND) continue;
    o.target_slot = h[w.winner].cand.slot, o.target_id = h[w.winner].cand.id;
    std::memcpy(o.X, h[w.winner].icp.transform, sizeof o.X);
  }
  lap(3);
  return LINS_OK;
}

}  // extern "C"
