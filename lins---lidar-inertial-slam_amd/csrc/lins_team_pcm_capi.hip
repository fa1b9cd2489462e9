// lins_team_pcm_capi.hip — C ABI of the pairwise-consistent team factors (include/lins_team.h
// lins_team_factors_consistent_batch): host orchestration around team_pcm_kernels.hip.  The groups are checked as
// lins_team_graph_solve checks them (the capacity apart: 64 factors a group), every factor becomes a record of
// host/team_pcm.h with the two frames' f64 estimates from the context's host graphs, and ONE table — the records | the
// offsets — is uploaded, answered by one launch and downloaded.  Nothing of the context but the staging (pose_graph_mem.h
// PcmWs) and the last launch's time is written.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/lins_team.h"
#include "host/team_pcm.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "pose_graph_mem.h"

using namespace lins;
using lins_pg::Graph;

namespace {

size_t align64(size_t x) { return (x + 63) & ~(size_t)63; }

// everything the call refuses, and the records of every group back to back
int pcm_check(const PgMem* m, int n_groups, const lins_team_member* members, const int32_t* moff, const lins_team_factor* factors,
              const int32_t* foff, std::vector<lins_pcm::Rec>& recs) {
  if (moff[0] != 0 || foff[0] != 0) return LINS_E_ARG;
  for (int g = 0; g < n_groups; ++g)
    if (moff[g + 1] <= moff[g] || foff[g + 1] < foff[g]) return LINS_E_ARG;  // (an empty group, as the solve)
  if (moff[n_groups] > m->n_slots) return LINS_E_ARG;                       // (some slot is named twice)
  if ((moff[n_groups] && !members) || (foff[n_groups] && !factors)) return LINS_E_ARG;
  std::vector<int> member_of(m->n_slots, -1), group_of(m->n_slots, -1);
  for (int g = 0; g < n_groups; ++g)
    for (int i = moff[g]; i < moff[g + 1]; ++i) {
      const int slot = members[i].slot;
      if (slot < 0 || slot >= m->n_slots || group_of[slot] >= 0 || m->g[slot].n_frames() == 0) return LINS_E_ARG;
      group_of[slot] = g, member_of[slot] = i - moff[g];
    }
  for (int g = 0; g < n_groups; ++g)
    for (int i = foff[g]; i < foff[g + 1]; ++i) {
      const lins_team_factor& f = factors[i];
      if (f.slot_b < 0 || f.slot_b >= m->n_slots || f.slot_a < 0 || f.slot_a >= m->n_slots) return LINS_E_ARG;
      if (group_of[f.slot_b] != g || group_of[f.slot_a] != g || f.slot_b == f.slot_a) return LINS_E_ARG;
      if (f.id_b < 0 || f.id_b >= m->g[f.slot_b].n_frames() || f.id_a < 0 || f.id_a >= m->g[f.slot_a].n_frames()) return LINS_E_ARG;
    }
  for (int i = 0; i < foff[n_groups]; ++i) {
    const lins_team_factor& f = factors[i];
    if (!lins_pg::team_z_ok(f.Z) || !lins_pg::team_var_ok(f.var)) return LINS_E_INPUT;
    if (!lins_pcm::finite12(&m->g[f.slot_b].T[12 * (size_t)f.id_b]) || !lins_pcm::finite12(&m->g[f.slot_a].T[12 * (size_t)f.id_a])) return LINS_E_INPUT;
  }
  for (int g = 0; g < n_groups; ++g)
    if (foff[g + 1] - foff[g] > lins_pcm::kMaxFactors || moff[g + 1] - moff[g] > LINS_TEAM_GRAPH_MAX_MEMBERS) return LINS_E_CAPACITY;
  recs.resize((size_t)foff[n_groups]);
  for (int i = 0; i < foff[n_groups]; ++i) {
    lins_team_factor f = factors[i];
    const double *Tb = &m->g[f.slot_b].T[12 * (size_t)f.id_b], *Ta = &m->g[f.slot_a].T[12 * (size_t)f.id_a];
    f.slot_b = member_of[f.slot_b], f.slot_a = member_of[f.slot_a];  // (the record's u < v are member indices, as the host call's)
    recs[i] = lins_pcm::record_of(f, Tb, Ta);
  }
  return LINS_OK;
}

}  // namespace

extern "C" {

void lins_team_pcm_default_params(lins_team_pcm_params* p) {
  if (p) lins_pcm::default_params(p);
}

int lins_team_factors_consistent_batch(lins_ctx* ctx, int n_groups, const lins_team_member* members, const int32_t* member_offsets,
                                       const lins_team_factor* factors, const int32_t* factor_offsets, const lins_team_pcm_params* prm,
                                       lins_team_pcm_result* out) {
  if (!ctx || n_groups < 0 || (n_groups && (!member_offsets || !factor_offsets || !out)) || !lins_pcm::params_ok(prm)) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  PcmWs& w = m->pcm;
  if (n_groups == 0) return LINS_OK;
  std::vector<lins_pcm::Rec> recs;
  if (int rc = pcm_check(m, n_groups, members, member_offsets, factors, factor_offsets, recs)) return rc;
  // (every refusal is behind us)
  w.kernel_ms = 0.f;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  const size_t rec_bytes = recs.size() * sizeof(lins_pcm::Rec), o_off = align64(rec_bytes),
               up_bytes = align64(o_off + ((size_t)n_groups + 1) * sizeof(int32_t)), down_bytes = (size_t)n_groups * sizeof(lins_team_pcm_result);
  BUF_TRY(ctx, w.h_up.grow(up_bytes));
  BUF_TRY(ctx, w.d_up.grow(up_bytes));
  BUF_TRY(ctx, w.h_down.grow(down_bytes));
  BUF_TRY(ctx, w.d_down.grow(down_bytes));
  for (int i = 0; i < 2; ++i) BUF_TRY(ctx, w.ev[i].create());
  if (rec_bytes) std::memcpy(w.h_up, recs.data(), rec_bytes);
  std::memcpy(w.h_up + o_off, factor_offsets, ((size_t)n_groups + 1) * sizeof(int32_t));
  hipStream_t st = ctx_stream(ctx);
  HIP_TRY(ctx, hipMemcpyAsync(w.d_up, w.h_up, up_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipEventRecord(w.ev[0], st));
  launch_team_pcm(st, n_groups, (const lins_pcm::Rec*)w.d_up.get(), (const int*)(w.d_up + o_off), *prm, (lins_team_pcm_result*)w.d_down.get());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(w.ev[1], st));
  HIP_TRY(ctx, hipMemcpyAsync(w.h_down, w.d_down, down_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&w.kernel_ms, w.ev[0], w.ev[1]));
  std::memcpy(out, w.h_down, down_bytes);
  return LINS_OK;
}

int lins_last_team_pcm_stats(lins_ctx* ctx, float* kernel_ms) {
  if (!ctx) return LINS_E_ARG;
  if (kernel_ms) *kernel_ms = mem_of(ctx)->pcm.kernel_ms;
  return LINS_OK;
}

/* Debug aid (tests/test_gpu_team_pcm.py): the search stage alone on a given graph, the twin of lins_host_team_pcm_clique
 * and with its refusals — the device function the production kernel calls, behind a kernel that loads rows and pair keys
 * from memory. */
int lins_debug_team_pcm_clique(lins_ctx* ctx, int n, const uint64_t* adj, const int32_t* pair, const lins_team_pcm_params* prm,
                               lins_team_pcm_result* out) {
  if (!ctx || !out || n < 0 || n > lins_pcm::kMaxFactors || (n && (!adj || !pair)) || !lins_pcm::params_ok(prm)) return LINS_E_ARG;
  if (int rc = lins_pcm::graph_check(n, adj, pair)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  DevBuf<uint64_t> d_adj;
  DevBuf<int> d_key;
  DevBuf<lins_team_pcm_result> d_out;
  BUF_TRY(ctx, d_adj.grow(lins_pcm::kMaxFactors));
  BUF_TRY(ctx, d_key.grow(lins_pcm::kMaxFactors));
  BUF_TRY(ctx, d_out.grow(1));
  hipStream_t st = ctx_stream(ctx);
  if (n) {
    HIP_TRY(ctx, hipMemcpyAsync(d_adj, adj, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_key, pair, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  }
  launch_team_pcm_clique(st, n, d_adj, d_key, *prm, d_out);
  HIP_TRY(ctx, hipGetLastError());
  lins_team_pcm_result r;
  HIP_TRY(ctx, hipMemcpyAsync(&r, d_out, sizeof r, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  *out = r;
  return LINS_OK;
}

}  // extern "C"
