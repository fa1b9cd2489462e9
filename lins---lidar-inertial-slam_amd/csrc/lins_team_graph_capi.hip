// lins_team_graph_capi.hip — C ABI of the team graph (include/lins_team.h lins_team_graph_*): host orchestration around
// team_graph_kernels.hip.  A group's rows are gathered from its members' rows on the device into the team workspace
// (pose_graph_mem.h TeamWs), solved there by one workgroup, and scattered back; the members' graphs on the host are
// written through Graph::store_solution and Graph::store_rebased, so that everything that follows a single solve or a
// rebase — a later solve, a snapshot, lins_pose_graph_apply_batch — follows a team solve by the same code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lins_map.h"
#include "../../include/lins_team.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "local_map.h"
#include "pose_graph_mem.h"
#include "pose_graph_team.h"

using namespace lins;
using lins_pg::Graph;
using lins_pg::LoopRec;
using lins_pg::State;
using lins_pg::TeamCopy;
using lins_pg::TeamFactorIn;
using lins_pg::TeamMember;
using lins_pg::TeamProb;
using lins_pg::TeamSpan;

namespace {

constexpr int kTeamTrials = 4;  // trials queued between two reads of the "still running" word: the single solve's

struct Group {  // a checked group
  int m0, m1, f0, f1;  // its members and factors in the call's arrays
  int frames, own_loops, q_rows;
  std::vector<TeamMember> mt;
  std::vector<TeamFactorIn> fin;
};

// everything lins_team_graph_solve refuses, and the groups as the solve takes them
int team_check(PgMem* m, int n_groups, const lins_team_member* members, const int32_t* moff, const lins_team_factor* factors,
               const int32_t* foff, std::vector<Group>& groups) {
  if (moff[0] != 0 || foff[0] != 0) return LINS_E_ARG;
  for (int g = 0; g < n_groups; ++g)
    if (moff[g + 1] <= moff[g] || foff[g + 1] < foff[g]) return LINS_E_ARG;  // (an empty group: no anchor)
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
  for (int g = 0; g < n_groups; ++g) {
    for (int i = moff[g] + 1; i < moff[g + 1]; ++i)
      for (int p = 0; p < 6; ++p)
        if (!lins_pg::team_var_ok(members[i].root_variance[p])) return LINS_E_INPUT;
    for (int i = foff[g]; i < foff[g + 1]; ++i)
      if (!lins_pg::team_z_ok(factors[i].Z) || !lins_pg::team_var_ok(factors[i].var)) return LINS_E_INPUT;
  }
  groups.assign(n_groups, Group());
  for (int g = 0; g < n_groups; ++g) {
    Group& G = groups[g];
    G.m0 = moff[g], G.m1 = moff[g + 1], G.f0 = foff[g], G.f1 = foff[g + 1];
    const int nm = G.m1 - G.m0;
    if (nm > lins_pg::kTeamMaxMembers) return LINS_E_CAPACITY;
    std::vector<int> counts(nm);
    std::vector<const double*> var(nm);
    G.own_loops = 0;
    for (int i = 0; i < nm; ++i) {
      const Graph& gr = m->g[members[G.m0 + i].slot];
      counts[i] = gr.n_frames(), var[i] = members[G.m0 + i].root_variance, G.own_loops += (int)gr.loops.size();
    }
    const long long cap = std::min<long long>(lins_pg::kMaxLoops, (long long)nm * m->L);
    if ((long long)G.own_loops + (G.f1 - G.f0) > cap) return LINS_E_CAPACITY;
    G.mt.resize(nm);
    G.frames = lins_pg::team_members(nm, counts.data(), var.data(), G.mt.data(), &G.q_rows);
    for (int i = G.f0; i < G.f1; ++i)
      G.fin.push_back(TeamFactorIn{member_of[factors[i].slot_b], factors[i].id_b, member_of[factors[i].slot_a], factors[i].id_a, factors[i].Z, factors[i].var});
  }
  return LINS_OK;
}

}  // namespace

extern "C" {

int lins_team_factor_from_alignment(lins_ctx* ctx, int slot_b, int id_b, int slot_a, int id_a, const double* X, double fitness,
                                    lins_team_factor* out) {
  if (!ctx || !out) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (slot_b < 0 || slot_b >= m->n_slots || slot_a < 0 || slot_a >= m->n_slots || slot_a == slot_b) return LINS_E_ARG;
  const Graph &gb = m->g[slot_b], &ga = m->g[slot_a];
  if (id_b < 0 || id_b >= gb.n_frames() || id_a < 0 || id_a >= ga.n_frames()) return LINS_E_ARG;
  const double var = (double)(float)fitness;
  if ((X && !lins_pg::rebase_x_ok(X)) || !lins_pg::team_var_ok(var)) return LINS_E_INPUT;
  double Xg[12];
  if (X) lins_pg::rebase_x_pose(X, Xg);
  std::memset(out, 0, sizeof *out);
  out->slot_b = slot_b, out->id_b = id_b, out->slot_a = slot_a, out->id_a = id_a, out->var = var;
  lins_pg::team_factor_z(&gb.T[12 * (size_t)id_b], &ga.T[12 * (size_t)id_a], X ? Xg : nullptr, out->Z);
  return LINS_OK;
}

int lins_team_graph_solve(lins_ctx* ctx, int n_groups, const lins_team_member* members, const int32_t* member_offsets,
                          const lins_team_factor* factors, const int32_t* factor_offsets, const lins_pose_graph_params* prm,
                          lins_team_graph_result* out) {
  if (!ctx || n_groups < 0 || (n_groups && (!member_offsets || !factor_offsets || !out)) || !lins_pg::params_ok(prm)) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  TeamWs& w = m->team;
  w.ms = 0.f, w.iterations = 0;
  if (n_groups == 0) return LINS_OK;
  std::vector<Group> groups;
  if (int rc = team_check(m, n_groups, members, member_offsets, factors, factor_offsets, groups)) return rc;

  std::vector<int> run;  // the groups with a loop or a factor: the others are returned with the bits they hold
  for (int g = 0; g < n_groups; ++g) {
    std::memset(out + g, 0, sizeof out[g]);
    out[g].n_frames = groups[g].frames, out[g].n_loops = groups[g].own_loops, out[g].n_factors = groups[g].f1 - groups[g].f0;
    if (groups[g].own_loops + (groups[g].f1 - groups[g].f0) > 0) run.push_back(g);
  }
  if (run.empty()) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx_device(ctx)));
  hipStream_t st = ctx_stream(ctx);
  const int nr = (int)run.size();

  // the workspace's sizes and every group's place in it
  size_t frames = 0, q_rows = 0, n_loops = 0, s_doubles = 0, n_members = 0;
  std::vector<size_t> at_frame(nr), at_q(nr), at_loop(nr), at_s(nr), at_member(nr);
  std::vector<LoopRec> loops, gl;
  std::vector<TeamSpan> spans, gs;
  std::vector<TeamMember> table;
  for (int i = 0; i < nr; ++i) {
    const Group& G = groups[run[i]];
    const int nm = G.m1 - G.m0;
    at_frame[i] = frames, at_q[i] = q_rows, at_loop[i] = n_loops, at_s[i] = s_doubles, at_member[i] = n_members;
    std::vector<const std::vector<LoopRec>*> own(nm);
    for (int k = 0; k < nm; ++k) own[k] = &m->g[members[G.m0 + k].slot].loops;
    lins_pg::team_loops(nm, G.mt.data(), own.data(), (int)G.fin.size(), G.fin.data(), gl, gs);
    loops.insert(loops.end(), gl.begin(), gl.end()), spans.insert(spans.end(), gs.begin(), gs.end());
    table.insert(table.end(), G.mt.begin(), G.mt.end());
    frames += (size_t)G.frames, q_rows += (size_t)G.q_rows, n_loops += gl.size(), s_doubles += 36 * gl.size() * gl.size(), n_members += (size_t)nm;
  }
  for (DevBuf<double>* p : {&w.d_Z, &w.d_D, &w.d_Dt, &w.d_I, &w.d_T, &w.d_Tt}) BUF_TRY(ctx, p->grow(frames * 12));
  BUF_TRY(ctx, w.d_Q.grow(q_rows * 12));
  BUF_TRY(ctx, w.d_B.grow(frames * 36));
  BUF_TRY(ctx, w.d_P.grow(frames * 36));
  BUF_TRY(ctx, w.d_c.grow(frames * 6));
  BUF_TRY(ctx, w.d_q.grow(frames * 6));
  BUF_TRY(ctx, w.d_S.grow(s_doubles));
  BUF_TRY(ctx, w.d_y.grow(n_loops * 18));
  BUF_TRY(ctx, w.d_loops.grow(n_loops));
  BUF_TRY(ctx, w.d_spans.grow(n_loops));
  BUF_TRY(ctx, w.d_members.grow(n_members));
  BUF_TRY(ctx, w.d_copy.grow(n_members));
  BUF_TRY(ctx, w.d_st.grow((size_t)nr));
  BUF_TRY(ctx, w.d_probs.grow((size_t)nr));

  std::vector<TeamProb> probs(nr);
  std::vector<State> states(nr);
  std::vector<TeamCopy> copies(n_members);
  for (int i = 0; i < nr; ++i) {
    const Group& G = groups[run[i]];
    const int nm = G.m1 - G.m0;
    const size_t f = at_frame[i];
    TeamProb& P = probs[i];
    P = TeamProb{};
    P.n_members = nm, P.n_frames = G.frames, P.n_loops = (int)((i + 1 < nr ? at_loop[i + 1] : n_loops) - at_loop[i]);
    P.members = w.d_members + at_member[i];
    P.Z = w.d_Z + 12 * f, P.D = w.d_D + 12 * f, P.Dt = w.d_Dt + 12 * f, P.I = w.d_I + 12 * f, P.T = w.d_T + 12 * f, P.Tt = w.d_Tt + 12 * f;
    P.Q = w.d_Q + 12 * at_q[i];
    P.B = w.d_B + 36 * f, P.c = w.d_c + 6 * f, P.P = w.d_P + 36 * f, P.q = w.d_q + 6 * f;
    P.loops = w.d_loops + at_loop[i], P.spans = w.d_spans + at_loop[i], P.S = w.d_S + at_s[i], P.y = w.d_y + 18 * at_loop[i];
    P.st = w.d_st + i;
    lins_pg::state_init(states[i], *prm);
    for (int k = 0; k < nm; ++k) {
      const int slot = members[G.m0 + k].slot;
      const Graph& gr = m->g[slot];
      const lins_pg::Prob own = prob_of(m, slot, 0);
      const int f0 = m->up_frames[slot], f1 = gr.n_frames();
      if (f1 > f0) {  // the member's new frames into its own rows, as a solve uploads them
        HIP_TRY(ctx, hipMemcpyAsync(own.Z + 12 * (size_t)f0, gr.Z.data() + 12 * (size_t)f0, 12 * (size_t)(f1 - f0) * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(own.D + 12 * (size_t)f0, gr.Z.data() + 12 * (size_t)f0, 12 * (size_t)(f1 - f0) * sizeof(double), hipMemcpyHostToDevice, st));
      }
      TeamCopy& c = copies[at_member[i] + k];
      const size_t row = f + (size_t)G.mt[k].off;
      c.mZ = own.Z, c.mD = own.D, c.mT = own.T;
      c.gZ = w.d_Z + 12 * row, c.gD = w.d_D + 12 * row, c.gT = w.d_T + 12 * row;
      c.n = f1, c.root = k > 0, c.store = 0, c.pad = 0;
    }
  }
  HIP_TRY(ctx, hipMemcpyAsync(w.d_members, table.data(), n_members * sizeof(TeamMember), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_copy, copies.data(), n_members * sizeof(TeamCopy), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_loops, loops.data(), n_loops * sizeof(LoopRec), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_spans, spans.data(), n_loops * sizeof(TeamSpan), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_probs, probs.data(), (size_t)nr * sizeof(TeamProb), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(w.d_st, states.data(), (size_t)nr * sizeof(State), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(m->d_running, 0, 128 * sizeof(int), st));
  HIP_TRY(ctx, hipStreamSynchronize(st));  // (pageable sources)
  for (int i = 0; i < nr; ++i)
    for (int k = groups[run[i]].m0; k < groups[run[i]].m1; ++k) m->up_frames[members[k].slot] = m->g[members[k].slot].n_frames();

  hipEvent_t e0, e1;
  ctx_events(ctx, &e0, &e1);
  HIP_TRY(ctx, hipEventRecord(e0, st));
  launch_team_graph_copy(st, (int)n_members, w.d_copy, false);
  launch_team_graph_begin(st, nr, w.d_probs);
  for (int done = 0, grp = 0; done < prm->max_iterations; ++grp) {
    const int cnt = std::min(kTeamTrials, prm->max_iterations - done);
    int* word = m->d_running + (grp & 127);
    if (grp >= 128) HIP_TRY(ctx, hipMemsetAsync(word, 0, sizeof(int), st));
    for (int i = 0; i < cnt; ++i) launch_team_graph_trial(st, nr, w.d_probs, *prm, i + 1 == cnt ? word : nullptr);
    HIP_TRY(ctx, hipGetLastError());
    done += cnt;
    if (done >= prm->max_iterations) break;
    HIP_TRY(ctx, hipMemcpyAsync(m->h_running, word, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (*m->h_running == 0) break;
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(e1, st));
  std::vector<double> T(12 * frames);
  HIP_TRY(ctx, hipMemcpyAsync(T.data(), w.d_T, T.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(states.data(), w.d_st, (size_t)nr * sizeof(State), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  HIP_TRY(ctx, hipEventElapsedTime(&w.ms, e0, e1));

  // the check of the solved poses, then the members' graphs on the host and their rows on the device
  for (int i = 0; i < nr; ++i) {
    const Group& G = groups[run[i]];
    const State& s = states[i];
    const double* Tg = T.data() + 12 * at_frame[i];
    bool ok = true;
    for (int k = 0; k < G.frames && ok; ++k) ok = lins_pg::team_pose_storable(Tg + 12 * (size_t)k);
    lins_pose_graph_result& r = out[run[i]].solve;
    r.cost_before = s.cost0, r.cost_after = s.cost, r.max_increment = s.max_inc;
    r.iterations = s.iterations, r.reason = s.reason, r.status = ok ? LINS_OK : LINS_E_INPUT;
    w.iterations += (uint64_t)s.iterations;
    for (int k = 0; k < G.m1 - G.m0; ++k) {
      copies[at_member[i] + k].store = ok;
      if (!ok) continue;
      Graph& gr = m->g[members[G.m0 + k].slot];
      const double* Tm = Tg + 12 * (size_t)G.mt[k].off;
      gr.store_solution(Tm, nullptr);
      if (k > 0) gr.store_rebased(Tm, Tm);  // the solved root is the prior now: Z[0], and frame 0's estimate
    }
  }
  HIP_TRY(ctx, hipMemcpyAsync(w.d_copy, copies.data(), n_members * sizeof(TeamCopy), hipMemcpyHostToDevice, st));
  launch_team_graph_copy(st, (int)n_members, w.d_copy, true);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return LINS_OK;
}

int lins_last_team_graph_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* iterations) {
  if (!ctx) return LINS_E_ARG;
  PgMem* m = mem_of(ctx);
  if (!m->n_slots) return LINS_E_STATE;
  if (kernel_ms) *kernel_ms = m->team.ms;
  if (iterations) *iterations = m->team.iterations;
  return LINS_OK;
}

}  // extern "C"
