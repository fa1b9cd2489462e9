// pose_graph_mem.h — what a context holds of its pose graphs, for the files that work on it: lins_pose_graph_capi.hip
// (the graphs, the single solve, the rebase, the write-back), lins_team_graph_capi.hip (the team solve over groups of
// them, with a workspace of its own that the first team solve allocates) and lins_team_pcm_capi.hip (which team factors
// agree: it reads the graphs' estimates and owns a staging of its own).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "lins_buf.h"
#include "local_map.h"
#include "pose_graph_team.h"

namespace lins {

// The team solve's workspace: the concatenated rows of every group of a call, grow-only.
//   per frame   Z, D, Dt, I, T, Tt (6 x 96 bytes), B and P (2 x 288), c and q (2 x 48): 1 248 bytes, and 96 bytes per
//               kPrefixBlock frames plus 192 per member for the prefix of blocks
//   per loop    the record (496 bytes), its support (32), 18 doubles of y (144), and 288 L bytes of S in a group of L loops
//   per group   the state (48 bytes), the problem record, 64 bytes a member of the member table
struct TeamWs {
  DevBuf<double> d_Z, d_D, d_Dt, d_I, d_T, d_Tt, d_Q, d_B, d_c, d_P, d_q, d_S, d_y;
  DevBuf<lins_pg::LoopRec> d_loops;
  DevBuf<lins_pg::TeamSpan> d_spans;
  DevBuf<lins_pg::TeamMember> d_members;
  DevBuf<lins_pg::TeamCopy> d_copy;
  DevBuf<lins_pg::State> d_st;
  DevBuf<lins_pg::TeamProb> d_probs;
  float ms = 0.f;
  uint64_t iterations = 0;
};

// The staging of lins_team_factors_consistent_batch (lins_team_pcm_capi.hip): grow-only, allocated by its first call.
struct PcmWs {
  DevBuf<char> d_up, d_down;  // (bytes) the records | the offsets; the results
  PinBuf<char> h_up, h_down;
  Event ev[2];  // around the launch
  float kernel_ms = 0.f;
};

struct PgMem {
  int n_slots = 0, F = 0, L = 0;
  std::vector<lins_pg::Graph> g;
  std::vector<int> up_frames, up_loops;  // what of each slot is on the device
  DevBuf<double> d_Z, d_D, d_Dt, d_I, d_T, d_Tt, d_Q;
  DevBuf<double> d_B, d_c, d_P, d_q, d_S, d_y;
  DevBuf<lins_pg::LoopRec> d_loops;
  DevBuf<lins_pg::State> d_st;
  DevBuf<lins_pg::Prob> d_probs;
  DevBuf<int> d_running;
  PinBuf<int> h_running;
  float ms = 0.f;
  uint64_t iterations = 0;
  TeamWs team;
  PcmWs pcm;
  size_t nq() const { return (size_t)F / lins_pg::kPrefixBlock + 2; }
};

inline void pg_free(void* p) { delete (PgMem*)p; }

inline PgMem* mem_of(lins_ctx* ctx) {
  void** slot = map_slot(ctx, kSlotGraph, pg_free);
  if (!*slot) *slot = new PgMem();
  return (PgMem*)*slot;
}

inline lins_pg::Prob prob_of(const PgMem* m, int slot, int idx) {
  const size_t s = (size_t)slot, F = (size_t)m->F, L = (size_t)m->L;
  lins_pg::Prob p{};
  p.n_frames = m->g[slot].n_frames(), p.n_loops = (int)m->g[slot].loops.size(), p.slot = slot;
  p.Z = m->d_Z + s * F * 12, p.D = m->d_D + s * F * 12, p.Dt = m->d_Dt + s * F * 12, p.I = m->d_I + s * F * 12;
  p.T = m->d_T + s * F * 12, p.Tt = m->d_Tt + s * F * 12, p.Q = m->d_Q + s * m->nq() * 12;
  p.B = m->d_B + s * F * 36, p.c = m->d_c + s * F * 6, p.P = m->d_P + s * F * 36, p.q = m->d_q + s * F * 6;
  p.loops = m->d_loops + s * L, p.S = m->d_S + s * 36 * L * L, p.y = m->d_y + s * 18 * L;
  p.st = m->d_st + idx;
  return p;
}

}  // namespace lins
