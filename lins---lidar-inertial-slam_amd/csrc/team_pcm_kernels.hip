// team_pcm_kernels.hip — pairwise-consistent team factors on the device (include/lins_team.h
// lins_team_factors_consistent_batch).  The rule is host/team_pcm.h: the kernel CALLS that text — form, consistent,
// subproblem, pair_winner, pair_head — on its LDS copy of the group, so every decision has the host's bits by
// construction.  One workgroup of 64 lanes serves one group, one lane per factor:
//   stage      the group's L <= 64 records, 39 8-byte words each (host/team_pcm.h Rec), are read once (8-byte loads, the
//              lanes stride over the group's words) into the 32 KiB block that later is the stack — 19.5 KiB of it
//   form       lane l forms X_l and p_l from its record and stores the 15 doubles and its four integers
//   adjacency  lane l keeps its own 15 doubles in registers and walks all L records — the same LDS address in every
//              lane, a broadcast — and packs its 64-bit row; on the way it finds the first factor of its member pair
//   search     lane s runs subproblem s; its stack of 64 words lies [depth][lane], so lanes at different depths meet in
//              one bank only by chance, and lanes at one depth never
//   reduce     per pair over LDS: lane l walks the sizes for its pair's winner; lane 0 packs the flags and stores the
//              32-byte record as two 16-byte vector stores
// The search and the reduction are one device function, search_and_store, with two callers: the production kernel and
// the debug kernel behind lins_debug_team_pcm_clique, which loads rows and pair keys from memory.
// No global atomics, no LDS atomics, no dynamically indexed private array; every loop bound in front of a barrier is the
// group's own L, and no return comes in front of a barrier.  Whatever crosses lanes goes through LDS and __syncthreads().
// The host has checked the group: L is in range before the launch.
#include <hip/hip_runtime.h>

#include "host/team_pcm.h"
#include "lins_launch.h"

namespace lins {
namespace {

using namespace lins_pcm;

static_assert(kPcmBlock == kMaxFactors, "one lane per factor");
constexpr int kStackWords = kLevels * kPcmBlock;  // 32 KiB: a complete graph of 64 in every lane
static_assert(kStackWords >= kMaxFactors * kRecWords, "the staged records fit the block that becomes the stack");

struct PcmShared {
  uint64_t stack[kStackWords];  // the staged records first
  double xp[kMaxFactors][kXp];
  Tag tag[kMaxFactors];
  uint64_t adj[kMaxFactors];
  uint64_t best[kMaxFactors];
  int32_t key[kMaxFactors];
  int32_t size[kMaxFactors];
  uint32_t nodes[kMaxFactors];
  unsigned char exhausted[kMaxFactors], kept[kMaxFactors], head[kMaxFactors], head_kept[kMaxFactors];
};

// adj and key of the L vertices are in sh and a barrier is behind them
__device__ void search_and_store(PcmShared& sh, int L, int tid, int min_support, uint32_t max_nodes, int4* __restrict__ out) {
  Sub sub = Sub{0, 0, 0u, 0};
  if (tid < L) sub = subproblem(tid, sh.adj, max_nodes, sh.stack + tid, kPcmBlock);
  sh.best[tid] = sub.best, sh.size[tid] = sub.size, sh.nodes[tid] = sub.nodes, sh.exhausted[tid] = (unsigned char)sub.exhausted;
  __syncthreads();
  bool kept = false, head = false, head_kept = false;
  if (tid < L) {
    const int w = pair_winner(tid, L, sh.key, sh.size);
    const bool pair_kept = sh.size[w] >= min_support;
    kept = pair_kept && ((sh.best[w] >> tid) & 1u);
    head = pair_head(tid, sh.key);
    head_kept = head && pair_kept;
  }
  sh.kept[tid] = kept, sh.head[tid] = head, sh.head_kept[tid] = head_kept;
  __syncthreads();
  if (tid == 0) {
    unsigned m0 = 0u, m1 = 0u, nodes_max = 0u;  // (two scalars: no private array indexed by l)
    int n_kept = 0, n_pairs = 0, n_pairs_kept = 0, exact = 1;
    for (int l = 0; l < L; ++l) {
      const unsigned bit = (unsigned)sh.kept[l] << (l & 31);
      if (l < 32)
        m0 |= bit;
      else
        m1 |= bit;
      n_kept += sh.kept[l], n_pairs += sh.head[l], n_pairs_kept += sh.head_kept[l];
      if (sh.exhausted[l]) exact = 0;
      if (sh.nodes[l] > nodes_max) nodes_max = sh.nodes[l];
    }
    out[0] = make_int4(L, n_kept, n_pairs, n_pairs_kept);
    out[1] = make_int4(exact, (int)nodes_max, (int)m0, (int)m1);
  }
}

__global__ __launch_bounds__(kPcmBlock) void team_pcm_kernel(const double* __restrict__ recs, const int* __restrict__ offsets, Bars bars,
                                                             int min_support, uint32_t max_nodes, int4* __restrict__ out) {
  __shared__ PcmShared sh;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int first = offsets[g];
  int L = offsets[g + 1] - first;
  L = L < 0 ? 0 : (L > kMaxFactors ? kMaxFactors : L);  // (the host has refused anything else; the kernel indexes nothing beyond its arrays all the same)
  // ---- stage ----
  const double* __restrict__ src = recs + (long long)first * kRecWords;
  double* staged = (double*)sh.stack;
  for (int i = tid; i < L * kRecWords; i += kPcmBlock) staged[i] = src[i];
  __syncthreads();
  // ---- form ----
  double mine[kXp];
  Tag tm = Tag{-1, -1, -1, -1};
#pragma unroll
  for (int j = 0; j < kXp; ++j) mine[j] = 0.0;
  if (tid < L) {
    const Rec* r = (const Rec*)(staged + tid * kRecWords);
    double Z[12], Tu[12], Tv[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) Z[j] = r->Z[j], Tu[j] = r->Tu[j], Tv[j] = r->Tv[j];
    form(Z, r->flip, Tu, Tv, mine);
    tm = r->tag;
#pragma unroll
    for (int j = 0; j < kXp; ++j) sh.xp[tid][j] = mine[j];
    sh.tag[tid] = tm;
  }
  __syncthreads();  // (the staged records are dead behind this barrier: the block is the stack now)
  // ---- adjacency ----
  uint64_t row = 0;
  int key = tid;
  if (tid < L)
    for (int m = L - 1; m >= 0; --m) {
      const Tag t = sh.tag[m];
      if (m != tid && consistent(mine, tm, sh.xp[m], t, bars)) row |= (uint64_t)1 << m;
      if (m < tid && t.u == tm.u && t.v == tm.v) key = m;  // (descending: the first of the pair stays)
    }
  sh.adj[tid] = row, sh.key[tid] = key;
  __syncthreads();
  search_and_store(sh, L, tid, min_support, max_nodes, out + 2 * g);
}

// the search on given rows: adj and key hold n entries
__global__ __launch_bounds__(kPcmBlock) void team_pcm_clique_kernel(const uint64_t* __restrict__ adj, const int* __restrict__ key, int n,
                                                                    int min_support, uint32_t max_nodes, int4* __restrict__ out) {
  __shared__ PcmShared sh;
  const int tid = threadIdx.x;
  const int L = n < 0 ? 0 : (n > kMaxFactors ? kMaxFactors : n);
  sh.adj[tid] = tid < L ? adj[tid] : 0, sh.key[tid] = tid < L ? key[tid] : -1 - tid;
  __syncthreads();
  search_and_store(sh, L, tid, min_support, max_nodes, out);
}

}  // namespace

void launch_team_pcm(hipStream_t s, int n_groups, const lins_pcm::Rec* recs, const int* offsets, const lins_team_pcm_params& prm,
                     lins_team_pcm_result* out) {
  if (n_groups > 0)
    hipLaunchKernelGGL(team_pcm_kernel, dim3(n_groups), dim3(kPcmBlock), 0, s, (const double*)recs, offsets, bars_of(prm), prm.min_support,
                       (uint32_t)prm.max_nodes, (int4*)out);
}

void launch_team_pcm_clique(hipStream_t s, int n, const uint64_t* adj, const int* key, const lins_team_pcm_params& prm, lins_team_pcm_result* out) {
  hipLaunchKernelGGL(team_pcm_clique_kernel, dim3(1), dim3(kPcmBlock), 0, s, adj, key, n, prm.min_support, (uint32_t)prm.max_nodes, (int4*)out);
}

}  // namespace lins
