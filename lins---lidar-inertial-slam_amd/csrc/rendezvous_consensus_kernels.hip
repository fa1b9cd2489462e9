// rendezvous_consensus_kernels.hip — the consensus rule of a rendezvous over a window, on the device (include/lins_team.h
// lins_rendezvous_consensus_batch).  The rule is host/rendezvous_consensus.h: the kernel CALLS that text — consistent,
// popcount16, before — on its LDS copy of the table, so every decision has the host's bits by construction.  One workgroup
// of 128 lanes serves one entry, one lane per hypothesis:
//   stage    the entry's H <= 128 hypotheses, 22 doubles each in the caller's layout, are read once (8-byte loads, the
//            lanes stride over the table's words): the 20 doubles into rec, the four integers into tag — 20 KiB + 2 KiB
//   support  lane a keeps its own record in registers and walks all H records — the same LDS address in every lane, a
//            broadcast — and forms its query mask
//   winner   a comparison tree over the lanes' indices in LDS, seven rounds under workgroup barriers; the order is
//            total, so the tree's shape does not show
//   members  every lane asks the winner about itself; lane 0 packs the flags and stores the 32-byte record as two
//            16-byte vector stores
// No global atomics, no LDS atomics, no scratch; nothing here depends on the wave size: whatever crosses lanes goes
// through LDS and __syncthreads().  The host has checked the table (lins_consensus::table_check): H, query and rank are
// in range before the launch.
#include <hip/hip_runtime.h>

#include "host/rendezvous_consensus.h"
#include "lins_launch.h"

namespace lins {
namespace {

using namespace lins_consensus;

constexpr int kCsWords = kDoubles + 2;  // a hypothesis in the caller's table, in 8-byte words
static_assert(kCsBlock == kMaxHyp, "one lane per hypothesis");

__global__ __launch_bounds__(kCsBlock) void rendezvous_consensus_kernel(const double* __restrict__ table, const int* __restrict__ offsets, Bars bars,
                                                                         int4* __restrict__ out) {
  __shared__ double rec[kMaxHyp][kDoubles];
  __shared__ Tag tag[kMaxHyp];
  __shared__ int support[kMaxHyp];
  __shared__ int best[kMaxHyp];
  __shared__ unsigned char member[kMaxHyp];
  const int e = blockIdx.x, tid = threadIdx.x;
  const int first = offsets[e];
  int H = offsets[e + 1] - first;
  H = H < 0 ? 0 : (H > kMaxHyp ? kMaxHyp : H);  // (the host has refused anything else; the kernel indexes nothing beyond its arrays all the same)
  // ---- stage ----
  const double* __restrict__ src = table + (long long)first * kCsWords;
  for (int i = tid; i < H * kCsWords; i += kCsBlock) {
    const int h = i / kCsWords, w = i - h * kCsWords;
    const double v = src[i];
    if (w < kDoubles) {
      rec[h][w] = v;
    } else {
      const long long bits = __double_as_longlong(v);
      int* t = (int*)&tag[h] + 2 * (w - kDoubles);  // (query, rank) | (slot, admissible)
      t[0] = (int)(unsigned)bits, t[1] = (int)(bits >> 32);
    }
  }
  __syncthreads();
  // ---- support ----
  double mine[kDoubles];
  Tag tm = Tag{0, 0, 0, 0};
  if (tid < H) {
#pragma unroll
    for (int j = 0; j < kDoubles; ++j) mine[j] = rec[tid][j];
    tm = tag[tid];
  } else {
#pragma unroll
    for (int j = 0; j < kDoubles; ++j) mine[j] = 0.0;
  }
  unsigned mask = tm.admissible ? 1u << tm.query : 0u;
  if (tm.admissible)
    for (int b = 0; b < H; ++b)
      if (b != tid && consistent(mine, tm, rec[b], tag[b], bars)) mask |= 1u << tag[b].query;
  support[tid] = popcount16(mask);
  best[tid] = tm.admissible ? tid : -1;
  __syncthreads();
  // ---- winner ----
  for (int s = kCsBlock >> 1; s > 0; s >>= 1) {
    if (tid < s) {
      const int a = best[tid], b = best[tid + s];
      if (b >= 0 && (a < 0 || before(support[b], rec[b][kFitness], tag[b], support[a], rec[a][kFitness], tag[a]))) best[tid] = b;
    }
    __syncthreads();
  }
  const int w = best[0];
  // ---- members ----
  member[tid] = w >= 0 && tid < H && (tid == w || consistent(rec[w], tag[w], mine, tm, bars)) ? 1 : 0;
  __syncthreads();
  if (tid == 0) {
    unsigned m[4] = {0u, 0u, 0u, 0u};
    int n_adm = 0;
    for (int h = 0; h < H; ++h) m[h >> 5] |= (unsigned)member[h] << (h & 31), n_adm += tag[h].admissible;
    out[2 * e] = make_int4(w, w >= 0 ? support[w] : 0, n_adm, 0);
    out[2 * e + 1] = make_int4((int)m[0], (int)m[1], (int)m[2], (int)m[3]);
  }
}

}  // namespace

void launch_rendezvous_consensus(hipStream_t s, int n, const lins_consensus_hyp* table, const int* offsets, double max_translation,
                                 double min_cos_rotation, lins_consensus_result* out) {
  static_assert(sizeof(lins_consensus_result) == 32, "two 16-byte stores");
  if (n > 0)
    hipLaunchKernelGGL(rendezvous_consensus_kernel, dim3(n), dim3(kCsBlock), 0, s, (const double*)table, offsets,
                       bars_of(max_translation, min_cos_rotation), (int4*)out);
}

}  // namespace lins
