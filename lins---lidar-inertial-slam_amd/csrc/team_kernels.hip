// team_kernels.hip — the team search on the device (include/lins_team.h; the contract is the lower part of
// host/place_math.h + host/place.cpp lins_host_place_team_topk, bit for bit; the records are place.h).
//   key        one wave per stale frame, a lane per sector: ring r's occupancy is the population count of the wave's
//              ballot of D[r][lane] > 0 — twenty coalesced 240-byte reads a frame; lane 0 stores the 32-byte record.
//   shortlist  one workgroup per (query, chunk of the call's concatenated candidates).  A lane forms the keys of the
//              candidates it strides over: the candidate's record is two 16-byte loads, the query's the same address in
//              every lane (scalar loads); dk = sumsq_q + sumsq_c - 2 dot, the dot of the 20 byte pairs five v_dot4_u32_u8
//              — integers, so the form changes no bit.  The lane finds its first candidate's slot by bisection over the
//              targets' first places and walks forward from there.  The chunk's keys lie in LDS; M rounds each take the
//              minimum above the last round's winner (the keys are distinct, so nothing is marked): a lane's minimum
//              over its stride, the wave's by shuffles on the key's halves, the workgroup's through LDS across the waves
//              — place_select_kernel's pattern.
//   merge      one workgroup per query: the same M rounds over its chunks' lists, re-read from L2 each round.
//   pair       place_search_kernel's column walk over (query, shortlist position) pairs instead of a contiguous range:
//              one workgroup per (query, ten positions); the ten candidates' records come from wherever their slots lie.
//              The query's columns are the same address in every lane, as there.  A pair's row key carries its
//              shortlist position where the search's carries the id.
// A minimum depends on no order and the shortlist's order is total: the bits depend neither on the chunk nor on the order
// of the targets.  Plain vector stores, no global atomics.
#include <hip/hip_runtime.h>

#include "host/place_math.h"
#include "lins_launch.h"
#include "place.h"

namespace lins {
namespace {

using namespace lins_place;

constexpr int kPrBlock = 128;                   // threads of the pair kernel: the search's shape
constexpr int kPrShifts = 5;                    // shifts per lane
constexpr int kPrLanes = kNS / kPrShifts;       // lanes per candidate
constexpr int kPrPass = kPrBlock / kPrLanes;    // candidates of one workgroup
static_assert(kPrLanes * kPrShifts == kNS && kPrPass * kPrLanes <= kPrBlock, "pair shape");
static_assert(kNR == 20 && kNS <= 64 && sizeof(RingKey) == 32, "key shape");
static_assert(kTmBlock % 64 == 0, "whole waves");

__global__ __launch_bounds__(kTmBlock) void team_key_kernel(int n, const TmStale* __restrict__ stale, const float* __restrict__ D,
                                                            uint4* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * (kTmBlock / 64) + (threadIdx.x >> 6);  // (uniform over the wave)
  if (f >= n) return;
  const TmStale z = stale[f];
  const float* __restrict__ d = D + z.rec * kCells;
  unsigned w[kNR / 4] = {0u, 0u, 0u, 0u, 0u}, sq = 0u;
#pragma unroll
  for (int r = 0; r < kNR; ++r) {
    const bool on = lane < kNS && d[r * kNS + lane] > 0.f;
    const unsigned occ = (unsigned)__popcll(__ballot(on));
    w[r / 4] |= occ << (8 * (r % 4)), sq += occ * occ;
  }
  if (lane == 0) {
    const unsigned long long t = (unsigned long long)__double_as_longlong(z.time);
    keys[2 * z.rec] = make_uint4(w[0], w[1], w[2], w[3]);
    keys[2 * z.rec + 1] = make_uint4(w[4], sq, (unsigned)t, (unsigned)(t >> 32));
  }
}

// the workgroup's minimum of `best` (every lane calls; two barriers); part: one word per wave
__device__ inline unsigned long long block_min(unsigned long long best, unsigned long long* part, unsigned long long* winner) {
  unsigned hi = (unsigned)(best >> 32), lo = (unsigned)best;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned ohi = __shfl_xor(hi, off), olo = __shfl_xor(lo, off);
    const bool less = ohi < hi || (ohi == hi && olo < lo);
    hi = less ? ohi : hi, lo = less ? olo : lo;
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ((unsigned long long)hi << 32) | lo;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long w = part[0];
    for (int i = 1; i < kTmBlock / 64; ++i) w = part[i] < w ? part[i] : w;
    *winner = w;
  }
  __syncthreads();  // (winner is written; part is free for the next round)
  return *winner;
}

// M rounds over the n keys at K (LDS or global): out[j] = the j-th smallest, kNoKey behind the last one there is
__device__ inline void take_minima(const unsigned long long* K, int n, int M, unsigned long long* __restrict__ out, unsigned long long* part,
                                   unsigned long long* winner) {
  unsigned long long last = 0ull;
  int j = 0;
  for (; j < M; ++j) {  // (j and the exit are uniform over the workgroup)
    unsigned long long best = kNoKey;
    for (int i = threadIdx.x; i < n; i += kTmBlock) {
      const unsigned long long key = K[i];
      if (key < best && (j == 0 || key > last)) best = key;
    }
    last = block_min(best, part, winner);
    if (last == kNoKey) break;
    if (threadIdx.x == 0) out[j] = last;
  }
  for (int i = j + threadIdx.x; i < M; i += kTmBlock) out[i] = kNoKey;
}

__global__ __launch_bounds__(kTmBlock) void team_shortlist_kernel(const TmQuery* __restrict__ queries, const TmTarget* __restrict__ targets, int n_targets,
                                                                  long long total, int chunk, int n_chunks, int M, const uint4* __restrict__ keys,
                                                                  unsigned long long* __restrict__ lists) {
  __shared__ unsigned long long K[kTmChunk];
  __shared__ unsigned long long part[kTmBlock / 64];
  __shared__ unsigned long long winner;
  const int tid = threadIdx.x;
  const int q = blockIdx.x / n_chunks, ch = blockIdx.x % n_chunks;
  const TmQuery e = queries[q];
  const long long g0 = (long long)ch * chunk;
  const int cnt = (int)(total - g0 < chunk ? total - g0 : chunk);  // <= chunk <= kTmChunk
  const uint4 qa = keys[2 * e.q_rec], qb = keys[2 * e.q_rec + 1];  // the same address in every lane
  if (tid < cnt) {
    // the target of this lane's first candidate: the last one whose first place is <= g (an empty slot shares its
    // successor's place and is passed over)
    int lo = 0, hi = n_targets - 1;
    const long long g = g0 + tid;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (targets[mid].first <= g) lo = mid; else hi = mid - 1;
    }
    int t = lo;
    TmTarget T = targets[t];
    for (int i = tid; i < cnt; i += kTmBlock) {
      const long long gi = g0 + i;
      while (t + 1 < n_targets && targets[t + 1].first <= gi) T = targets[++t];
      const int id = (int)(gi - T.first);  // < T.nf: gi < total, and the next target with frames starts at T.first + T.nf
      const uint4 ca = keys[2 * (T.base + id)], cb = keys[2 * (T.base + id) + 1];
      double time_c;
      const unsigned long long tb = (unsigned long long)cb.z | ((unsigned long long)cb.w << 32);
      __builtin_memcpy(&time_c, &tb, 8);
      unsigned dot = __builtin_amdgcn_udot4(qa.x, ca.x, 0u, false);
      dot = __builtin_amdgcn_udot4(qa.y, ca.y, dot, false);
      dot = __builtin_amdgcn_udot4(qa.z, ca.z, dot, false);
      dot = __builtin_amdgcn_udot4(qa.w, ca.w, dot, false);
      dot = __builtin_amdgcn_udot4(qb.x, cb.x, dot, false);
      const int dk = (int)(qb.y + cb.y - 2u * dot);
      K[i] = team_admits(T.slot, id, time_c, e.slot, e.id, e.now, e.gap) ? pack_team_key(dk, T.slot, id) : kNoKey;
    }
  }
  __syncthreads();
  take_minima(K, cnt, M, lists + (long long)blockIdx.x * M, part, &winner);
}

__global__ __launch_bounds__(kTmBlock) void team_merge_kernel(int n_chunks, int M, const unsigned long long* __restrict__ lists,
                                                              unsigned long long* __restrict__ shortlist) {
  __shared__ unsigned long long part[kTmBlock / 64];
  __shared__ unsigned long long winner;
  take_minima(lists + (long long)blockIdx.x * n_chunks * M, n_chunks * M, M, shortlist + (long long)blockIdx.x * M, part, &winner);
}

__device__ inline void load_column(float* w, const float* col) {
  for (int r = 0; r < kNR; r += 4) {
    const float4 v = *(const float4*)(col + r);
    w[r] = v.x, w[r + 1] = v.y, w[r + 2] = v.z, w[r + 3] = v.w;
  }
}

__device__ inline unsigned long long mask_of(const float* rec) {
  const unsigned* w = (const unsigned*)rec;
  return (unsigned long long)w[kPlMaskWord] | ((unsigned long long)w[kPlMaskWord + 1] << 32);
}

__global__ __launch_bounds__(kPrBlock) void team_pair_kernel(const TmQuery* __restrict__ queries, int M, int passes, int max_frames,
                                                             const unsigned long long* __restrict__ shortlist, const float* __restrict__ recs,
                                                             unsigned long long* __restrict__ row) {
  __shared__ __attribute__((aligned(16))) float cu[kPrPass][kPlRecWords];
  __shared__ unsigned long long cbest[kPrPass];
  __shared__ long long crec[kPrPass];
  const int tid = threadIdx.x;
  const int q = blockIdx.x / passes, m0 = (blockIdx.x % passes) * kPrPass;
  const int nc = M - m0 < kPrPass ? M - m0 : kPrPass;
  const float* __restrict__ Q = recs + queries[q].q_rec * kPlRecWords;  // the same address in every lane: scalar loads
  if (tid < kPrPass) {
    const unsigned long long key = tid < nc ? shortlist[(long long)q * M + m0 + tid] : kNoKey;
    int dk, slot, id;
    unpack_team_key(key, &dk, &slot, &id);
    crec[tid] = key == kNoKey ? -1ll : (long long)slot * max_frames + id;
    cbest[tid] = kNoKey;
  }
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    if (crec[c] < 0) continue;  // (uniform)
    const float4* src = (const float4*)(recs + crec[c] * kPlRecWords);
    float4* dst = (float4*)&cu[c][0];
    for (int i = tid; i < kPlRecWords / 4; i += kPrBlock) dst[i] = src[i];
  }
  __syncthreads();
  const int ci = tid / kPrLanes, k0 = (tid % kPrLanes) * kPrShifts;
  if (ci < nc && crec[ci] >= 0) {
    const float* C = cu[ci];
    float W[kPrShifts][kNR], sim[kPrShifts];
#pragma unroll
    for (int i = 0; i < kPrShifts; ++i) sim[i] = 0.f, load_column(W[i], C + (k0 + i) * kNR);
    for (int jj = 0; jj < kNS; jj += kPrShifts) {
#pragma unroll
      for (int u = 0; u < kPrShifts; ++u) {  // query column j = jj + u; candidate column j + k0 + i lies in W[(u + i) % 5]
        float qc[kNR];
        load_column(qc, Q + (jj + u) * kNR);
#pragma unroll
        for (int i = 0; i < kPrShifts; ++i) {
          const float* w = W[(u + i) % kPrShifts];
          float d = 0.f;
#pragma unroll
          for (int r = 0; r < kNR; ++r) d = fmaf(qc[r], w[r], d);
          sim[i] += d;
        }
        int col = jj + u + kPrShifts + k0;  // < 2 kNS
        col -= col >= kNS ? kNS : 0;
        load_column(W[u], C + col * kNR);
      }
    }
    const unsigned long long all = (1ull << kNS) - 1ull, vq = mask_of(Q), vc = mask_of(C);
    unsigned long long best = kNoKey;
#pragma unroll
    for (int i = 0; i < kPrShifts; ++i) {
      const int k = k0 + i;
      const unsigned long long rc = ((vc >> k) | (vc << (kNS - k))) & all;  // bit j: the candidate's column (j + k) % kNS
      const unsigned long long key = pack_key(distance_of(sim[i], __popcll(vq & rc)), m0 + ci, k);
      best = key < best ? key : best;
    }
    atomicMin(&cbest[ci], best);
  }
  __syncthreads();
  if (tid < nc) row[(long long)q * M + m0 + tid] = cbest[tid];
}

}  // namespace

void launch_team_keys(hipStream_t s, int n, const TmStale* stale, const float* D, uint4* keys) {
  const int per = kTmBlock / 64;
  if (n > 0) hipLaunchKernelGGL(team_key_kernel, dim3((n + per - 1) / per), dim3(kTmBlock), 0, s, n, stale, D, keys);
}

void launch_team_shortlist(hipStream_t s, int n_queries, const TmQuery* queries, int n_targets, const TmTarget* targets, long long total, int chunk,
                           int n_chunks, int M, const uint4* keys, unsigned long long* lists, unsigned long long* shortlist) {
  if (n_queries <= 0) return;
  if (n_chunks > 0)
    hipLaunchKernelGGL(team_shortlist_kernel, dim3(n_queries * n_chunks), dim3(kTmBlock), 0, s, queries, targets, n_targets, total, chunk, n_chunks, M,
                       keys, lists);
  hipLaunchKernelGGL(team_merge_kernel, dim3(n_queries), dim3(kTmBlock), 0, s, n_chunks, M, lists, shortlist);
}

void launch_team_pairs(hipStream_t s, int n_queries, const TmQuery* queries, int M, int max_frames, const unsigned long long* shortlist,
                       const float* recs, unsigned long long* row) {
  const int passes = (M + kPrPass - 1) / kPrPass;
  if (n_queries > 0)
    hipLaunchKernelGGL(team_pair_kernel, dim3(n_queries * passes), dim3(kPrBlock), 0, s, queries, M, passes, max_frames, shortlist, recs, row);
}

}  // namespace lins
