// place_kernels.hip — place recognition on the device (include/lins_place.h; the contract is host/place_math.h +
// host/place.cpp, bit for bit; the records are place.h).
//   build    one workgroup per stale frame, reading the frame's block in the archive's arena where it lies.  The cell
//            maxima form in LDS: a counted height is positive, so its bits order as integers and an LDS integer max is
//            the f32 max, in any order.  Then one lane per column: the norm's fmaf chain, the division, the valid bit.
//   search   one workgroup per (entry, chunk of candidates).  The candidates' normalised columns stream through LDS, ten
//            at a time; twelve lanes serve a candidate, five consecutive shifts each.  A lane walks the query's columns in
//            order — the order of the contract's sum — and keeps the five candidate columns its shifts need in
//            registers: the next query column needs one new candidate column (five 16-byte LDS reads) for 100 fused
//            multiply-adds.  The query's own columns never enter LDS: their address is the same in every lane, so they
//            come by scalar loads and feed the multiply-adds as SGPR operands.  A lane group's column reads start 25
//            sixteen-byte slots apart — 9 modulo the 16 slots of a bank row, distinct for twelve lanes — so the layout
//            needs no padding.  An invalid column is stored as zeros: its dot is exactly +0, which
//            leaves the sum's bits alone; the count of valid pairs is a population count of the two columns' valid bits.
//   reduce   a chunk's best is the minimum of the packed keys (bits(d) << 32) | (id << 6) | shift, d clamped at 0 so its
//            bits are monotone; one workgroup per entry takes the minimum of its chunks' bests.  A minimum depends neither
//            on order nor on the split.  Plain vector stores, no global atomics.
// No MFMA: v_mfma_f32_*f32 would give the k-ordered fmaf chain, but the contract's sum over the columns is a plain add.
#include <hip/hip_runtime.h>

#include "host/place_math.h"
#include "lins_launch.h"
#include "place.h"

namespace lins {
namespace {

using namespace lins_place;

constexpr int kPlBlock = 128;                   // threads of the search
constexpr int kPlShifts = 5;                    // shifts per lane
constexpr int kPlLanes = kNS / kPlShifts;       // lanes per candidate
constexpr int kPlPass = kPlBlock / kPlLanes;    // candidates in LDS at a time
static_assert(kPlLanes * kPlShifts == kNS && kPlPass * kPlLanes <= kPlBlock, "search shape");
static_assert(kNR % 4 == 0 && (kPlRecWords * 4) % 16 == 0, "16-byte column reads");

__global__ __launch_bounds__(kPlBuildBlock) void place_build_kernel(const PlStale* __restrict__ stale, const float4* __restrict__ arena, PlParams prm,
                                                                    float* __restrict__ Dout, float* __restrict__ recs) {
  __shared__ unsigned cells[kCells];
  __shared__ unsigned long long valid;
  const int tid = threadIdx.x;
  const PlStale f = stale[blockIdx.x];
  for (int i = tid; i < kCells; i += kPlBuildBlock) cells[i] = 0u;
  if (tid == 0) valid = 0ull;
  __syncthreads();
  long long off = f.src;
  for (int q = 0; q < 3; ++q) {
    if (prm.clouds & (1 << q)) {
      for (int i = tid; i < f.n[q]; i += kPlBuildBlock) {
        const float4 p = arena[off + i];
        const float pu = prm.up == 0 ? p.x : prm.up == 1 ? p.y : p.z;
        const float pa = prm.up == 0 ? p.y : prm.up == 1 ? p.z : p.x;
        const float pb = prm.up == 0 ? p.z : prm.up == 1 ? p.x : p.y;
        float h;
        const int cell = cell_of(pu, pa, pb, prm.r_max, prm.lift, prm.inv_r, &h);
        if (cell >= 0) atomicMax(&cells[cell], __float_as_uint(h));
      }
    }
    off += f.n[q];
  }
  __syncthreads();
  const float* D = (const float*)cells;
  float* out = Dout + f.dst * kCells;
  for (int i = tid; i < kCells; i += kPlBuildBlock) out[i] = D[i];
  float* rec = recs + f.dst * kPlRecWords;
  if (tid < kNS) {
    float u[kNR];
    const float norm = column(D, tid, u);
    for (int r = 0; r < kNR; ++r) rec[tid * kNR + r] = u[r];
    if (norm > 0.f) atomicOr(&valid, 1ull << tid);
  }
  __syncthreads();
  if (tid == 0) {
    unsigned* w = (unsigned*)rec;
    w[kPlMaskWord] = (unsigned)valid, w[kPlMaskWord + 1] = (unsigned)(valid >> 32);
    const unsigned long long t = (unsigned long long)__double_as_longlong(f.time);
    w[kPlTimeWord] = (unsigned)t, w[kPlTimeWord + 1] = (unsigned)(t >> 32);
  }
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

__global__ __launch_bounds__(kPlBlock) void place_search_kernel(const PlEntry* __restrict__ entries, const int2* __restrict__ chunks, int chunk,
                                                                const float* __restrict__ recs, unsigned long long* __restrict__ chunk_best,
                                                                unsigned long long* __restrict__ row) {
  __shared__ __attribute__((aligned(16))) float cu[kPlPass][kPlRecWords];
  __shared__ unsigned long long cbest[kPlPass];
  __shared__ unsigned long long wbest;
  const int tid = threadIdx.x;
  const int2 ch = chunks[blockIdx.x];  // (entry, first candidate)
  const PlEntry e = entries[ch.x];
  const int c_end = ch.y + chunk < e.nf ? ch.y + chunk : e.nf;
  const float* __restrict__ Q = recs + e.q_rec * kPlRecWords;  // the same address in every lane: scalar loads, the columns live in SGPRs
  if (tid == 0) wbest = kNoKey;
  const int ci = tid / kPlLanes, k0 = (tid % kPlLanes) * kPlShifts;
  for (int c0 = ch.y; c0 < c_end; c0 += kPlPass) {
    const int nc = c_end - c0 < kPlPass ? c_end - c0 : kPlPass;
    __syncthreads();  // (the previous pass's readers are done with cu and cbest)
    {
      const float4* src = (const float4*)(recs + (e.base + c0) * kPlRecWords);
      float4* dst = (float4*)&cu[0][0];
      for (int i = tid; i < nc * (kPlRecWords / 4); i += kPlBlock) dst[i] = src[i];
    }
    if (tid < kPlPass) cbest[tid] = kNoKey;
    __syncthreads();
    if (ci < nc) {
      const float* C = cu[ci];
      const int id = c0 + ci;
      double time_c;
      __builtin_memcpy(&time_c, C + kPlTimeWord, 8);
      if (id != e.skip && time_admits(time_c, e.now, e.gap)) {
        float W[kPlShifts][kNR], sim[kPlShifts];
#pragma unroll
        for (int i = 0; i < kPlShifts; ++i) sim[i] = 0.f, load_column(W[i], C + (k0 + i) * kNR);
        for (int jj = 0; jj < kNS; jj += kPlShifts) {
#pragma unroll
          for (int u = 0; u < kPlShifts; ++u) {  // query column j = jj + u; candidate column j + k0 + i lies in W[(u + i) % 5]
            float q[kNR];
            load_column(q, Q + (jj + u) * kNR);
#pragma unroll
            for (int i = 0; i < kPlShifts; ++i) {
              const float* w = W[(u + i) % kPlShifts];
              float d = 0.f;
#pragma unroll
              for (int r = 0; r < kNR; ++r) d = fmaf(q[r], w[r], d);
              sim[i] += d;
            }
            int col = jj + u + kPlShifts + k0;  // < 2 kNS
            col -= col >= kNS ? kNS : 0;
            load_column(W[u], C + col * kNR);
          }
        }
        const unsigned long long all = (1ull << kNS) - 1ull, vq = mask_of(Q), vc = mask_of(C);
        unsigned long long best = kNoKey;
#pragma unroll
        for (int i = 0; i < kPlShifts; ++i) {
          const int k = k0 + i;
          const unsigned long long rc = ((vc >> k) | (vc << (kNS - k))) & all;  // bit j: the candidate's column (j + k) % kNS
          const unsigned long long key = pack_key(distance_of(sim[i], __popcll(vq & rc)), id, k);
          best = key < best ? key : best;
        }
        atomicMin(&cbest[ci], best);
      }
    }
    __syncthreads();
    if (tid < nc) {
      if (row) row[e.row + c0 + tid] = cbest[tid];
      atomicMin(&wbest, cbest[tid]);
    }
  }
  __syncthreads();
  if (tid == 0) chunk_best[blockIdx.x] = wbest;
}

__global__ __launch_bounds__(64) void place_reduce_kernel(const PlEntry* __restrict__ entries, const unsigned long long* __restrict__ chunk_best,
                                                          unsigned long long* __restrict__ out) {
  __shared__ unsigned long long part[64];
  const PlEntry e = entries[blockIdx.x];
  unsigned long long best = kNoKey;
  for (int i = threadIdx.x; i < e.n_chunks; i += 64) {
    const unsigned long long k = chunk_best[e.chunk0 + i];
    best = k < best ? k : best;
  }
  part[threadIdx.x] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 64; ++i) best = part[i] < best ? part[i] : best;
    out[blockIdx.x] = best;
  }
}

// The k best separated candidates of an entry from its row (place_math.h "top-K"): one workgroup per entry, k rounds.  A
// round: each lane takes the minimum of the row keys it strides over whose candidate `separated` still admits — the ids
// chosen so far sit in LDS, the same in every lane —, the wave's minimum comes by shuffles on the key's two 32-bit
// halves, the workgroup's through LDS across the waves; lane 0 publishes the round's winner.  The row is re-read from L2
// every round (at most 64 KB an entry).  A minimum depends on no order: the bits are select_topk's.  Plain vector stores.
__global__ __launch_bounds__(kPlSelectBlock) void place_select_kernel(const PlEntry* __restrict__ entries, const unsigned long long* __restrict__ row, int k,
                                                                      int min_sep, unsigned long long* __restrict__ out) {
  constexpr int kWaves = kPlSelectBlock / 64;
  __shared__ unsigned long long part[kWaves];
  __shared__ unsigned long long winner;
  __shared__ int chosen[kMaxK];
  const int tid = threadIdx.x;
  const PlEntry e = entries[blockIdx.x];
  const unsigned long long* __restrict__ R = row + e.row;
  unsigned long long* __restrict__ O = out + (long long)blockIdx.x * k;
  int j = 0;
  for (; j < k; ++j) {  // (j and the exit are uniform over the workgroup)
    unsigned long long best = kNoKey;
    for (int c = tid; c < e.nf; c += kPlSelectBlock) {
      const unsigned long long key = R[c];
      if (key < best && separated(c, chosen, j, min_sep)) best = key;
    }
    unsigned hi = (unsigned)(best >> 32), lo = (unsigned)best;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned ohi = __shfl_xor(hi, off), olo = __shfl_xor(lo, off);
      const bool less = ohi < hi || (ohi == hi && olo < lo);
      hi = less ? ohi : hi, lo = less ? olo : lo;
    }
    if ((tid & 63) == 0) part[tid >> 6] = ((unsigned long long)hi << 32) | lo;
    __syncthreads();
    if (tid == 0) {
      unsigned long long w = part[0];
      for (int i = 1; i < kWaves; ++i) w = part[i] < w ? part[i] : w;
      winner = w;
      if (w != kNoKey) chosen[j] = (int)((w & 0xffffffffull) >> 6), O[j] = w;
    }
    __syncthreads();  // (winner and chosen[j] are written; part is free for the next round)
    if (winner == kNoKey) break;
  }
  for (int i = j + tid; i < k; i += kPlSelectBlock) O[i] = kNoKey;
}

}  // namespace

void launch_place_select(hipStream_t s, int n_entries, const PlEntry* entries, const unsigned long long* row, int k, int min_sep,
                         unsigned long long* out) {
  if (n_entries > 0) hipLaunchKernelGGL(place_select_kernel, dim3(n_entries), dim3(kPlSelectBlock), 0, s, entries, row, k, min_sep, out);
}

void launch_place_build(hipStream_t s, int n, const PlStale* stale, const float4* arena, const PlParams& prm, float* D, float* recs) {
  if (n > 0) hipLaunchKernelGGL(place_build_kernel, dim3(n), dim3(kPlBuildBlock), 0, s, stale, arena, prm, D, recs);
}

void launch_place_search(hipStream_t s, int n_entries, int n_chunks, const PlEntry* entries, const int2* chunks, int chunk, const float* recs,
                         unsigned long long* chunk_best, unsigned long long* row, unsigned long long* out) {
  if (n_chunks > 0) hipLaunchKernelGGL(place_search_kernel, dim3(n_chunks), dim3(kPlBlock), 0, s, entries, chunks, chunk, recs, chunk_best, row);
  if (n_entries > 0) hipLaunchKernelGGL(place_reduce_kernel, dim3(n_entries), dim3(64), 0, s, entries, chunk_best, out);
}

}  // namespace lins
