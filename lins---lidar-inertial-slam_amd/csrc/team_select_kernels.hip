// team_select_kernels.hip — which key frames of a team of slots a merged local map takes, on the device
// (include/lins_map.h lins_keyposes_team_select_batch).  The contract is host/team_select.h, bit for bit; the scalar pieces
// are keypose_select_math.h (kp_dist2, kp_cell, kp_cells_fit: the statements the one-slot selection uses).  One workgroup
// serves one entry, over the key poses of the entry's targets in the archive's device mirror:
//   candidates  the targets' frames concatenated in ascending slot order; a lane finds the target of its first candidate
//               by bisection over the targets' first places and walks forward from there (team_kernels.hip's shortlist)
//   pass 1      every candidate: the hit count and the min / max of the hits' cells per axis (floor and the product with
//               inv > 0 are monotone, so the min of the cells is the cell of the min); voxel_grid's 2^31-cell rule
//   pass 2      every hit again, into an open-addressing table in LDS keyed by its linear cell index in the box (< 2^31):
//               the place is claimed by a compare-and-swap on the key, the value is a 64-bit atomic min of
//               (bits(d) << 32) | place — d is a finite non-negative float, so its bits order as an unsigned, and a place
//               orders as (slot, id).  Per cell only a minimum is wanted, so the number of HITS is not bounded; only the
//               number of OCCUPIED CELLS is, by kTsCells: above it the entry is flagged and the host text serves it.
//               The table has 2 * kTsCells places and a lane claims at most one per hit after reading the flag clear, so a
//               probe always meets a free place; the probe loop is bounded by the table's size all the same.
//   output      the values compacted in any order (the places are distinct), each place mapped back to (slot << 32) | id by
//               the bisection, a bitonic sort of at most kTsCells words, plain vector stores of the (slot, id) pairs
// A minimum depends on no order and the last step sorts: the bits depend neither on the order the lanes arrive in nor on
// the batch.  LDS atomics only, no global atomics.  Nothing here depends on the wave size: counts, box and table go
// through LDS and workgroup barriers.
#include <hip/hip_runtime.h>

#include "../../include/lins_ieskf.h"
#include "keyframe_archive.h"
#include "keypose_select_math.h"
#include "lins_launch.h"

namespace lins {
namespace {

using namespace lins_kp;

constexpr int kTsBlock = 1024;
constexpr unsigned kTsFree = 0xffffffffu;              // no cell: a linear cell index is below 2^31
constexpr unsigned long long kTsPad = ~0ull;           // sorts behind every value
constexpr unsigned long long kTsSign = 1ull << 63;     // a signed cell as an unsigned that orders alike
constexpr int kTsBits = 13;                             // the table's places: 2^kTsBits
static_assert(kTsSlots == 1 << kTsBits, "ts_hash keeps kTsBits bits");
static_assert((kTsSlots & (kTsSlots - 1)) == 0 && kTsSlots >= kTsCells + kTsBlock + 1, "a probe meets a free place");

// the target of place g: the last one whose first place is <= g (n_targets >= 1)
__device__ inline int ts_target_of(const TsTarget* __restrict__ T, int n_targets, int g) {
  int lo = 0, hi = n_targets - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T[mid].first <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ inline unsigned ts_hash(unsigned cell) { return (cell * 2654435761u) >> (32 - kTsBits); }

// keys[0, p2) ascending, p2 a power of two >= 2 (kp_sort's pattern)
__device__ inline void ts_sort(unsigned long long* keys, int p2) {
  for (int k = 2; k <= p2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (p2 >> 1); t += kTsBlock) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
        const unsigned long long a = keys[i], b = keys[l];
        if ((a > b) == ((i & k) == 0)) keys[i] = b, keys[l] = a;
      }
      __syncthreads();
    }
  }
}

// one entry's record, two 16-byte stores (the records lie 32 bytes apart from a 64-byte boundary)
__device__ inline void ts_put(KpOut* __restrict__ out, int n, int hits, int status, int host) {
  int4* o = (int4*)out;
  o[0] = make_int4(n, hits, status, host);
  o[1] = make_int4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kTsBlock) void team_select_kernel(const TsEntry* __restrict__ entries, const TsTarget* __restrict__ targets,
                                                               const float4* __restrict__ poses, int2* __restrict__ pairs,
                                                               KpOut* __restrict__ out) {
  __shared__ unsigned long long val[kTsSlots];
  __shared__ unsigned long long srt[kTsCells];  // the table's keys (kTsSlots unsigned) in pass 2, the sort's words after it
  __shared__ unsigned long long box[6];         // min, max of the hits' cells per axis (sign-flipped)
  __shared__ int cnt, occ, over, nout;
  unsigned* key = (unsigned*)srt;
  static_assert(sizeof(srt) == kTsSlots * sizeof(unsigned), "the keys lie where the sort's words will");
  const int k = blockIdx.x, tid = threadIdx.x;
  const TsEntry e = entries[k];
  const TsTarget* __restrict__ T = targets + e.t0;
  if (e.host) {  // (uniform over the workgroup, as every return below)
    if (tid == 0) ts_put(out + k, 0, 0, LINS_OK, 1);
    return;
  }
  if (tid == 0) cnt = 0, occ = 0, over = 0, nout = 0;
  if (tid < 3) box[tid] = ~0ull, box[3 + tid] = 0ull;
  for (int i = tid; i < kTsSlots; i += kTsBlock) key[i] = kTsFree, val[i] = kTsPad;
  __syncthreads();
  // ---- pass 1: hits and their cell box ----
  {
    long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, hi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
    int mine = 0;
    if (tid < e.total) {
      int t = ts_target_of(T, e.n_targets, tid);
      for (int g = tid; g < e.total; g += kTsBlock) {
        while (t + 1 < e.n_targets && T[t + 1].first <= g) ++t;
        const float4 p = poses[T[t].base + (g - T[t].first)];  // g - first < the slot's frames: the next target with frames starts there
        const float d = kp_dist2(p.x, p.y, p.z, e.c[0], e.c[1], e.c[2]);
        if (d <= e.r2) {
          ++mine;
          const long long c[3] = {kp_cell(p.x, e.inv), kp_cell(p.y, e.inv), kp_cell(p.z, e.inv)};
#pragma unroll
          for (int a = 0; a < 3; ++a) lo[a] = c[a] < lo[a] ? c[a] : lo[a], hi[a] = c[a] > hi[a] ? c[a] : hi[a];
        }
      }
    }
    if (mine) {
      atomicAdd(&cnt, mine);
#pragma unroll
      for (int a = 0; a < 3; ++a) atomicMin(&box[a], (unsigned long long)lo[a] ^ kTsSign), atomicMax(&box[3 + a], (unsigned long long)hi[a] ^ kTsSign);
    }
  }
  __syncthreads();
  const int hits = cnt;
  long long minb[3] = {0, 0, 0}, div[3] = {1, 1, 1};
  if (hits)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      minb[a] = (long long)(box[a] ^ kTsSign);
      // (max - min of two long long as an unsigned: exact; anything from 2^32 up is refused as too large below)
      const unsigned long long span = (box[3 + a] ^ kTsSign) - (box[a] ^ kTsSign);
      div[a] = span >= (1ull << 32) ? (1ll << 32) : (long long)span + 1;
    }
  if (!kp_cells_fit(div[0], div[1], div[2])) {
    if (tid == 0) ts_put(out + k, 0, hits, LINS_E_CAPACITY, 0);
    return;
  }
  // ---- pass 2: per occupied cell the minimum of (d, place) ----
  if (hits && tid < e.total) {
    int t = ts_target_of(T, e.n_targets, tid);
    for (int g = tid; g < e.total; g += kTsBlock) {
      while (t + 1 < e.n_targets && T[t + 1].first <= g) ++t;
      const float4 p = poses[T[t].base + (g - T[t].first)];
      const float d = kp_dist2(p.x, p.y, p.z, e.c[0], e.c[1], e.c[2]);
      if (!(d <= e.r2)) continue;
      if (*(volatile int*)&over) break;  // (the entry goes to the host: nothing of the table is read)
      const long long ix = kp_cell(p.x, e.inv) - minb[0], iy = kp_cell(p.y, e.inv) - minb[1], iz = kp_cell(p.z, e.inv) - minb[2];
      const unsigned cell = (unsigned)(ix + iy * div[0] + iz * div[0] * div[1]);  // < 2^31
      unsigned h = ts_hash(cell);
      int probes = 0;
      for (; probes < kTsSlots; ++probes, h = (h + 1) & (unsigned)(kTsSlots - 1)) {
        const unsigned was = atomicCAS(&key[h], kTsFree, cell);
        if (was == kTsFree && atomicAdd(&occ, 1) >= kTsCells) over = 1;
        if (was == kTsFree || was == cell) break;
      }
      if (probes == kTsSlots) {
        over = 1;
        break;
      }
      atomicMin(&val[h], ((unsigned long long)kp_float_bits(d) << 32) | (unsigned)g);
    }
  }
  __syncthreads();
  if (over) {
    if (tid == 0) ts_put(out + k, 0, hits, LINS_OK, 1);
    return;
  }
  const int nsel = occ;  // <= kTsCells
  if (nsel > e.stride) {
    if (tid == 0) ts_put(out + k, 0, hits, LINS_E_CAPACITY, 0);
    return;
  }
  // ---- output: the survivors as (slot << 32) | id, sorted ----
  // (the barrier above: every lane is done with the keys; the words the sort reads are all written below)
  int p2 = 2;
  while (p2 < nsel) p2 <<= 1;
  unsigned long long w[kTsSlots / kTsBlock];
#pragma unroll
  for (int j = 0; j < kTsSlots / kTsBlock; ++j) w[j] = val[tid + j * kTsBlock];
  __syncthreads();
  for (int r = nsel + tid; r < p2; r += kTsBlock) srt[r] = kTsPad;
#pragma unroll
  for (int j = 0; j < kTsSlots / kTsBlock; ++j)
    if (w[j] != kTsPad) {
      const int g = (int)(unsigned)w[j];
      const int t = ts_target_of(T, e.n_targets, g);
      srt[atomicAdd(&nout, 1)] = ((unsigned long long)(unsigned)T[t].slot << 32) | (unsigned)(g - T[t].first);
    }
  __syncthreads();
  ts_sort(srt, p2);
  int2* dst = pairs + (long long)k * e.stride;
  for (int r = tid; r < nsel; r += kTsBlock) dst[r] = make_int2((int)(srt[r] >> 32), (int)(unsigned)srt[r]);
  if (tid == 0) ts_put(out + k, nsel, hits, LINS_OK, 0);
}

}  // namespace

void launch_team_select(hipStream_t s, int n, const TsEntry* entries, const TsTarget* targets, const float4* poses, int2* pairs, KpOut* out) {
  if (n > 0) hipLaunchKernelGGL(team_select_kernel, dim3(n), dim3(kTsBlock), 0, s, entries, targets, poses, pairs, out);
}

}  // namespace lins
