// keypose_select_kernels.hip — which key frames a global map, a surrounding map or a loop closure takes, on the device
// (include/lins_map.h lins_keyposes_*; LM:989-1007, 1050-1067, 1247-1308).  The contract is host/keyframe_select.h +
// host/voxel_map.h voxel_grid, bit for bit; the scalar pieces are keypose_select_math.h.  One workgroup serves one entry,
// over the slot's key poses in the archive's device mirror:
//   hits        every frame with d <= r2 becomes the packed key (bits(d) << 32) | id in LDS, in any order (the keys are
//               distinct); more than kSortCap hits: the entry is flagged and the host text serves it
//   order       a bitonic sort of the keys: ascending (d, id)
//   pose grid   the cell box is the min / max of the hits' cells (floor and the product with inv > 0 are monotone, so the
//               min of the cells is the cell of the min); voxel_grid's 2^31-cell rule; a second sort of (cell << 32) | rank
//               groups the hits by cell, stably; the lane that holds a cell's first hit walks the run and forms the f32
//               sum of (float)id sequentially in hit order; (int)(sum / (float)count) goes out in ascending cell order
//   list rule   kp_surround_list in parallel: atomic-min marks of the selection's first positions, the survivors compacted
//               in order by a prefix scan, their ids marked -1, the first occurrences that are no survivor compacted behind
// Nothing here depends on the wave size: the scan and the sorts go through LDS and workgroup barriers only.
#include <hip/hip_runtime.h>

#include "../../include/lins_ieskf.h"
#include "keyframe_archive.h"
#include "keypose_select_math.h"
#include "lins_launch.h"

namespace lins {
namespace {

using namespace lins_kp;

constexpr int kKpBlock = 1024;
constexpr int kKpLoopBlock = 256;
constexpr unsigned long long kKpPad = ~0ull;              // sorts behind every key
constexpr unsigned long long kKpSign = 1ull << 63;        // a signed cell as an unsigned that orders alike

// exclusive prefix of v over the workgroup in thread order, the workgroup's sum in *total (part: kKpBlock ints of LDS;
// every thread of the workgroup calls it, the same number of times)
__device__ inline int kp_block_excl(int v, int* part, int* total) {
  const int t = threadIdx.x;
  __syncthreads();  // (the readers of the previous call are done with part)
  part[t] = v;
  __syncthreads();
  for (int o = 1; o < kKpBlock; o <<= 1) {
    const int u = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += u;
    __syncthreads();
  }
  *total = part[kKpBlock - 1];
  return part[t] - v;
}

// keys[0, p2) ascending, p2 a power of two >= 2
__device__ inline void kp_sort(unsigned long long* keys, int p2) {
  for (int k = 2; k <= p2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (p2 >> 1); t += kKpBlock) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
        const unsigned long long a = keys[i], b = keys[l];
        if ((a > b) == ((i & k) == 0)) keys[i] = b, keys[l] = a;
      }
      __syncthreads();
    }
  }
}

template <bool kSurround>
__global__ __launch_bounds__(kKpBlock) void kp_select_kernel(const KpEntry* __restrict__ entries, const float4* __restrict__ poses, int* __restrict__ ids,
                                                             const int* __restrict__ list_in, int* __restrict__ list_out, int* scratch,
                                                             KpOut* __restrict__ out) {
  __shared__ unsigned long long keys[kSortCap];
  __shared__ int idr[kSortCap];  // the id of the hit of rank r
  __shared__ int part[kKpBlock];
  __shared__ unsigned long long box[6];  // min, max of the hits' cells per axis (sign-flipped)
  __shared__ int cnt, bad;
  const int k = blockIdx.x, tid = threadIdx.x;
  const KpEntry e = entries[k];
  const float4* P = poses + e.base;
  if (tid == 0) cnt = 0, bad = 0;
  if (tid < 3) box[tid] = ~0ull, box[3 + tid] = 0ull;
  __syncthreads();
  for (int i = tid; i < e.nf; i += kKpBlock) {
    const float4 p = P[i];
    const float d = kp_dist2(p.x, p.y, p.z, e.c[0], e.c[1], e.c[2]);
    if (d <= e.r2) {
      const int at = atomicAdd(&cnt, 1);
      if (at < kSortCap) keys[at] = kp_key(d, i);
    }
  }
  __syncthreads();
  const int hits = cnt;
  KpOut o{};
  o.hits = hits;
  if (hits > kSortCap) {  // (uniform over the workgroup, as every return below)
    o.host = 1;
    if (tid == 0) out[k] = o;
    return;
  }
  int p2 = 2;
  while (p2 < hits) p2 <<= 1;
  for (int r = hits + tid; r < p2; r += kKpBlock) keys[r] = kKpPad;
  __syncthreads();
  kp_sort(keys, p2);
  // the cell box; idr
  {
    long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, hi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
    for (int r = tid; r < hits; r += kKpBlock) {
      const int id = kp_key_id(keys[r]);
      idr[r] = id;
      const float4 p = P[id];
      const long long c[3] = {kp_cell(p.x, e.inv), kp_cell(p.y, e.inv), kp_cell(p.z, e.inv)};
      for (int a = 0; a < 3; ++a) lo[a] = c[a] < lo[a] ? c[a] : lo[a], hi[a] = c[a] > hi[a] ? c[a] : hi[a];
    }
    if (tid < hits)
      for (int a = 0; a < 3; ++a) atomicMin(&box[a], (unsigned long long)lo[a] ^ kKpSign), atomicMax(&box[3 + a], (unsigned long long)hi[a] ^ kKpSign);
  }
  __syncthreads();
  long long minb[3] = {0, 0, 0}, div[3] = {1, 1, 1};
  if (hits)
    for (int a = 0; a < 3; ++a) {
      minb[a] = (long long)(box[a] ^ kKpSign);
      // (max - min of two long long as an unsigned: exact; anything from 2^32 up is refused as too large below)
      const unsigned long long span = (box[3 + a] ^ kKpSign) - (box[a] ^ kKpSign);
      div[a] = span >= (1ull << 32) ? (1ll << 32) : (long long)span + 1;
    }
  if (!kp_cells_fit(div[0], div[1], div[2])) {
    o.status = LINS_E_CAPACITY;
    if (tid == 0) out[k] = o;
    return;
  }
  // group by cell, stably: (cell << 32) | rank
  for (int r = tid; r < hits; r += kKpBlock) {
    const float4 p = P[idr[r]];
    const long long ix = kp_cell(p.x, e.inv) - minb[0], iy = kp_cell(p.y, e.inv) - minb[1], iz = kp_cell(p.z, e.inv) - minb[2];
    const long long cell = ix + iy * div[0] + iz * div[0] * div[1];  // < 2^31
    keys[r] = ((unsigned long long)cell << 32) | (unsigned)r;
  }
  __syncthreads();  // (the pads behind the hits are still in place)
  kp_sort(keys, p2);
  // one output per cell, in ascending cell order
  const int per = (hits + kKpBlock - 1) / kKpBlock, lo = min(tid * per, hits), hi = min(lo + per, hits);
  int heads = 0;
  for (int q = lo; q < hi; ++q) heads += q == 0 || (keys[q] >> 32) != (keys[q - 1] >> 32);
  int nsel;
  int at = kp_block_excl(heads, part, &nsel);
  o.n = nsel;
  int* dst = kSurround ? scratch + e.mark_off + e.nf : ids + (long long)k * e.stride;
  if (!kSurround && nsel > e.stride) {
    o.n = 0, o.status = LINS_E_CAPACITY;
    if (tid == 0) out[k] = o;
    return;
  }
  for (int q = lo; q < hi; ++q) {
    const unsigned cell = (unsigned)(keys[q] >> 32);
    if (q && cell == (unsigned)(keys[q - 1] >> 32)) continue;
    float sum = 0.f;
    int run = 0;
    for (int w = q; w < hits && (unsigned)(keys[w] >> 32) == cell; ++w) sum += (float)idr[(unsigned)keys[w]], ++run;
    const int sel = (int)(sum / (float)run);
    if (kSurround && (sel < 0 || sel >= e.nf)) bad = 1;  // (a rounded mean beyond the slot's frames: no mark to take)
    dst[at++] = sel;
  }
  if (!kSurround) {
    if (tid == 0) out[k] = o;
    return;
  }
  // ---- the list rule (kp_surround_list) ----
  int* mark = scratch + e.mark_off;
  const int* ds = dst;
  const int* lst = list_in + (long long)k * e.stride;
  int* lout = list_out + (long long)k * e.stride;
  for (int i = tid; i < e.nf; i += kKpBlock) mark[i] = kUnmarked;
  __threadfence_block();
  __syncthreads();
  if (bad) {
    o.host = 1;
    if (tid == 0) out[k] = o;
    return;
  }
  for (int i = tid; i < nsel; i += kKpBlock) atomicMin(&mark[ds[i]], i);
  __threadfence_block();
  __syncthreads();
  const int lper = (e.n_list + kKpBlock - 1) / kKpBlock, llo = min(tid * lper, e.n_list), lhi = min(llo + lper, e.n_list);
  int keep = 0;
  for (int j = llo; j < lhi; ++j) keep += mark[lst[j]] != kUnmarked;
  int nsurv;
  at = kp_block_excl(keep, part, &nsurv);  // (its barriers stand between the reads above and the -1 marks below)
  for (int j = llo; j < lhi; ++j) {
    const int id = lst[j];
    if (mark[id] != kUnmarked) lout[at++] = id, mark[id] = -1;  // (-1 is still "marked" to a lane that reads it late)
  }
  __threadfence_block();
  __syncthreads();
  int fresh = 0;
  for (int i = lo; i < min(hi, nsel); ++i) fresh += mark[ds[i]] == i;
  int nnew;
  at = kp_block_excl(fresh, part, &nnew);
  o.n_list = nsurv + nnew;
  if (o.n_list > e.stride) {
    o.n_list = e.n_list, o.status = LINS_E_CAPACITY;
    if (tid == 0) out[k] = o;
    return;
  }
  for (int i = lo; i < min(hi, nsel); ++i)
    if (mark[ds[i]] == i) lout[nsurv + at++] = ds[i];
  if (tid == 0) out[k] = o;
}

__global__ __launch_bounds__(kKpLoopBlock) void kp_find_loop_kernel(const KpEntry* __restrict__ entries, const float4* __restrict__ poses,
                                                                    const double* __restrict__ times, int* __restrict__ closest) {
  __shared__ unsigned long long best;
  const int k = blockIdx.x, tid = threadIdx.x;
  const KpEntry e = entries[k];
  if (tid == 0) best = kKpPad;
  __syncthreads();
  unsigned long long mine = kKpPad;
  for (int i = tid; i < e.nf; i += kKpLoopBlock) {
    const float4 p = poses[e.base + i];
    const float d = kp_dist2(p.x, p.y, p.z, e.c[0], e.c[1], e.c[2]);
    if (d <= e.r2 && fabs(times[e.base + i] - e.now) > e.gap) {
      const unsigned long long key = kp_key(d, i);
      mine = key < mine ? key : mine;
    }
  }
  if (mine != kKpPad) atomicMin(&best, mine);
  __syncthreads();
  if (tid == 0) closest[k] = best == kKpPad ? -1 : kp_key_id(best);
}

__global__ __launch_bounds__(256) void kp_refresh_kernel(int n, const KpStale* __restrict__ stale, float4* __restrict__ poses, double* __restrict__ times) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const KpStale s = stale[i];
  poses[s.dst] = make_float4(s.x, s.y, s.z, 0.f);
  times[s.dst] = s.time;
}

}  // namespace

void launch_kp_refresh(hipStream_t s, int n, const KpStale* stale, float4* poses, double* times) {
  if (n > 0) hipLaunchKernelGGL(kp_refresh_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, stale, poses, times);
}

void launch_kp_select(hipStream_t s, int n, const KpEntry* entries, const float4* poses, int* ids, KpOut* out) {
  if (n > 0) hipLaunchKernelGGL(kp_select_kernel<false>, dim3(n), dim3(kKpBlock), 0, s, entries, poses, ids, nullptr, nullptr, nullptr, out);
}

void launch_kp_surround(hipStream_t s, int n, const KpEntry* entries, const float4* poses, const int* list_in, int* list_out, int* scratch, KpOut* out) {
  if (n > 0) hipLaunchKernelGGL(kp_select_kernel<true>, dim3(n), dim3(kKpBlock), 0, s, entries, poses, nullptr, list_in, list_out, scratch, out);
}

void launch_kp_find_loop(hipStream_t s, int n, const KpEntry* entries, const float4* poses, const double* times, int* closest) {
  if (n > 0) hipLaunchKernelGGL(kp_find_loop_kernel, dim3(n), dim3(kKpLoopBlock), 0, s, entries, poses, times, closest);
}

}  // namespace lins
