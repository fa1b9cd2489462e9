// archive_kernels.hip — the key-frame archive's assembly on the device (include/lins_map.h lins_archive_assemble;
// LM:984-1031, 1043-1112).  An assembly is the local-map build's VoxelGrid (local_map_kernels.hip: setup, keys, hist,
// scatter, heads, starts, sum — its arithmetic contract is not restated here) around three pieces of its own:
//   gather      the chosen clouds of the chosen frames out of the archive arena into the map frame (the point arithmetic
//               of lm_transform_kernel); the f32 box is folded wave -> LDS -> ONE set of six atomics per workgroup (min /
//               max of the order-preserving encoding: the result does not depend on the order)
//   scan        a large job's (256 digits x tiles) histogram and its per-tile counts scanned over many workgroups:
//               chunk sums -> scan of the chunk sums -> each chunk re-scanned from its offset (keyframe_archive.h).
//               Integer sums: the same bits as the one-workgroup scan, whatever the chunk
//   compaction  leaf == 0: per-tile keep counts -> the same scan -> stable scatter in input order
// Every kernel takes all jobs of a call in one launch, over a (job, tile) or a (job, chunk) table.
// The arena itself is compacted when slots are released (include/lins_lifecycle.h): ar_reclaim_gather / _scatter / _move
// at the end of this file run the passes of the plan of host/arena_reclaim.h over a (segment, tile) table.
#include <hip/hip_runtime.h>

#include "../../include/lins_ieskf.h"
#include "keyframe_archive.h"
#include "lins_launch.h"
#include "local_map.h"

namespace lins {
namespace {

constexpr int kWaves = kLmTile / 64;

__device__ inline unsigned long long lane_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// exclusive prefix of v over the workgroup in thread order, the workgroup's sum in *total (wsum: kWaves ints of LDS;
// every thread of the workgroup calls it, the same number of times)
__device__ inline int block_excl(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o);
    if (lane >= o) inc += u;
  }
  __syncthreads();  // (the readers of the previous call are done with wsum)
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kWaves; ++w) {
    const int c = wsum[w];
    all += c;
    if (w < wave) before += c;
  }
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kLmTile) void ar_gather_kernel(const LmSeg* __restrict__ segs, const int2* __restrict__ blocks,
                                                            const float4* __restrict__ arena, float4* __restrict__ stage,
                                                            LmState* __restrict__ states) {
  const int2 b = blocks[blockIdx.x];
  const LmSeg& s = segs[b.x];
  const int i = b.y * kLmTile + threadIdx.x;
  const bool valid = i < s.n;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) {
    const float4 p = arena[s.src + i];
    const float* t = s.t;  // ctRoll, stRoll, ctPitch, stPitch, ctYaw, stYaw, tInX, tInY, tInZ
    const float x1 = t[4] * p.x - t[5] * p.y;
    const float y1 = t[5] * p.x + t[4] * p.y;
    const float z1 = p.z;
    const float x2 = x1;
    const float y2 = t[0] * y1 - t[1] * z1;
    const float z2 = t[1] * y1 + t[0] * z1;
    q = make_float4(t[2] * x2 + t[3] * z2 + t[6], y2 + t[7], -t[3] * x2 + t[2] * z2 + t[8], p.w);
    stage[s.dst + i] = q;
    const bool ok = fabsf(q.x) <= 1e6f && fabsf(q.y) <= 1e6f && fabsf(q.z) <= 1e6f;  // (false for NaN)
    if (!ok) atomicOr(&states[s.job].flags, 1);
  }
  // the box: wave -> LDS -> one set of six atomics per workgroup
  __shared__ float wbox[kWaves][6];
  float v[6] = {valid ? q.x : INFINITY, valid ? q.y : INFINITY, valid ? q.z : INFINITY,
                valid ? q.x : -INFINITY, valid ? q.y : -INFINITY, valid ? q.z : -INFINITY};
  for (int o = 32; o; o >>= 1)
    for (int a = 0; a < 3; ++a) v[a] = fminf(v[a], __shfl_xor(v[a], o)), v[3 + a] = fmaxf(v[3 + a], __shfl_xor(v[3 + a], o));
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 6; ++a) wbox[threadIdx.x >> 6][a] = v[a];
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY, x_lo = INFINITY, x_hi = -INFINITY;
    for (int w = 0; w < kWaves; ++w) {
      lo = fminf(lo, wbox[w][a]), hi = fmaxf(hi, wbox[w][3 + a]);
      x_lo = fminf(x_lo, wbox[w][0]), x_hi = fmaxf(x_hi, wbox[w][3]);
    }
    if (x_lo <= x_hi) {
      LmState* st = &states[s.job];
      atomicMin(&st->mn[a], lm_enc(lo)), atomicMax(&st->mx[a], lm_enc(hi));
    }
  }
}

// the digit-major row of a job's counts: element e of [0, m) lies at base[(e / nt) * stride + e % nt]
struct ArRow {
  int* base;
  long long m;
  int nt, stride;
};
__device__ inline ArRow row_of(int rows, const LmJob& jb, const LmState& st, int* data) {
  ArRow r;
  r.nt = (st.n + kLmTile - 1) / kLmTile, r.stride = jb.ntiles;
  r.m = (long long)rows * r.nt, r.base = data + (long long)jb.tile0 * rows;
  return r;
}
__device__ inline int* row_at(const ArRow& r, long long e) { return r.base + (e / r.nt) * r.stride + e % r.nt; }

__global__ __launch_bounds__(kLmTile) void ar_chunk_sum_kernel(int rows, int pass, int chunk, const ArChunk* __restrict__ chunks,
                                                               const LmJob* __restrict__ jobs, const LmState* __restrict__ states,
                                                               int* __restrict__ data, int* __restrict__ csum) {
  const ArChunk ck = chunks[blockIdx.x];
  const LmState& st = states[ck.job];
  if (pass >= 0 && pass >= st.passes) return;
  const ArRow r = row_of(rows, jobs[ck.job], st, data);
  const long long span = (long long)rows * chunk;
  const long long lo = ck.k * span < r.m ? ck.k * span : r.m, hi = lo + span < r.m ? lo + span : r.m;
  int local = 0;
  for (long long e = lo + threadIdx.x; e < hi; e += kLmTile) local += *row_at(r, e);
  for (int o = 32; o; o >>= 1) local += __shfl_xor(local, o);
  __shared__ int wsum[kWaves];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < kWaves; ++w) c += wsum[w];
    csum[ck.c0 + ck.k] = c;
  }
}

__global__ __launch_bounds__(kLmTile) void ar_chunk_scan_kernel(int pass, int write_total, const ArSplit* __restrict__ splits,
                                                                LmState* __restrict__ states, int* __restrict__ csum) {
  const ArSplit sp = splits[blockIdx.x];
  LmState& st = states[sp.job];
  if (pass >= 0 && pass >= st.passes) return;
  __shared__ int wsum[kWaves];
  int run = 0;
  for (int b = 0; b < sp.nc; b += kLmTile) {
    const int i = b + threadIdx.x;
    const int v = i < sp.nc ? csum[sp.c0 + i] : 0;
    int total;
    const int ex = block_excl(v, wsum, &total);
    if (i < sp.nc) csum[sp.c0 + i] = run + ex;
    run += total;
  }
  if (write_total && threadIdx.x == 0) st.nvox = run;
}

__global__ __launch_bounds__(kLmTile) void ar_chunk_apply_kernel(int rows, int pass, int chunk, const ArChunk* __restrict__ chunks,
                                                                 const LmJob* __restrict__ jobs, const LmState* __restrict__ states,
                                                                 int* __restrict__ data, const int* __restrict__ csum) {
  const ArChunk ck = chunks[blockIdx.x];
  const LmState& st = states[ck.job];
  if (pass >= 0 && pass >= st.passes) return;
  const ArRow r = row_of(rows, jobs[ck.job], st, data);
  const long long span = (long long)rows * chunk;
  const long long lo = ck.k * span < r.m ? ck.k * span : r.m, hi = lo + span < r.m ? lo + span : r.m;
  __shared__ int wsum[kWaves];
  int run = csum[ck.c0 + ck.k];
  for (long long b = lo; b < hi; b += kLmTile) {  // (lo, hi are the workgroup's: every thread makes the same rounds)
    const long long e = b + threadIdx.x;
    int* p = e < hi ? row_at(r, e) : nullptr;
    const int v = p ? *p : 0;
    int total;
    const int ex = block_excl(v, wsum, &total);
    if (p) *p = run + ex;
    run += total;
  }
}

// (int)intensity >= 0 as x86 evaluates the cast for every float (host/voxel_map.h keeps_nonnegative)
__device__ inline bool keeps(int jflag, float w) { return !(jflag & 1) || (w > -1.0f && w < 2147483648.0f); }

__global__ void ar_keep_setup_kernel(int j0, int n_jobs, LmState* __restrict__ states) {
  const int j = j0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= j0 + n_jobs) return;
  LmState& st = states[j];
  st.passes = 0, st.nvox = 0;
  if (st.flags & 1) st.status = LINS_E_INPUT, st.n = 0;
}

__global__ __launch_bounds__(kLmTile) void ar_keep_kernel(const int2* __restrict__ tiles, const LmJob* __restrict__ jobs,
                                                          const LmState* __restrict__ states, const int* __restrict__ jflags,
                                                          const float4* __restrict__ stage, int* __restrict__ tilecnt) {
  const int2 tl = tiles[blockIdx.x];
  const LmJob& jb = jobs[tl.x];
  const LmState& st = states[tl.x];
  if (tl.y * kLmTile >= st.n) return;
  const int i = tl.y * kLmTile + threadIdx.x;
  const bool keep = i < st.n && keeps(jflags[tl.x], stage[jb.off_in + i].w);
  __shared__ int wc[kWaves];
  const unsigned long long kb = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(kb);
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < kWaves; ++w) c += wc[w];
    tilecnt[jb.tile0 + tl.y] = c;
  }
}

__global__ __launch_bounds__(kLmTile) void ar_compact_kernel(const int2* __restrict__ tiles, const LmJob* __restrict__ jobs,
                                                             const LmState* __restrict__ states, const int* __restrict__ jflags,
                                                             const float4* __restrict__ stage, const int* __restrict__ tilecnt,
                                                             float4* __restrict__ out) {
  const int2 tl = tiles[blockIdx.x];
  const LmJob& jb = jobs[tl.x];
  const LmState& st = states[tl.x];
  if (tl.y * kLmTile >= st.n) return;
  const int i = tl.y * kLmTile + threadIdx.x;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < st.n) p = stage[jb.off_in + i];
  const bool keep = i < st.n && keeps(jflags[tl.x], p.w);
  __shared__ int wc[kWaves];
  const unsigned long long kb = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(kb);
  __syncthreads();
  if (!keep) return;
  int before = tilecnt[jb.tile0 + tl.y];  // (exclusive over the job's tiles by now)
  for (int w = 0; w < (int)threadIdx.x / 64; ++w) before += wc[w];
  out[jb.off_out + before + __popcll(kb & lane_lt())] = p;
}

// ---- the arena's compaction (lins_archive_release_slots): one workgroup per (segment, tile) entry of a pass, one float4
// per lane, one guarded block.  No lane reads what another lane of the same launch writes: gather and scatter have the
// staging buffer on one side, and a pass is moved inside the arena only when its destination range ends at or before
// its first source (host/arena_reclaim.h "direct").
__global__ __launch_bounds__(kLmTile) void ar_reclaim_gather_kernel(const ArMove* __restrict__ segs, const int2* __restrict__ blocks,
                                                                    const float4* __restrict__ arena, float4* __restrict__ stage) {
  const int2 b = blocks[blockIdx.x];
  const ArMove& s = segs[b.x];
  const long long i = (long long)b.y * kLmTile + threadIdx.x;
  if (i < s.n) stage[s.stg + i] = arena[s.src + i];
}

__global__ __launch_bounds__(kLmTile) void ar_reclaim_scatter_kernel(const ArMove* __restrict__ segs, const int2* __restrict__ blocks,
                                                                     const float4* __restrict__ stage, float4* __restrict__ arena) {
  const int2 b = blocks[blockIdx.x];
  const ArMove& s = segs[b.x];
  const long long i = (long long)b.y * kLmTile + threadIdx.x;
  if (i < s.n) arena[s.dst + i] = stage[s.stg + i];
}

__global__ __launch_bounds__(kLmTile) void ar_reclaim_move_kernel(const ArMove* __restrict__ segs, const int2* __restrict__ blocks,
                                                                  float4* arena) {
  const int2 b = blocks[blockIdx.x];
  const ArMove& s = segs[b.x];
  const long long i = (long long)b.y * kLmTile + threadIdx.x;
  if (i < s.n) arena[s.dst + i] = arena[s.src + i];
}

}  // namespace

void launch_ar_reclaim_gather(hipStream_t s, int n_blocks, const ArMove* segs, const int2* blocks, const float4* arena, float4* stage) {
  if (n_blocks) hipLaunchKernelGGL(ar_reclaim_gather_kernel, dim3(n_blocks), dim3(kLmTile), 0, s, segs, blocks, arena, stage);
}

void launch_ar_reclaim_scatter(hipStream_t s, int n_blocks, const ArMove* segs, const int2* blocks, const float4* stage, float4* arena) {
  if (n_blocks) hipLaunchKernelGGL(ar_reclaim_scatter_kernel, dim3(n_blocks), dim3(kLmTile), 0, s, segs, blocks, stage, arena);
}

void launch_ar_reclaim_move(hipStream_t s, int n_blocks, const ArMove* segs, const int2* blocks, float4* arena) {
  if (n_blocks) hipLaunchKernelGGL(ar_reclaim_move_kernel, dim3(n_blocks), dim3(kLmTile), 0, s, segs, blocks, arena);
}

void launch_ar_gather(hipStream_t s, int n_blocks, const LmSeg* segs, const int2* blocks, const float4* arena, float4* stage, LmState* states) {
  if (n_blocks) hipLaunchKernelGGL(ar_gather_kernel, dim3(n_blocks), dim3(kLmTile), 0, s, segs, blocks, arena, stage, states);
}

void launch_ar_scan(hipStream_t s, int rows, int pass, int chunk_tiles, int n_chunks, const ArChunk* chunks, int n_splits, const ArSplit* splits,
                    const LmJob* jobs, LmState* states, int* data, int* csum) {
  if (!n_chunks || !n_splits) return;
  hipLaunchKernelGGL(ar_chunk_sum_kernel, dim3(n_chunks), dim3(kLmTile), 0, s, rows, pass, chunk_tiles, chunks, jobs, states, data, csum);
  hipLaunchKernelGGL(ar_chunk_scan_kernel, dim3(n_splits), dim3(kLmTile), 0, s, pass, rows == 1 ? 1 : 0, splits, states, csum);
  hipLaunchKernelGGL(ar_chunk_apply_kernel, dim3(n_chunks), dim3(kLmTile), 0, s, rows, pass, chunk_tiles, chunks, jobs, states, data, csum);
}

void launch_ar_keep(hipStream_t s, int j0, int n_jobs, int n_tiles, const int2* tiles, const LmJob* jobs, LmState* states, const int* jflags,
                    const float4* stage, int* tilecnt) {
  if (!n_jobs) return;
  hipLaunchKernelGGL(ar_keep_setup_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, s, j0, n_jobs, states);
  if (n_tiles) hipLaunchKernelGGL(ar_keep_kernel, dim3(n_tiles), dim3(kLmTile), 0, s, tiles, jobs, states, jflags, stage, tilecnt);
}

void launch_ar_compact(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const int* jflags, const float4* stage,
                       const int* tilecnt, float4* out) {
  if (n_tiles) hipLaunchKernelGGL(ar_compact_kernel, dim3(n_tiles), dim3(kLmTile), 0, s, tiles, jobs, states, jflags, stage, tilecnt, out);
}

}  // namespace lins
