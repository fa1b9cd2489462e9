// local_map_kernels.hip — the mapping node's local map and scan downsampling on the device (include/lins_map.h
// lins_local_map_build; LM:1201-1349).  VoxelGrid is a stable sort by PCL's linear voxel index followed by sequential
// sums per run, so the build is:
//   transform   the window's frames into the map frame (f32 as LM:627-650), written to the staging arena; per-job
//               f32 box by atomic min / max on an order-preserving encoding (the result does not depend on the order)
//   setup       per job: voxel box, divisions, 2^31-cell check, the number of 8-bit radix passes
//   keys        32-bit voxel index + point position per point
//   sort        LSD radix, per pass: tile histograms -> per-job exclusive scan over (digit, tile) -> stable scatter
//               (in-tile rank: wave peers by ballots, wave order by an LDS prefix) — stable by construction
//   runs        run heads counted per tile -> per-job scan -> run starts
//   sum         one lane per voxel adds its run sequentially in input order and writes the centroid to its slot
// Every kernel takes a whole stage (all entries of a batch) in one launch: the tile kernels run over a (job, tile)
// table, the scans over jobs.  A job that needs fewer passes, or a tile past a job's count, returns at once.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/lins_ieskf.h"
#include "lins_launch.h"
#include "local_map.h"

namespace lins {
namespace {

constexpr int kWaves = kLmTile / 64;

__device__ inline unsigned long long lane_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// exclusive scan in place over the rows x nt elements base[r * stride + t] (row-major), one workgroup; returns the total
__device__ int block_scan_rows(int* base, int rows, int nt, int stride) {
  __shared__ int part[kLmTile];
  const int tid = threadIdx.x;
  const long long m = (long long)rows * nt;
  const long long per = (m + kLmTile - 1) / kLmTile;
  const long long lo = tid * per < m ? tid * per : m, hi = lo + per < m ? lo + per : m;
  int local = 0;
  for (long long e = lo; e < hi; ++e) local += base[(e / nt) * stride + e % nt];
  part[tid] = local;
  __syncthreads();
  for (int o = 1; o < kLmTile; o <<= 1) {
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - local;
  for (long long e = lo; e < hi; ++e) {
    int* p = base + (e / nt) * stride + e % nt;
    const int c = *p;
    *p = run;
    run += c;
  }
  const int total = part[kLmTile - 1];
  __syncthreads();
  return total;
}

__device__ inline void fold_box(LmState* st, float x, float y, float z, bool valid) {
  float v[6] = {valid ? x : INFINITY, valid ? y : INFINITY, valid ? z : INFINITY,
                valid ? x : -INFINITY, valid ? y : -INFINITY, valid ? z : -INFINITY};
  for (int o = 32; o; o >>= 1)
    for (int a = 0; a < 3; ++a) v[a] = fminf(v[a], __shfl_xor(v[a], o)), v[3 + a] = fmaxf(v[3 + a], __shfl_xor(v[3 + a], o));
  if ((threadIdx.x & 63) == 0 && v[0] <= v[3])
    for (int a = 0; a < 3; ++a) atomicMin(&st->mn[a], lm_enc(v[a])), atomicMax(&st->mx[a], lm_enc(v[3 + a]));
}

__global__ __launch_bounds__(kLmTile) void lm_transform_kernel(const LmSeg* __restrict__ segs, const int2* __restrict__ blocks,
                                                               const float4* __restrict__ frames, float4* __restrict__ stage,
                                                               LmState* __restrict__ states) {
  const int2 b = blocks[blockIdx.x];
  const LmSeg& s = segs[b.x];
  const int i = b.y * kLmTile + threadIdx.x;
  const bool valid = i < s.n;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) {
    const float4 p = frames[s.src + i];
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
  fold_box(&states[s.job], q.x, q.y, q.z, valid);
}

// The scan clouds of lins_local_map_build_streams: what lins_local_map_build's host pass does to the clouds it is handed —
// the input contract, the f32 box, the packing into the staging arena — for clouds that lie in the streams' arenas in
// the sensor's axes.  The box is folded wave -> LDS -> one set of six atomics per workgroup (archive_kernels.hip's
// gather): min / max of the order-preserving encoding, the bits the host's fold leaves.
__global__ __launch_bounds__(kLmTile) void lm_stage_scans_kernel(const LmScanSeg* __restrict__ segs, const int2* __restrict__ blocks,
                                                                 float4* __restrict__ stage, LmState* __restrict__ states) {
  const int2 b = blocks[blockIdx.x];
  const LmScanSeg s = segs[b.x];
  const int i = b.y * kLmTile + threadIdx.x;
  const bool valid = i < s.n;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  bool bad = false;
  if (valid) {
    const float4 p = s.src[i];
    q = make_float4(p.y, p.z, p.x, p.w);  // the mapping node's axes (SE:1128-1131)
    stage[s.dst + i] = q;
    bad = !(fabsf(q.x) <= 1e6f && fabsf(q.y) <= 1e6f && fabsf(q.z) <= 1e6f);  // (true for NaN and infinities)
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&states[s.job].flags, 1);
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
    float lo = INFINITY, hi = -INFINITY;
    for (int w = 0; w < kWaves; ++w) lo = fminf(lo, wbox[w][a]), hi = fmaxf(hi, wbox[w][3 + a]);
    if (lo <= hi) {  // (a tile of the table holds at least one point)
      LmState* st = &states[s.job];
      atomicMin(&st->mn[a], lm_enc(lo)), atomicMax(&st->mx[a], lm_enc(hi));
    }
  }
}

__global__ void lm_setup_kernel(int j0, int n_jobs, const LmJob* __restrict__ jobs, LmState* __restrict__ states) {
  const int j = j0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= j0 + n_jobs) return;
  const LmJob& jb = jobs[j];
  LmState& st = states[j];
  if (jb.src_a >= 0) {  // stage B: the input is the two stage-A outputs (empty when either failed)
    const LmState &a = states[jb.src_a], &b = states[jb.src_b];
    st.n = (a.status || b.status) ? 0 : a.nvox + b.nvox;
  }
  st.passes = 0, st.nvox = 0;
  if (st.flags & 1) st.status = LINS_E_INPUT;
  if (st.status || st.n == 0) {
    st.n = 0;
    return;
  }
  long long div[3];
  for (int a = 0; a < 3; ++a) {
    st.minb[a] = (int)floorf(lm_dec(st.mn[a]) * jb.inv);
    div[a] = (long long)(int)floorf(lm_dec(st.mx[a]) * jb.inv) - st.minb[a] + 1;
  }
  const long long ncell = div[0] * div[1] * div[2];
  if (div[0] * div[1] > (1ll << 31) || ncell > (1ll << 31)) {  // (each division < 2^25: neither product overflows)
    st.status = LINS_E_CAPACITY, st.n = 0;
    return;
  }
  int bits = 0;
  while ((1ll << bits) < ncell) ++bits;
  st.passes = (bits + kLmDigit - 1) / kLmDigit;
  st.d0 = (unsigned)div[0], st.d01 = (unsigned)(div[0] * div[1]);
}

__global__ __launch_bounds__(kLmTile) void lm_keys_kernel(const int2* __restrict__ tiles, const LmJob* __restrict__ jobs,
                                                          const LmState* __restrict__ states, const float4* __restrict__ stage,
                                                          unsigned* __restrict__ keys, int* __restrict__ vals) {
  const int2 tl = tiles[blockIdx.x];
  const LmJob& jb = jobs[tl.x];
  const LmState& st = states[tl.x];
  const int i = tl.y * kLmTile + threadIdx.x;
  if (i >= st.n) return;
  const float4 p = stage[jb.off_in + i];
  const unsigned ix = (unsigned)((int)floorf(p.x * jb.inv) - st.minb[0]);
  const unsigned iy = (unsigned)((int)floorf(p.y * jb.inv) - st.minb[1]);
  const unsigned iz = (unsigned)((int)floorf(p.z * jb.inv) - st.minb[2]);
  keys[jb.off_in + i] = ix + iy * st.d0 + iz * st.d01;
  vals[jb.off_in + i] = i;
}

__global__ __launch_bounds__(kLmTile) void lm_hist_kernel(int pass, const int2* __restrict__ tiles, const LmJob* __restrict__ jobs,
                                                          const LmState* __restrict__ states, const unsigned* __restrict__ keys,
                                                          int* __restrict__ hist) {
  const int2 tl = tiles[blockIdx.x];
  const LmJob& jb = jobs[tl.x];
  const LmState& st = states[tl.x];
  if (pass >= st.passes || tl.y * kLmTile >= st.n) return;
  __shared__ int h[256];
  if (threadIdx.x < 256) h[threadIdx.x] = 0;
  __syncthreads();
  const int i = tl.y * kLmTile + threadIdx.x;
  if (i < st.n) atomicAdd(&h[(keys[jb.off_in + i] >> (kLmDigit * pass)) & 255u], 1);  // (counts: order does not matter)
  __syncthreads();
  if (threadIdx.x < 256) hist[(long long)jb.tile0 * 256 + (long long)threadIdx.x * jb.ntiles + tl.y] = h[threadIdx.x];
}

__global__ __launch_bounds__(kLmTile) void lm_scan_kernel(int pass, int j0, const LmJob* __restrict__ jobs,
                                                          const LmState* __restrict__ states, int* __restrict__ hist) {
  const LmJob& jb = jobs[j0 + blockIdx.x];
  const LmState& st = states[j0 + blockIdx.x];
  if (pass >= st.passes) return;
  const int nt = (st.n + kLmTile - 1) / kLmTile;
  block_scan_rows(hist + (long long)jb.tile0 * 256, 256, nt, jb.ntiles);
}

__global__ __launch_bounds__(kLmTile) void lm_scatter_kernel(int pass, const int2* __restrict__ tiles, const LmJob* __restrict__ jobs,
                                                             const LmState* __restrict__ states, const int* __restrict__ hist,
                                                             const unsigned* __restrict__ kin, const int* __restrict__ vin,
                                                             unsigned* __restrict__ kout, int* __restrict__ vout) {
  const int2 tl = tiles[blockIdx.x];
  const LmJob& jb = jobs[tl.x];
  const LmState& st = states[tl.x];
  if (pass >= st.passes || tl.y * kLmTile >= st.n) return;
  __shared__ int wcnt[kWaves][256];
  for (int e = threadIdx.x; e < kWaves * 256; e += kLmTile) wcnt[e / 256][e % 256] = 0;
  __syncthreads();
  const int i = tl.y * kLmTile + threadIdx.x, wave = threadIdx.x / 64;
  const bool valid = i < st.n;
  const unsigned key = valid ? kin[jb.off_in + i] : 0u;
  const int val = valid ? vin[jb.off_in + i] : 0;
  const unsigned d = (key >> (kLmDigit * pass)) & 255u;
  unsigned long long peers = __ballot(valid);
  for (int b = 0; b < kLmDigit; ++b) {
    const unsigned long long bb = __ballot((d >> b) & 1u);
    peers &= ((d >> b) & 1u) ? bb : ~bb;
  }
  const int rank = __popcll(peers & lane_lt());
  if (valid && rank == 0) wcnt[wave][d] = __popcll(peers);
  __syncthreads();
  if (threadIdx.x < 256) {  // exclusive prefix over the waves, per digit
    int run = 0;
    for (int w = 0; w < kWaves; ++w) {
      const int c = wcnt[w][threadIdx.x];
      wcnt[w][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
  if (!valid) return;
  const long long pos = jb.off_in + hist[(long long)jb.tile0 * 256 + (long long)d * jb.ntiles + tl.y] + wcnt[wave][d] + rank;
  kout[pos] = key;
  vout[pos] = val;
}

__device__ inline bool is_head(const LmState& st, const unsigned* k, int i) { return i < st.n && (i == 0 || k[i] != k[i - 1]); }

__global__ __launch_bounds__(kLmTile) void lm_heads_kernel(const int2* __restrict__ tiles, const LmJob* __restrict__ jobs,
                                                           const LmState* __restrict__ states, const unsigned* __restrict__ keys_a,
                                                           const unsigned* __restrict__ keys_b, int* __restrict__ tilecnt) {
  const int2 tl = tiles[blockIdx.x];
  const LmJob& jb = jobs[tl.x];
  const LmState& st = states[tl.x];
  if (tl.y * kLmTile >= st.n) return;
  const unsigned* k = ((st.passes & 1) ? keys_b : keys_a) + jb.off_in;
  __shared__ int wc[kWaves];
  const unsigned long long hb = __ballot(is_head(st, k, tl.y * kLmTile + threadIdx.x));
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x / 64] = __popcll(hb);
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < kWaves; ++w) c += wc[w];
    tilecnt[jb.tile0 + tl.y] = c;
  }
}

__global__ __launch_bounds__(kLmTile) void lm_heads_scan_kernel(int j0, const LmJob* __restrict__ jobs, LmState* __restrict__ states,
                                                                int* __restrict__ tilecnt) {
  const LmJob& jb = jobs[j0 + blockIdx.x];
  LmState& st = states[j0 + blockIdx.x];
  if (st.n == 0) return;
  const int total = block_scan_rows(tilecnt + jb.tile0, 1, (st.n + kLmTile - 1) / kLmTile, 0);
  if (threadIdx.x == 0) st.nvox = total;
}

__global__ __launch_bounds__(kLmTile) void lm_starts_kernel(const int2* __restrict__ tiles, const LmJob* __restrict__ jobs,
                                                            const LmState* __restrict__ states, const unsigned* __restrict__ keys_a,
                                                            const unsigned* __restrict__ keys_b, const int* __restrict__ tilecnt,
                                                            int* __restrict__ starts) {
  const int2 tl = tiles[blockIdx.x];
  const LmJob& jb = jobs[tl.x];
  const LmState& st = states[tl.x];
  if (tl.y * kLmTile >= st.n) return;
  const unsigned* k = ((st.passes & 1) ? keys_b : keys_a) + jb.off_in;
  __shared__ int wc[kWaves];
  const int i = tl.y * kLmTile + threadIdx.x;
  const bool head = is_head(st, k, i);
  const unsigned long long hb = __ballot(head);
  if ((threadIdx.x & 63) == 0) wc[threadIdx.x / 64] = __popcll(hb);
  __syncthreads();
  if (!head) return;
  int before = tilecnt[jb.tile0 + tl.y];
  for (int w = 0; w < (int)threadIdx.x / 64; ++w) before += wc[w];
  starts[jb.off_in + before + __popcll(hb & lane_lt())] = i;
}

__global__ __launch_bounds__(kLmTile) void lm_sum_kernel(const int2* __restrict__ tiles, const LmJob* __restrict__ jobs,
                                                         LmState* __restrict__ states, const int* __restrict__ vals_a, const int* __restrict__ vals_b,
                                                         const int* __restrict__ starts, float4* __restrict__ stage,
                                                         float4* __restrict__ out) {
  const int2 tl = tiles[blockIdx.x];
  const LmJob& jb = jobs[tl.x];
  LmState& st = states[tl.x];
  const int v = tl.y * kLmTile + threadIdx.x;
  if (tl.y * kLmTile >= st.nvox) return;
  const bool valid = v < st.nvox;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) {
    const int* vals = ((st.passes & 1) ? vals_b : vals_a) + jb.off_in;
    const float4* src = stage + jb.off_in;
    const int lo = starts[jb.off_in + v], hi = v + 1 < st.nvox ? starts[jb.off_in + v + 1] : st.n;
    float sx = 0.f, sy = 0.f, sz = 0.f, si = 0.f;
    for (int k = lo; k < hi; ++k) {  // the run in input order (the sort is stable), added left to right
      const float4 p = src[vals[k]];
      sx += p.x, sy += p.y, sz += p.z, si += p.w;
    }
    const float c = (float)(hi - lo);
    q = make_float4(sx / c, sy / c, sz / c, si / c);
    out[jb.off_out + (jb.out_after >= 0 ? states[jb.out_after].nvox : 0) + v] = q;
    if (jb.feed >= 0) stage[jobs[jb.feed].off_in + (jb.feed_after >= 0 ? states[jb.feed_after].nvox : 0) + v] = q;
  }
  if (jb.feed >= 0) fold_box(&states[jb.feed], q.x, q.y, q.z, valid);
  if (jb.map) {  // the 1 m box scan-to-map grids this cloud into (map_upload's cloud_box)
    int c[6] = {valid ? (int)floorf(q.x) : INT_MAX, valid ? (int)floorf(q.y) : INT_MAX, valid ? (int)floorf(q.z) : INT_MAX,
                valid ? (int)floorf(q.x) : INT_MIN, valid ? (int)floorf(q.y) : INT_MIN, valid ? (int)floorf(q.z) : INT_MIN};
    for (int o = 32; o; o >>= 1)
      for (int a = 0; a < 3; ++a) c[a] = min(c[a], __shfl_xor(c[a], o)), c[3 + a] = max(c[3 + a], __shfl_xor(c[3 + a], o));
    if ((threadIdx.x & 63) == 0 && c[0] <= c[3])
      for (int a = 0; a < 3; ++a) atomicMin(&st.bmin[a], c[a]), atomicMax(&st.bmax[a], c[3 + a]);
  }
}

}  // namespace

void launch_lm_transform(hipStream_t s, int n_blocks, const LmSeg* segs, const int2* blocks, const float4* frames, float4* stage, LmState* states) {
  if (n_blocks)
    hipLaunchKernelGGL(lm_transform_kernel, dim3(n_blocks), dim3(kLmTile), 0, s, segs, blocks, frames, stage, states);
}

void launch_lm_stage_scans(hipStream_t s, int n_blocks, const LmScanSeg* segs, const int2* blocks, float4* stage, LmState* states) {
  if (n_blocks) hipLaunchKernelGGL(lm_stage_scans_kernel, dim3(n_blocks), dim3(kLmTile), 0, s, segs, blocks, stage, states);
}

// the kernels of a stage one by one (what launch_lm_stage runs; the key-frame archive runs the same kernels around its
// own scans, lins_archive_capi.hip): the job kernels over jobs [j0, j0 + n_jobs), the tile kernels over tiles [0, n_tiles)
void launch_lm_setup(hipStream_t s, int j0, int n_jobs, const LmJob* jobs, LmState* states) {
  if (n_jobs) hipLaunchKernelGGL(lm_setup_kernel, dim3((n_jobs + 63) / 64), dim3(64), 0, s, j0, n_jobs, jobs, states);
}
void launch_lm_keys(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const float4* stage, unsigned* keys, int* vals) {
  if (n_tiles) hipLaunchKernelGGL(lm_keys_kernel, dim3(n_tiles), dim3(kLmTile), 0, s, tiles, jobs, states, stage, keys, vals);
}
void launch_lm_hist(hipStream_t s, int pass, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const unsigned* kin, int* hist) {
  if (n_tiles) hipLaunchKernelGGL(lm_hist_kernel, dim3(n_tiles), dim3(kLmTile), 0, s, pass, tiles, jobs, states, kin, hist);
}
void launch_lm_scan(hipStream_t s, int pass, int j0, int n_jobs, const LmJob* jobs, const LmState* states, int* hist) {
  if (n_jobs) hipLaunchKernelGGL(lm_scan_kernel, dim3(n_jobs), dim3(kLmTile), 0, s, pass, j0, jobs, states, hist);
}
void launch_lm_scatter(hipStream_t s, int pass, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const int* hist, const unsigned* kin,
                       const int* vin, unsigned* kout, int* vout) {
  if (n_tiles) hipLaunchKernelGGL(lm_scatter_kernel, dim3(n_tiles), dim3(kLmTile), 0, s, pass, tiles, jobs, states, hist, kin, vin, kout, vout);
}
void launch_lm_heads(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const unsigned* keys_a, const unsigned* keys_b,
                     int* tilecnt) {
  if (n_tiles) hipLaunchKernelGGL(lm_heads_kernel, dim3(n_tiles), dim3(kLmTile), 0, s, tiles, jobs, states, keys_a, keys_b, tilecnt);
}
void launch_lm_heads_scan(hipStream_t s, int j0, int n_jobs, const LmJob* jobs, LmState* states, int* tilecnt) {
  if (n_jobs) hipLaunchKernelGGL(lm_heads_scan_kernel, dim3(n_jobs), dim3(kLmTile), 0, s, j0, jobs, states, tilecnt);
}
void launch_lm_starts(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const unsigned* keys_a, const unsigned* keys_b,
                      const int* tilecnt, int* starts) {
  if (n_tiles) hipLaunchKernelGGL(lm_starts_kernel, dim3(n_tiles), dim3(kLmTile), 0, s, tiles, jobs, states, keys_a, keys_b, tilecnt, starts);
}
void launch_lm_sum(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, LmState* states, const int* vals_a, const int* vals_b, const int* starts,
                   float4* stage, float4* out) {
  if (n_tiles) hipLaunchKernelGGL(lm_sum_kernel, dim3(n_tiles), dim3(kLmTile), 0, s, tiles, jobs, states, vals_a, vals_b, starts, stage, out);
}

// one stage: jobs [j0, j0 + n_jobs), tiles [0, n_tiles) of `tiles`.  The first n_split jobs have their two scans — each
// radix pass's histogram, the per-tile run heads — split over many workgroups (launch_ar_scan over the chunk tables, as
// lins_archive_assemble builds them); the others take the one-workgroup scans.  Both kinds share every other launch.
void launch_lm_stage_split(hipStream_t s, int j0, int n_split, int n_jobs, int n_tiles, const int2* tiles, const LmJob* jobs, LmState* states,
                           float4* stage, unsigned* keys_a, unsigned* keys_b, int* vals_a, int* vals_b, int* hist, int* tilecnt,
                           int* starts, float4* out, int chunk_tiles, int n_chunks, const ArChunk* chunks, const ArSplit* splits, int* csum) {
  if (!n_jobs) return;
  launch_lm_setup(s, j0, n_jobs, jobs, states);
  if (!n_tiles) return;
  launch_lm_keys(s, n_tiles, tiles, jobs, states, stage, keys_a, vals_a);
  for (int p = 0; p < kLmPasses; ++p) {
    unsigned *kin = (p & 1) ? keys_b : keys_a, *kout = (p & 1) ? keys_a : keys_b;
    int *vin = (p & 1) ? vals_b : vals_a, *vout = (p & 1) ? vals_a : vals_b;
    launch_lm_hist(s, p, n_tiles, tiles, jobs, states, kin, hist);
    launch_lm_scan(s, p, j0 + n_split, n_jobs - n_split, jobs, states, hist);
    launch_ar_scan(s, 256, p, chunk_tiles, n_chunks, chunks, n_split, splits, jobs, states, hist, csum);
    launch_lm_scatter(s, p, n_tiles, tiles, jobs, states, hist, kin, vin, kout, vout);
  }
  launch_lm_heads(s, n_tiles, tiles, jobs, states, keys_a, keys_b, tilecnt);
  launch_lm_heads_scan(s, j0 + n_split, n_jobs - n_split, jobs, states, tilecnt);
  launch_ar_scan(s, 1, -1, chunk_tiles, n_chunks, chunks, n_split, splits, jobs, states, tilecnt, csum);
  launch_lm_starts(s, n_tiles, tiles, jobs, states, keys_a, keys_b, tilecnt, starts);
  launch_lm_sum(s, n_tiles, tiles, jobs, states, vals_a, vals_b, starts, stage, out);
}

// a stage without split jobs
void launch_lm_stage(hipStream_t s, int j0, int n_jobs, int n_tiles, const int2* tiles, const LmJob* jobs, LmState* states,
                     float4* stage, unsigned* keys_a, unsigned* keys_b, int* vals_a, int* vals_b, int* hist, int* tilecnt,
                     int* starts, float4* out) {
  launch_lm_stage_split(s, j0, 0, n_jobs, n_tiles, tiles, jobs, states, stage, keys_a, keys_b, vals_a, vals_b, hist, tilecnt, starts, out, 0, 0,
                        nullptr, nullptr, nullptr);
}

}  // namespace lins
