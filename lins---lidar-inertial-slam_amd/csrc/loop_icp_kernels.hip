// loop_icp_kernels.hip — the loop-closure ICP on the device (include/lins_map.h lins_loop_icp_*; performLoopClosure's
// pcl::IterativeClosestPoint, LM:1114-1141): per round one search + sums kernel and one step kernel, queued back to
// back; the arithmetic is loop_icp_math.h, the text the CPU restatement compiles too.
//
// The target (tens of thousands of points) is bucketed into 1 m cells by map_grid_kernel.  kLoopLanes lanes share a
// query: they scan its own cell, then the Chebyshev shells r = 1, 2, ... around it (clipped to the box; a query outside
// the box starts from the nearest box cell), keeping the smallest (squared-distance bits, index) key.  After every
// shell a certificate is tried: every unscanned cell lies, on some axis, beyond a cell face at distance m of the query,
// so an unscanned point has |x' - p| >= m on that axis.  With m' a float not above m, rounding being monotone, the
// point's computed d is >= fl(m' m'); the search ends when the best d is BELOW that — strictly, so that an unscanned
// point of equal d and smaller index cannot exist either.  A query still open after `shells` shells is finished by the
// whole wave scanning the whole target (the deferred hard search of the batch IESKF kernel): the answer is the
// exhaustive search's whatever the budget.
#include <hip/hip_runtime.h>

#include "lins_launch.h"
#include "loop_icp.h"

namespace lins {

using lins_licp::kSums;
using lins_licp::State;

namespace {

constexpr unsigned long long kNoKey = ((unsigned long long)0x7F800000u << 32) | 0xFFFFFFFFull;

__device__ __forceinline__ unsigned long long key_of(float qx, float qy, float qz, const float4& t) {
  const float d = lins_licp::sqdist(qx, qy, qz, t.x, t.y, t.z);
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(t.w);
}

__device__ __forceinline__ int cell_coord(float v, int cmin, int cdim) {
  // defined for every float (the clamp of map_corr_kernel), then clipped to the box: the nearest box cell
  const float kFar = 1073741824.f;
  const long long c = (long long)(int)floorf(fminf(fmaxf(v, -kFar), kFar)) - cmin;
  return c < 0 ? 0 : (c >= cdim ? cdim - 1 : (int)c);
}

}  // namespace

__global__ __launch_bounds__(kLoopBlock) void loop_search_kernel(int n_problems, int blocks_per_problem, int mode, int shells, float cap2,
                                                                 const LoopDev* __restrict__ probs, State* __restrict__ states,
                                                                 const float4* __restrict__ pts, const int* __restrict__ cells,
                                                                 double* __restrict__ partials, int32_t* __restrict__ out_idx,
                                                                 float* __restrict__ out_d) {
  // the XCD-aware block -> (problem, block) mapping of map_corr_kernel: one problem's target sits in one L2
  const int xcd = blockIdx.x & 7, kk = blockIdx.x >> 3;
  const int prob = (kk / blocks_per_problem) * 8 + xcd, blk = kk % blocks_per_problem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (prob >= n_problems) return;
  const LoopDev pd = probs[prob];
  State* const st = states + prob;
  if (pd.status || blk * kLoopQPerBlock >= pd.n_src) return;  // (uniform; the step kernel adds this problem's own tiles only)
  if (mode == 0 && !st->active) return;
  float M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = st->M[i];
  const int q = blk * kLoopQPerBlock + tid / kLoopLanes, sub = tid % kLoopLanes;
  const bool valid = q < pd.n_src;
  const MapGrid g = pd.g;
  const float4* gp = pts + g.off_pts;
  const int* gc = cells + g.off_cells;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  unsigned long long key = kNoKey;
  bool open = false;  // no certificate within the shell budget
  if (valid) {
    const float4 po = pd.src[q];
    lins_licp::move_point(M, po.x, po.y, po.z, sx, sy, sz);
    const int cx = cell_coord(sx, g.cmin[0], g.cdim[0]), cy = cell_coord(sy, g.cmin[1], g.cdim[1]), cz = cell_coord(sz, g.cmin[2], g.cdim[2]);
    const int c[3] = {cx, cy, cz};
    const float s3[3] = {sx, sy, sz};
    open = true;
    for (int r = 0; r < shells && open; ++r) {
      for (int dz = -r; dz <= r; ++dz) {
        const int iz = cz + dz;
        if (iz < 0 || iz >= g.cdim[2]) continue;
        for (int dy = -r; dy <= r; ++dy) {
          const int iy = cy + dy;
          if (iy < 0 || iy >= g.cdim[1]) continue;
          const int row = (iz * g.cdim[1] + iy) * g.cdim[0];
          const bool face = dz == -r || dz == r || dy == -r || dy == r;
          // a face row of the shell: the x-span is one run of consecutive cells; an inner row: its two end cells
          const int x0 = cx - r, x1 = cx + r;
          const int a0 = x0 < 0 ? (face ? 0 : -1) : x0, a1 = face ? (x1 >= g.cdim[0] ? g.cdim[0] - 1 : x1) : x0;
          if (a0 >= 0) {
            const int s = gc[row + a0], e = gc[row + a1 + 1];
            for (int p = s + sub; p < e; p += kLoopLanes) {
              const unsigned long long ck = key_of(sx, sy, sz, gp[p]);
              key = ck < key ? ck : key;
            }
          }
          if (!face && r > 0 && x1 < g.cdim[0]) {
            const int s = gc[row + x1], e = gc[row + x1 + 1];
            for (int p = s + sub; p < e; p += kLoopLanes) {
              const unsigned long long ck = key_of(sx, sy, sz, gp[p]);
              key = ck < key ? ck : key;
            }
          }
        }
      }
      // the query's lanes agree on the best so far (they are in the same control flow: the shell count is the query's)
#pragma unroll
      for (int m = 1; m < kLoopLanes; m <<= 1) {
        const unsigned long long ok = __shfl_xor(key, m);
        key = ok < key ? ok : key;
      }
      // certificate over the cells beyond shell r
      float mfar = INFINITY;
      bool any = false;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (c[a] - r - 1 >= 0) any = true, mfar = fminf(mfar, s3[a] - (float)(g.cmin[a] + c[a] - r));
        if (c[a] + r + 1 < g.cdim[a]) any = true, mfar = fminf(mfar, (float)(g.cmin[a] + c[a] + r + 1) - s3[a]);
      }
      if (!any) {
        open = false;  // the whole box was scanned
      } else if (mfar > 0.f) {  // (false for a NaN too: such a query goes the far way)
        const float ml = mfar * 0.99999f;  // not above the real distance: the subtraction rounds by 2^-24 at most
        const float bound = ml * ml;
        if (__uint_as_float((unsigned)(key >> 32)) < bound) open = false;
      }
    }
  }
  // the open queries, one after the other, by the whole wave over the whole target
  unsigned long long farmask = __ballot(open);
  if (lane == 0 && farmask) atomicAdd(&st->far, (unsigned)(__popcll(farmask) / kLoopLanes));
  while (farmask) {  // (uniform)
    const int leader = __ffsll((long long)farmask) - 1;
    farmask &= ~(0xFFull << leader);
    const float qx = __shfl(sx, leader), qy = __shfl(sy, leader), qz = __shfl(sz, leader);
    unsigned long long k = kNoKey;
    for (int p = lane; p < pd.n_tgt; p += 64) {
      const unsigned long long ck = key_of(qx, qy, qz, gp[p]);
      k = ck < k ? ck : k;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long ok = __shfl_xor(k, o);
      k = ok < k ? ok : k;
    }
    if ((lane & ~(kLoopLanes - 1)) == leader) key = k;
  }
  double v[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = 0.0;
  if (valid && sub == 0) {
    const float d = __uint_as_float((unsigned)(key >> 32));
    const bool counted = key != kNoKey && (mode == 1 || cap2 < 0.f || d <= cap2);
    const int idx = (int)(unsigned)key;
    if (counted) {
      const float4 t = pd.tgt[idx];
      lins_licp::corr_terms(sx, sy, sz, t.x, t.y, t.z, d, v);
    }
    if (out_idx) out_idx[q] = counted ? idx : -1, out_d[q] = counted ? d : 0.f;
  }
  // the sums: wave butterfly over the lanes 32, 16, 8 apart (tree8 of loop_icp_math.h), then the four waves in order
  __shared__ double wsum[kLoopBlock / 64][kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    double x = v[k];
#pragma unroll
    for (int o = 32; o >= kLoopLanes; o >>= 1) {
      const int lo = __shfl_xor(__double2loint(x), o), hi = __shfl_xor(__double2hiint(x), o);
      x += __hiloint2double(hi, lo);
    }
    if (lane == 0) wsum[wave][k] = x;
  }
  __syncthreads();
  if (tid < kSums) {
    double s = 0.0;
    for (int w = 0; w < kLoopBlock / 64; ++w) s += wsum[w][tid];
    partials[((size_t)prob * blocks_per_problem + blk) * kSums + tid] = s;
  }
}

__global__ __launch_bounds__(64) void loop_step_kernel(int n_problems, int blocks_per_problem, int mode, lins_loop_icp_params prm,
                                                       const LoopDev* __restrict__ probs, State* __restrict__ states,
                                                       const double* __restrict__ partials, int* __restrict__ still_running) {
  __shared__ double sums[kSums];
  const int k = blockIdx.x, lane = threadIdx.x;
  const LoopDev pd = probs[k];
  if (pd.status) return;
  if (mode == 0 && !states[k].active) return;  // (uniform)
  const int ntiles = (pd.n_src + kLoopQPerBlock - 1) / kLoopQPerBlock;
  if (lane < kSums) {
    double s = 0.0;
    for (int b = 0; b < ntiles; ++b) s += partials[((size_t)k * blocks_per_problem + b) * kSums + lane];
    sums[lane] = s;
  }
  __syncthreads();
  if (lane == 0) {  // 3 x 3 algebra: one lane (the wave's other lanes only add the partials)
    State s = states[k];
    if (mode == 0) {
      double D[16], q[4];
      lins_licp::step_from_sums(prm, sums, s, D, q);
      if (s.active && still_running) atomicAdd(still_running, 1);
    } else {
      lins_licp::fitness_from_sums(sums, s);
    }
    states[k] = s;
  }
}

void launch_loop_search(hipStream_t s, int n_problems, int blocks_per_problem, int mode, int shells, float cap2, const LoopDev* probs,
                        State* states, const float4* pts, const int* cells, double* partials, int32_t* out_idx, float* out_d) {
  // (one-dimensional grid: 8 x blocks_per_problem x ceil(n_problems / 8), as launch_map_corr)
  hipLaunchKernelGGL(loop_search_kernel, dim3(8 * blocks_per_problem * ((n_problems + 7) / 8)), dim3(kLoopBlock), 0, s, n_problems,
                     blocks_per_problem, mode, shells, cap2, probs, states, pts, cells, partials, out_idx, out_d);
}

void launch_loop_step(hipStream_t s, int n_problems, int blocks_per_problem, int mode, const lins_loop_icp_params& prm, const LoopDev* probs,
                      State* states, const double* partials, int* still_running) {
  hipLaunchKernelGGL(loop_step_kernel, dim3(n_problems), dim3(64), 0, s, n_problems, blocks_per_problem, mode, prm, probs, states, partials,
                     still_running);
}

}  // namespace lins
