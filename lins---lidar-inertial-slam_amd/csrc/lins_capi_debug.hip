// lins_capi_debug.hip — every lins_debug_* entry point of the C ABI (include/lins_ieskf.h): test and measurement aids,
// not part of the drop-in surface.
#include <vector>

#include "lins_ctx.h"
#include "lm_math.h"
#include "loop_icp.h"

using namespace lins;

extern "C" {

/* Debug aid (unit tests of the device math against the oracle; see debug_kernels.hip for the op codes):
 * evaluates op on n items of n_in doubles each, n_out doubles out per item. */
int lins_debug_math(lins_ctx* ctx, int op, int n, const double* in, int n_in, double* out, int n_out) {
  if (ctx && in && out && op >= 100 && op <= 111 && n >= 1 && n_in >= 9 && n_out == 2) {  // cycle microbenchmarks, n blocks
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<double> d_in, d_out;
    BUF_TRY(ctx, d_in.grow(9));
    BUF_TRY(ctx, d_out.grow((size_t)n * 2));
    HIP_TRY(ctx, hipMemcpy(d_in, in, 9 * 8, hipMemcpyHostToDevice));
    launch_debug_cycles(ctx->stream, op, n, d_in, d_out);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, d_out, (size_t)n * 2 * 8, hipMemcpyDeviceToHost));
    return LINS_OK;
  }
  static const int kIn[20] = {4, 3, 3, 37, 38, 4, 24, 42, 42, 448, 448, 42, 42, 3, 4, 4, 43, 43, 72, 72};
  static const int kOut[20] = {3, 4, 9, 19, 18, 12, 3, 6, 6, 28, 28, 6, 6, 4, 3, 12, 6, 6, 44, 44};
  if (!ctx || !in || !out || op < 0 || op > 19 || n < 0 || n_in != kIn[op] || n_out != kOut[op]) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DevBuf<double> d_in, d_out;
  DevBuf<LmCarry> d_lm;
  BUF_TRY(ctx, d_in.grow((size_t)n * n_in));
  hipError_t e = (hipError_t)d_out.grow((size_t)n * n_out);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, (size_t)n * n_in * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    if (op == 9 || op == 10)
      launch_debug_reduce_rows(ctx->stream, op, n, d_in, d_out);
    else if (op == 8 || op == 12)
      launch_debug_wave_solve(ctx->stream, n, op == 12, d_in, d_out);
    else if (op == 16 || op == 17)
      launch_debug_icp_gn(ctx->stream, n, op == 17, d_in, d_out);
    else if (op == 18 || op == 19) {  // lm_step_from_sums: one thread (lm_math.h) / over a wave (lm_wave.h); 72 in, 44 out
      e = (hipError_t)d_lm.grow((size_t)n);
      if (e == hipSuccess) launch_debug_lm_step(ctx->stream, n, op == 19, d_in, d_out, d_lm);
    }
    else
      launch_debug_math(ctx->stream, op, n, n_in, n_out, d_in, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * n_out * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx_fail_hip(ctx, e, "lins_debug_math");
  return LINS_OK;
}

/* Debug aid (not part of the drop-in surface; tests/test_gpu_context_state.py): read (write = 0) or write (write = 1)
 * `bytes` bytes at `offset_bytes` of the context's scratch state that outlives a run — which = 0: the carry records of
 * the batch kernel (ieskf_lds_lean.h, kRelayLaneInts ints per scan), 1: the walk cache (32 B per query slot).
 * Synchronous, ordered behind both launch queues and the gather stream. */
int lins_debug_scratch(lins_ctx* ctx, int which, int write, size_t offset_bytes, size_t bytes, void* host) {
  if (!ctx || !host || (which != 0 && which != 1)) return LINS_E_ARG;
  char* const base = which == 0 ? reinterpret_cast<char*>(ctx->d_relay_lane) : reinterpret_cast<char*>(ctx->d_walk_cache);
  const size_t cap = which == 0 ? (size_t)ctx->max_batch * kRelayLaneInts * sizeof(int) : ctx->slot_cap * 32;
  if (!base || offset_bytes > cap || bytes > cap - offset_bytes) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = pipe_join(ctx)) return rc;
  if (write)
    HIP_TRY(ctx, hipMemcpyAsync(base + offset_bytes, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  else
    HIP_TRY(ctx, hipMemcpyAsync(host, base + offset_bytes, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}


/* Debug aid (not part of the drop-in surface): enable / read the per-workgroup phase
 * profile of the persistent kernel: 16 int64 shader-clock ticks per scan
 * ([0] setup [1] correspondence [2] reduction [3] solve [4] update [5] total [6..10] per wave). */
int lins_debug_phase_profile(lins_ctx* ctx, int enable, long long* out, int n_scans) {
  if (!ctx) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  if (enable && !ctx->d_prof) {
    // (16 words per scan, then — behind the records of the launch — 32 words per scan of per-wave phase ticks, written by
    // libraries built with -DLINS_PROF2=k: lins_debug_wave_phases)
    BUF_TRY(ctx, ctx->d_prof.grow((size_t)ctx->max_batch * 80));
    HIP_TRY(ctx, hipMemset(ctx->d_prof, 0, (size_t)ctx->max_batch * 80 * sizeof(long long)));
  }
  if (out && ctx->d_prof) {
    if (n_scans > ctx->max_batch) return LINS_E_CAPACITY;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_prof, (size_t)n_scans * 16 * sizeof(long long), hipMemcpyDeviceToHost));
  }
  if (!enable) ctx->d_prof.reset();
  return LINS_OK;
}

/* Debug aid (libraries built with -DLINS_QUEUE_TRACE=1, a several-part run): per workgroup of the last launch, in
 * workgroup-index order, four words: start, item in hand, end (100 MHz wall clock) and the item (scan | part << 27, -1 =
 * none: the later part of an update that had ended).                                                                  */
int lins_debug_queue_trace(lins_ctx* ctx, long long* out, int n_wg) {
  if (!ctx || !out || n_wg < 0) return LINS_E_ARG;
  if (!ctx->d_queue || n_wg > 15 * ctx->max_batch) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, ctx->d_queue + lds_mr_queue_flags_offset() + (size_t)ctx->max_batch, (size_t)n_wg * 32, hipMemcpyDeviceToHost));
  return LINS_OK;
}

/* Debug aid (libraries built with -DLINS_PROF2=k, profile enabled, whole updates of the batch kernel): per scan 8 waves x
 * 8 phases of 32-bit shader-clock ticks summed over the iterations >= k — [0] query load + de-skew [1] nearest
 * neighbour: certificates + searches [2] second / third point [3] rows [4] row reduction [5] wait at the barrier behind
 * it [6] fold + barrier [7] solve / update (the waves that do not solve wait here).  n_scans = the scans of the last run. */
int lins_debug_wave_phases(lins_ctx* ctx, int* out, int n_scans) {
  if (!ctx || !out) return LINS_E_ARG;
  if (!ctx->d_prof || n_scans != ctx->n_uploaded) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, ctx->d_prof + (size_t)n_scans * 16, (size_t)n_scans * 64 * sizeof(int), hipMemcpyDeviceToHost));
  return LINS_OK;
}

/* Debug aid (LINS_PROF2 builds): per scan 8 waves x 8 counts over the iterations >= k — nearest-neighbour phase: max over
 * the lanes of the window scans (scan_spans calls) and of the grid positions they cover, the sums of both over the lanes;
 * then the same four for the walk phase. */
int lins_debug_wave_counts(lins_ctx* ctx, int* out, int n_scans) {
  if (!ctx || !out) return LINS_E_ARG;
  if (!ctx->d_prof || n_scans != ctx->n_uploaded) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, ctx->d_prof + (size_t)n_scans * 48, (size_t)n_scans * 64 * sizeof(int), hipMemcpyDeviceToHost));
  return LINS_OK;
}

/* Debug aid (LINS_PROF2 builds): the per-query slots of the uploaded batch (int4 each), where the profiled batch kernel
 * leaves (searches, walks, walk mask by iteration, ring) of every query. */
int lins_debug_query_slots(lins_ctx* ctx, int* out, int n_slots) {
  if (!ctx || !out || n_slots < 0 || (size_t)n_slots > ctx->slot_cap) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, ctx->d_idx, (size_t)n_slots * sizeof(int4), hipMemcpyDeviceToHost));
  return LINS_OK;
}

/* Measurement aid ("measure a device-copy ceiling with a stream kernel and report
 * against both"): a grid-stride float4 copy of `bytes` bytes inside the context's point arenas,
 * timed with HIP events on the context's stream; *gbs = (read + written bytes) / time of the best
 * of `reps` launches.  An uploaded batch stays valid (only the scratch arena is written).       */
int lins_debug_stream_copy(lins_ctx* ctx, uint64_t bytes, int reps, double* gbs) {
  if (!ctx || !gbs || reps < 1) return LINS_E_ARG;
  const size_t cap = ctx->arena_cap * sizeof(float4);
  if (bytes > cap) bytes = cap;
  const size_t n4 = bytes / sizeof(float4);
  if (!n4) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  float best = 1e30f;  // (source = the cloud arena, untouched; destination = the sorted-copy arena, scratch)
  for (int r = 0; r < reps + 1; ++r) {  // (first launch: warm-up)
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    launch_stream_copy(ctx->stream, ctx->d_arena, ctx->d_binned, n4);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev2));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev2));
    if (r && ms < best) best = ms;
  }
  *gbs = 2.0 * (double)(n4 * sizeof(float4)) / ((double)best * 1e-3) / 1e9;
  return LINS_OK;
}

/* measurement aid (tools/pull_copy_rate.py): `bytes` of the pinned staging arena to the device arena — mode 0: hipMemcpyAsync
 * (what the uploads do), mode 1: a copy KERNEL reading the host memory over PCIe (launch_stream_copy on the mapped pointer) —
 * best of `reps`, GB/s one way. */
int lins_debug_pull_copy(lins_ctx* ctx, uint64_t bytes, int reps, int mode, double* gbs) {
  if (!ctx || !gbs || reps < 1) return LINS_E_ARG;
  const size_t cap = ctx->arena_cap * sizeof(float4);
  if (bytes > cap) bytes = cap;
  const size_t n4 = bytes / sizeof(float4);
  if (!n4) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = pipe_join(ctx)) return rc;
  float4* mapped = nullptr;
  HIP_TRY(ctx, hipHostGetDevicePointer((void**)&mapped, ctx->h_arena, 0));
  float best = 1e30f;
  for (int r = 0; r < reps + 1; ++r) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    if (mode == 0)
      HIP_TRY(ctx, hipMemcpyAsync(ctx->d_binned, ctx->h_arena, n4 * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    else
      launch_stream_copy(ctx->stream, mapped, ctx->d_binned, n4);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev2));
    float ms = 0;
    HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev2));
    if (r && ms < best) best = ms;
  }
  *gbs = (double)(n4 * sizeof(float4)) / ((double)best * 1e-3) / 1e9;
  return LINS_OK;
}

/* Debug aids of the loop-closure ICP (not part of the drop-in surface; tests/test_gpu_loop_icp.py; declared by their users).
 * rounds: lins_loop_icp_batch of this context stops every problem after `rounds` rounds (0: off) — a problem still running
 * then reports converged = 0, reason = LINS_ICP_NONE and the T, mse, n_corr of its last round, so that every round of the
 * device's own loop can be held against the restatement's trace.
 * shells: the search scans at most `shells` shells per query (1: its own cell only) before the query is finished by the
 * whole-target scan; 0 sends every query that way; negative: the default.  Results are the same bits for every value.
 * group: rounds queued between two reads of the "still running" word (0: the default); a speed knob, same bits.
 * last_far: the queries the last lins_loop_icp_batch / lins_loop_icp_correspondences finished by the whole-target scan. */
int lins_debug_loop_icp_rounds(lins_ctx* ctx, int rounds) { return loop_icp_debug_set(ctx, 0, rounds); }
int lins_debug_loop_icp_shells(lins_ctx* ctx, int shells) { return loop_icp_debug_set(ctx, 1, shells < 0 ? loop_icp_debug_shells_default() : shells); }
int lins_debug_loop_icp_group(lins_ctx* ctx, int group) { return loop_icp_debug_set(ctx, 2, group); }
int lins_debug_loop_icp_last_far(lins_ctx* ctx, uint32_t* far_searches) {
  if (!ctx || !far_searches) return LINS_E_ARG;
  *far_searches = loop_icp_last_far(ctx);
  return LINS_OK;
}

/* step: the device's step kernel (launch_loop_step: the tile loop, the fit, the composition, the stop rule) on sums the
 * caller hands over instead of the search — the device side of lins_host_loop_icp_step (include/lins_host.h;
 * tests/test_gpu_loop_fit.py).  n problems; problem k adds its first n_tiles[k] <= blocks_per_problem tiles of
 * partials[(k * blocks_per_problem + tile) * 17 + sum], in order (the tiles behind them are not read); status[k] != 0: the
 * problem is not run.  mode as launch_loop_step.  states: in and out (`move` out only); an inactive problem (mode 0) or
 * one with a status comes back as it went in.  still_running (may be null): the problems that go on after the round. */
int lins_debug_loop_icp_step(lins_ctx* ctx, int n, int blocks_per_problem, const int32_t* n_tiles, const int32_t* status, const double* partials,
                             const lins_loop_icp_params* prm, int mode, lins_loop_icp_state* states, int32_t* still_running) {
  if (!ctx || n < 1 || blocks_per_problem < 1 || !n_tiles || !status || !partials || !prm || (mode != 0 && mode != 1) || !states) return LINS_E_ARG;
  std::vector<LoopDev> probs(n, LoopDev{});
  std::vector<lins_licp::State> st(n);
  for (int k = 0; k < n; ++k) {
    if (n_tiles[k] < 0 || n_tiles[k] > blocks_per_problem) return LINS_E_ARG;
    probs[k].n_src = n_tiles[k] * kLoopQPerBlock, probs[k].status = status[k];
    for (int a = 0; a < 3; ++a) probs[k].g.cdim[a] = 1;
    lins_licp::state_from_public(states[k], st[k]);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t np = (size_t)n * blocks_per_problem * lins_licp::kSums;
  DevBuf<LoopDev> d_probs;
  DevBuf<lins_licp::State> d_states;
  DevBuf<double> d_partials;
  DevBuf<int> d_running;
  int running = 0;
  hipError_t e = (hipError_t)grow_all(d_probs, (size_t)n, d_states, (size_t)n, d_partials, np, d_running, 1);
  if (e == hipSuccess) e = hipMemcpyAsync(d_probs, probs.data(), (size_t)n * sizeof(LoopDev), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_states, st.data(), (size_t)n * sizeof(lins_licp::State), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_partials, partials, np * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_running, 0, sizeof(int), ctx->stream);
  if (e == hipSuccess) {
    launch_loop_step(ctx->stream, n, blocks_per_problem, mode, *prm, d_probs, d_states, d_partials, d_running);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(st.data(), d_states, (size_t)n * sizeof(lins_licp::State), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&running, d_running, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx_fail_hip(ctx, e, "lins_debug_loop_icp_step");
  for (int k = 0; k < n; ++k) lins_licp::state_to_public(st[k], states[k]);  // (every problem: what the kernel left)
  if (still_running) *still_running = running;
  return LINS_OK;
}

/* Debug aid (not part of the drop-in surface; tests/test_gpu_cov_update.py): the covariance update of the iterated update
 * (SE:594-598) ALONE, by the program one of the update paths runs — path 0: joseph_epilogue of the 1024-thread LDS
 * kernel ("lds"), 1: of its one-lane shape ("lds1"), 2: of the batch kernel ("mr") (debug_cov_update_kernel of each
 * family, ieskf_lds_impl.h: the kernels' own epilogue function on a prior and sums put into their LDS block), 3:
 * ieskf_joseph_kernel, the any-size path's ("binned", "brute").  n cases in ONE launch, one workgroup each: P n x 324
 * the priors, sums n x 21 the upper triangle of A = H^T H row by row (what sym6 reads), r2 = sigma^2, diverged[k] != 0:
 * case k's prior is passed through.  out: n x 324. */
int lins_debug_cov_update(lins_ctx* ctx, int path, int n, const double* P, const double* sums, double r2, const int32_t* diverged, double* out) {
  if (!ctx || path < 0 || path > 3 || n < 1 || !P || !sums || !diverged || !out) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<OutRec> recs(n, OutRec{});
  for (int k = 0; k < n; ++k) recs[k].diverged = diverged[k] != 0;
  const size_t c = (size_t)n;
  DevBuf<double> d_P, d_sums, d_out;
  DevBuf<int> d_div;
  DevBuf<OutRec> d_recs;
  hipError_t e = (hipError_t)grow_all(d_P, c * 324, d_sums, c * 21, d_out, c * 324, d_div, c, d_recs, c);
  if (e == hipSuccess) e = hipMemcpyAsync(d_P, P, (size_t)n * 324 * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_sums, sums, (size_t)n * 21 * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_div, diverged, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_recs, recs.data(), (size_t)n * sizeof(OutRec), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d_out, 0xFF, (size_t)n * 324 * 8, ctx->stream);  // (NaN: an element no thread wrote is seen)
  if (e == hipSuccess) {
    if (path == 3) {
      DevParams prm{};
      prm.r2 = r2;
      launch_joseph(ctx->stream, n, prm, d_P, d_sums, d_recs, d_out);
    } else if (path == 2) {
      launch_debug_cov_lds_mr(ctx->stream, n, r2, d_P, d_sums, d_div, d_out);
    } else {
      launch_debug_cov_lds(ctx->stream, n, path == 0 ? 3 : 1, r2, d_P, d_sums, d_div, d_out);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * 324 * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return ctx_fail_hip(ctx, e, "lins_debug_cov_update");
  return LINS_OK;
}

}  // extern "C"
