// lins_capi.hip — implementation of the C ABI in include/lins_ieskf.h.
//
// Owns: one HIP stream, the device arena (all four clouds of every uploaded scan
// pair, 64-byte aligned spans of float4), per-scan descriptors, prior / posterior
// state + covariance, and pinned host staging.  Caller owns every host buffer it
// passes in; nothing is retained after a call returns.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <new>
#include <thread>
#include <string>
#include <vector>

#include <dlfcn.h>
// RCCL: types only — the library is dlopen()ed on first use (lins_rccl_*), never linked.  Without its header (a ROCm
// install with no rccl-dev; -DLINS_NO_RCCL_HEADER to check) the four types the entry points need are declared here:
// their ABI (an opaque communicator pointer, the 128-byte id, int enums with ncclSuccess = ncclChar = 0) has not changed
// since NCCL 2.0, and a box without the library answers LINS_E_UNSUPPORTED at run time as before.
#if __has_include(<rccl/rccl.h>) && !defined(LINS_NO_RCCL_HEADER)
#include <rccl/rccl.h>
#else
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclChar = 0 } ncclDataType_t;
#endif

#include "../../include/lins_host.h"
#include "ieskf_device.h"
#include "ieskf_grid.h"
#include "lins_ctx_priv.h"

namespace lins {
void launch_persistent(hipStream_t, int, const DevParams&, const ScanDesc*, const float4*, const double*,
                       const double*, double*, double*, double*, void*, int4*, lins_pose_record*, int, float4*, long long*);
void launch_pass(hipStream_t, int, const DevParams&, const ScanDesc*, const float4*, const double*, const double*,
                 int, int4*, lins_corr*, double*, int*, float4*);
void launch_joseph(hipStream_t, int, const DevParams&, const double*, const double*, const void*, double*);
void launch_lds(hipStream_t, int, const DevParams&, int, const ScanDesc*, const float4*, const float4*, const GridTables*, const double*, const double*,
                double*, double*, double*, void*, int4*, lins_pose_record*, int, long long*, int*);
void launch_lds_pass(hipStream_t, int, const DevParams&, int, const ScanDesc*, const float4*, const float4*, const GridTables*, const double*,
                     const double*, int, int4*, lins_corr*, double*, int*);
int lds_np_cap();
void launch_lds_mr(hipStream_t, int, const DevParams&, const ScanDesc*, const int*, const float4*, const float4*, const GridTables*, const double*,
                   const double*, double*, double*, double*, void*, int4*, lins_pose_record*, int, long long*, const RelayArgs*, unsigned*, int, int*);
int lds_mr_resident_workgroups(int n_cu);
bool lds_mr_has_parts();
int lds_mr_queue_flags_offset();
void launch_lds_mr_pass(hipStream_t, int, const DevParams&, const ScanDesc*, const float4*, const float4*, const GridTables*, const double*,
                        const double*, int, int4*, lins_corr*, double*, int*);
int lds_mr_np_cap();
void launch_debug_math(hipStream_t, int, int, int, int, const double*, double*);
void launch_debug_cycles(hipStream_t, int, int, const double*, double*);
void launch_debug_wave_solve(hipStream_t, int, int, const double*, double*);
void launch_debug_icp_gn(hipStream_t, int, int, const double*, double*);
void launch_debug_lm_step(hipStream_t, int, int, const double*, double*, void*);
size_t map_carry_size();
void launch_debug_reduce_rows(hipStream_t, int, int, const double*, double*);
void launch_lds_mr_icp(hipStream_t, int, const DevParams&, const ScanDesc*, const float4*, const float4*, const GridTables*, const double*, double*,
                       void*, int4*);
void launch_transform_to_end(hipStream_t, int, int, const void*, const float4*, float4*, float4*);
size_t reproject_job_size();
void launch_stream_copy(hipStream_t, const float4*, float4*, size_t);
void launch_frontend(hipStream_t, int, const void*, const float4*, const float*, const unsigned*, const unsigned char*,
                     double, int*, float4*, int*);
void launch_reproject_in_place(hipStream_t, int, int, const void*, const double*, float4*, double);
size_t stream_cloud_size();
void launch_segment(hipStream_t, int, const void*, const float4*, float, float, float, float, float, unsigned*, int*, void*, float4*,
                    float*, unsigned*, unsigned char*, int*);
size_t sg_raw_size();
struct SgRawHost {
  long long off;
  int n, pad;
};
struct StreamCloudHost {
  long long off;
  int n, stream;
};
size_t fe_scan_size();
int fe_pick_stride();
struct FeScanHost {
  long long off;
  int n;
  int start_ring[16], end_ring[16];
  float start_ori, end_ori, ori_diff;
  int pad;
  long long o_sharp, o_less_sharp, o_flat, o_less_flat;
};
struct ReprojectJobHost {
  long long off;
  int n, has_yzx;
  double t[3], q[4];
  double inv_period;
};
size_t out_rec_size();
struct OutRecHost {
  double residual_norm, update_norm;
  int iters, converged, diverged, m_surf, m_corner, pad[3];
};
}  // namespace lins

using namespace lins;

struct lins_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;  // IESKF kernel start / end, Joseph kernel end
  hipStream_t copy_stream = nullptr;  // lins_ieskf_update_batch: uploads of the next chunk beside the running one
  hipEvent_t ev_copy = nullptr;
  size_t slots_uploaded = 0;    // query slots of the uploaded batch
  lins_params prm{};
  DevParams dprm{};
  int max_batch = 0, max_targets = 0;
  size_t arena_cap = 0, slot_cap = 0;  // points / query slots
  // pinned host staging
  float4* h_arena = nullptr;
  ScanDesc* h_desc = nullptr;
  double* h_state = nullptr;
  double* h_cov = nullptr;
  // The per-scan records of a batch live in ONE pinned block and two device blocks of the same layout —
  //   host      [state | cov | out records | descriptors]      (h_state, h_cov, h_out, h_desc point into it)
  //   device in [state | cov |   (unused)  | descriptors]      (d_state_in, d_cov_in, d_desc)
  //   device out[state | cov | out records]                    (d_state_out, d_cov_out, d_out)
  // so that a batch that fills the context (n == max_batch: the single-scan context of a live filter, the bench's batch)
  // goes up in ONE copy besides the clouds and comes back in ONE: every hipMemcpyAsync is ~8 us of host time and as much
  // in-order latency on the stream (round 6: lins_ieskf_update of one scan 245 -> see DESIGN.md section 7).
  char *h_meta = nullptr, *d_meta_in = nullptr, *d_meta_out = nullptr;
  size_t meta_in_bytes = 0, meta_out_bytes = 0;
  OutRecHost* h_out = nullptr;
  // device
  float4* d_arena = nullptr;
  float4* d_binned = nullptr;  // (ring x column)-sorted copies of the target clouds (any-size kernel), re-projection output
  // search index of the uploaded target clouds (ieskf_grid.h: grid-sorted copy + tables per scan), built by
  // grid_index_kernel where the clouds arrive — the reference's setInputCloud (SE:1156-1160)
  float4* d_gsorted = nullptr;
  GridTables* d_gridtab = nullptr;
  hipEvent_t ev_idx0 = nullptr, ev_idx1 = nullptr;
  bool idx_timed = false;
  // several-part updates of the batch kernel (ieskf_lds_impl.h "relay"): hand-over buffers, the work queue, launch counter
  int relay_at = 4, relay_gen = 0;  // (relay_at: iterations per part; 0 = whole updates.  1024 scans x 10 iterations: 2 -> 0.647 ms,
                                    // 3 -> 0.625, 4 -> 0.615, 5 -> 0.641, 6 -> 0.623, 7 -> 0.626, 8 -> 0.641; whole updates 0.665)
  int relay_cuts = 2;               // cuts an update gets at most: at relay_at, 2 relay_at, ... (the last part runs to the end)
  int relay_list_parts = 0, relay_list_n = 0;  // the item list that is on the device (0 = none for this upload / order)
  double* d_relay_hdr = nullptr;
  int *d_relay_lane = nullptr, *d_queue = nullptr;  // d_queue: ticket counters + one flag per scan (ieskf_lds_impl.h kQ*)
  int queue_grid = 0;               // workgroups of the batch kernel resident at once on this device: larger batches are cut into parts
  long long queue_timeouts = 0;     // hand-over waits that ran out, over the life of the context (lins_last_cut)
  // walk cache of the one-lane-per-query kernels (ieskf_lds_impl.h): per query slot 32 B — the second / third points of the
  // nearest neighbour a query had before; cleared wherever new target clouds arrive, tagged with the launch number
  unsigned* d_walk_cache = nullptr;
  int run_gen = 0;
  int* h_relay_err = nullptr;       // (pinned, device-visible) queue waits that ran out in a launch: checked at lins_sync
  int relay_spins = 1 << 21;        // polls (~1 us) a workgroup waits at an empty queue slot before the launch gives up
  bool streams_fuse = true;         // lins_streams_step: updatePointCloud as one kernel (re-projection + index); debug knob LINS_STREAMS_FUSE
  int last_parts = 0;  // how the last run was cut (lins_last_cut)
  ScanDesc* d_desc = nullptr;
  bool use_order = true;  // (LINS_LAUNCH_ORDER=0 with the debug gate: index order, for A/B timing)
  int *h_order = nullptr, *d_order = nullptr;  // launch order of the uploaded batch (longest-expected-first), see launch_order()
  double *d_state_in = nullptr, *d_cov_in = nullptr, *d_state_out = nullptr, *d_cov_out = nullptr;
  double* d_lin = nullptr;
  float4* d_aux = nullptr;     // third point arena (YZX copies of the re-projection), lazily allocated
  void* d_jobs = nullptr;
  float reproject_ms = 0.f;
  uint64_t reproject_bytes = 0;
  // feature front-end (lins_extract_features_batch): device buffers, allocated on first use for fe_cap scans
  struct Frontend {
    int cap = 0;
    void* d_scans = nullptr;
    float4 *d_cloud = nullptr, *d_out = nullptr;  // d_out: per scan [192 | 1920 | 384 | LINS_CLOUD_MAX]
    float* d_range = nullptr;
    unsigned* d_col = nullptr;
    unsigned char* d_ground = nullptr;
    int *d_picks = nullptr, *d_counts = nullptr;
    // pinned host staging of the packed inputs (grow-only, h_cap points)
    size_t h_cap = 0;
    float4* h_cloud = nullptr;
    float* h_range = nullptr;
    unsigned* h_col = nullptr;
    unsigned char* h_ground = nullptr;
    float ms = 0.f;
    uint64_t bytes = 0;
    // image_projection stage (lins_segment_batch / the raw-cloud streams path): raw points + per-cell scratch
    int sg_cap = 0;
    size_t raw_cap = 0, h_raw_cap = 0;
    float4 *d_raw = nullptr, *h_raw = nullptr;
    void* d_raws = nullptr;
    unsigned* d_cellidx = nullptr;
    int *d_segrows = nullptr, *d_outliers = nullptr;
    float sg_ms = 0.f;
  } fe;
  // device-resident streams (lins_streams_step): per stream two feature slots (this scan's / the last
  // scan's clouds) inside one arena, so that ScanDesc offsets address both
  struct Streams {
    int n = 0, cur = 0;           // slot the NEXT scan's features go to
    float4 *d_arena = nullptr, *d_sorted = nullptr, *d_gsorted = nullptr;
    GridTables* d_gridtab = nullptr;
    ScanDesc* d_desc = nullptr;
    ScanDesc* d_desc_next = nullptr;  // the clouds of the scan just taken in as the NEXT step's targets (fused re-projection + index)
    bool index_ready = false;         // d_gsorted / d_gridtab hold the index of the resident last scans (built by the step before)
    void* d_jobs = nullptr;
    std::vector<int> last_counts;  // per stream: less sharp, less flat of the resident last scan (-1: none yet)
    bool failed = false;           // a step stopped half way (HIP error): the resident clouds are not trustworthy any more
    float update_ms = 0.f, frontend_ms = 0.f, reproject_ms = 0.f;
  } st;
  void* map_state = nullptr;  // scan-to-map row (lins_map_capi.hip), freed through map_state_free
  void (*map_state_free)(void*) = nullptr;
  long long* d_prof = nullptr;  // optional per-workgroup phase profile (lins_debug_phase_profile)
  double* d_a6 = nullptr;  // upper triangle of the last iteration's H^T H, per scan
  void* d_out = nullptr;
  int4* d_idx = nullptr;
  lins_corr* d_dump = nullptr;
  double* d_sums = nullptr;
  int* d_counts = nullptr;
  int n_uploaded = 0;
  bool lds_ok = false;  // every uploaded scan fits the LDS-resident kernel
  bool mr_ok = false;   // ... the multi-resident (hybrid LDS / global) kernel
  int n_cu = 256;       // compute units of the device ("auto": batches beyond this take the mr kernel)
  int last_search = -1; // kernel family the last batch actually ran
  bool lds3_ok = false; // every uploaded scan has at most 336 queries (one round of the 3-lane shape)
  bool ran = false;
  uint64_t bytes_per_iter = 0;
  uint64_t total_iters = 0;
  std::string hip_err;
  // ---- pipelined staged mode (lins_set_pipelined): the pose gather of run k travels on its own stream beside the
  // kernels of run k + 1; the caller alternates two pose buffers, run k uses buffer k & 1
  struct Pipe {
    bool on = false;
    hipStream_t s_comm = nullptr;
    hipEvent_t ev_comm[2] = {nullptr, nullptr};
    // (what a gather waits for are the run's own end-of-launch events — lins_ctx::hist1[h], and hist1b[h] of the second launch
    // queue when the run went out on both: an event record is ~5 us of in-order latency on its stream, so a run records no
    // event that says what another one already does)
    int h_of[2] = {0, 0};
    bool run_split[2] = {false, false};
    bool comm_pending[2] = {false, false};
    unsigned runs = 0;  // staged runs so far (parity = set)
  } pipe;
  // kernel-time history of lins_batch_run: start / end events of the last kHist update kernels
  static constexpr int kHist = 64;
  hipEvent_t hist0[kHist] = {}, hist1[kHist] = {};
  unsigned hist_n = 0;
  // Two launch queues (round 6).  A batch beyond the device's workgroup slots is run as launches of at most that many
  // scans — whole updates, every workgroup resident from its launch's start — dealt alternately to the context's stream
  // and to `stream2`: the slots one launch leaves idle while its slowest updates finish are taken by the workgroups of the
  // other queue's launch, of this run or of the next (runs are not joined: each queue is in order, the two own disjoint
  // scan ranges).  Everything else the context enqueues goes to `stream` behind a join (split_join).
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr;
  int split_h = 0;  // hist1b[split_h]: the end of the last run that used the second launch queue
  hipEvent_t hist0b[kHist] = {}, hist1b[kHist] = {};  // start / end of a run's launches on stream2 (null timing when it had none)
  bool hist_split[kHist] = {};
  bool split_pending = false;  // stream2 holds work the context's stream has not been ordered behind
  bool split_dirty = true;     // the context's stream holds work (uploads, other calls) stream2 has not been ordered behind
  bool comm_default_prio = false;  // (debug knob LINS_COMM_PRIO=0: the gather's stream at the default priority, as before round 6)
  int split_mode = 1;          // 0: one launch per run (several-part updates when the batch exceeds the slots)
  // RCCL (dlopen): one communicator per context
  struct Rccl {
    void* lib = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 0;
    ncclResult_t (*get_unique_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    const char* (*get_error_string)(ncclResult_t) = nullptr;
  } rccl;
};

namespace lins {
hipStream_t ctx_stream(lins_ctx* ctx) { return ctx->stream; }
int ctx_device(lins_ctx* ctx) { return ctx->device; }
int ctx_fail_hip(lins_ctx* ctx, hipError_t e, const char* what) {
  if (ctx) ctx->hip_err = std::string(what) + ": " + hipGetErrorString(e);
  return LINS_E_HIP;
}
void** ctx_map_slot(lins_ctx* ctx, void (*free_fn)(void*)) {
  ctx->map_state_free = free_fn;
  return &ctx->map_state;
}
void ctx_events(lins_ctx* ctx, hipEvent_t* a, hipEvent_t* b) { *a = ctx->ev0, *b = ctx->ev2; }
const lins_params* ctx_params(const lins_ctx* ctx) { return &ctx->prm; }
}  // namespace lins

namespace {

constexpr size_t kLaneIntsPerScan = 4 * 512 * 4;  // ieskf_lds_impl.h kRelayLaneInts: [4][512] 16-byte words per scan

int fail_hip(lins_ctx* ctx, hipError_t e, const char* what) {
  if (ctx) ctx->hip_err = std::string(what) + ": " + hipGetErrorString(e);
  return LINS_E_HIP;
}
#define HIP_TRY(ctx, expr)                          \
  do {                                              \
    hipError_t e__ = (expr);                        \
    if (e__ != hipSuccess) return fail_hip(ctx, e__, #expr); \
  } while (0)

inline size_t align4(size_t n) { return (n + 3) & ~size_t(3); }

void pipe_free(lins_ctx* ctx) {
  auto& q = ctx->pipe;
  if (q.s_comm) (void)hipStreamSynchronize(q.s_comm), (void)hipStreamDestroy(q.s_comm);
  for (int k = 0; k < 2; ++k) {
    if (q.ev_comm[k]) (void)hipEventDestroy(q.ev_comm[k]);
  }
  q = lins_ctx::Pipe{};
}

void rccl_free(lins_ctx* ctx) {
  auto& r = ctx->rccl;
  if (r.comm && r.comm_destroy) (void)r.comm_destroy(r.comm);
  if (r.lib) (void)dlclose(r.lib);
  r = lins_ctx::Rccl{};
}

// Everything the side streams of the pipelined mode still have in flight is ordered before what is enqueued on the
// main stream next (no host wait).  Called by every staged entry point that touches buffers the side streams read.
// Order the context's stream behind whatever the second launch queue still runs, and mark that queue as behind the
// context's stream (the next split run forks again).  Called by every entry point that enqueues on ctx->stream or reads
// what the update kernels wrote; lins_batch_run() itself does not join (see lins_ctx::stream2).
int split_join(lins_ctx* ctx) {
  ctx->split_dirty = true;
  if (ctx->split_pending) {
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->hist1b[ctx->split_h], 0));
    ctx->split_pending = false;
  }
  return LINS_OK;
}

int pipe_join(lins_ctx* ctx) {
  if (int rc = split_join(ctx)) return rc;
  auto& q = ctx->pipe;
  for (int k = 0; k < 2; ++k) {
    if (q.comm_pending[k]) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, q.ev_comm[k], 0));
    q.comm_pending[k] = false;
  }
  return LINS_OK;
}


// input contract: finite fields, int(intensity) in [0, LINS_MAX_RING) — the relative-time
// fraction may be slightly negative (SE:631-650 produces -0.025..0.125), and C truncation
// maps (-1, 0) to ring 0 exactly as the reference's int() does; reports ring-sortedness
// (packed 16-byte points: the arena's own layout — also what a strided cloud is checked as after it was gathered there)
int check_cloud(const lins_point* p, int n, bool* sorted) {
  int prev = -1;
  bool s = true;  // "grid-able": ring-sorted and every ring id < 16 (binned search precondition)
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(p[i].x) || !std::isfinite(p[i].y) || !std::isfinite(p[i].z) || !std::isfinite(p[i].intensity))
      return LINS_E_INPUT;
    if (p[i].intensity <= -1.f || p[i].intensity >= (float)LINS_MAX_RING) return LINS_E_INPUT;
    int r = (int)p[i].intensity;
    if (r < prev || r >= 16) s = false;
    prev = r;
  }
  if (sorted) *sorted = s;
  return LINS_OK;
}

void make_dev_params(const lins_params& p, int search, DevParams& d) {
  d.num_iter = p.num_iter;
  d.icp_freq = p.icp_freq;
  d.fixed_iters = p.fixed_iters;
  d.search = search;
  d.r2 = p.lidar_std * p.lidar_std;
  d.lidar_scale = p.lidar_scale;
  d.inv_period = (double)(1.f / p.scan_period);  // (1.f / SCAN_PERIOD), SE:1067
  d.nearest = p.nearest_sq_dist;
  d.nearest_f = (float)p.nearest_sq_dist;
  d.pad = 0;
  d.margin_cold = 0.20f;  // (metres; swept on the batch workload after the late iterations got cheaper: 0.10 / 0.04 -> 0.789 ms, 0.20 / 0.08 -> 0.771 ms)
  d.margin_warm = 0.08f;
  d.reseed_drift = 0.15f;  // (metres; any value gives the same results: it only picks between two bounds of an exact search)
  d.pad2 = 0;
  // Tuning / profiling knobs, honoured only when LINS_ENABLE_DEBUG_KNOBS=1 is set as well: a stray variable in a
  // production environment changes nothing.  The margins only trade search work for certificate hits (any value
  // >= 0 gives the same results); LINS_DEBUG_SKIP deliberately breaks the searches (profiling aid).
  const char* gate = std::getenv("LINS_ENABLE_DEBUG_KNOBS");
  if (gate && gate[0] == '1') {
    if (const char* e = std::getenv("LINS_MARGIN_COLD")) d.margin_cold = std::max(0.f, (float)std::atof(e));
    if (const char* e = std::getenv("LINS_MARGIN_WARM")) d.margin_warm = std::max(0.f, (float)std::atof(e));
    if (const char* e = std::getenv("LINS_RESEED_DRIFT")) d.reseed_drift = std::max(0.f, (float)std::atof(e));
    if (const char* e = std::getenv("LINS_DEBUG_SKIP")) d.pad = std::atoi(e);  // 1 = skip walks, 2 = skip search, 8 = verify
  }
}

// "auto": one workgroup per CU is all a small batch can use — the 1024-thread kernel gives each
// scan the shortest critical path; beyond that the multi-resident kernel keeps two scans per CU.
// The 3-lane shape is the single-round kernel: query sets beyond its 336 slots (more than a VLP-16
// front-end can emit) take the 1-lane shapes, whose several-rounds path is the tested one.
int effective_search(const lins_ctx* ctx, int n) {
  int s = ctx->dprm.search;
  if (s == SEARCH_AUTO) s = n > ctx->n_cu ? (int)SEARCH_MR : (int)SEARCH_LDS3;
  if (s == SEARCH_LDS3 && !ctx->lds3_ok) s = SEARCH_LDS;
  return s;
}

void streams_free(lins_ctx* ctx) {
  auto& t = ctx->st;
  (void)hipFree(t.d_arena), (void)hipFree(t.d_sorted), (void)hipFree(t.d_desc), (void)hipFree(t.d_jobs), (void)hipFree(t.d_desc_next);
  t.d_desc_next = nullptr, t.index_ready = false;
  (void)hipFree(t.d_gsorted), (void)hipFree(t.d_gridtab);
  t = lins_ctx::Streams{};
}

void fe_free(lins_ctx* ctx) {
  auto& f = ctx->fe;
  void* ptrs[] = {f.d_scans, f.d_cloud, f.d_out, f.d_range, f.d_col, f.d_ground, f.d_picks, f.d_counts};
  for (void* p : ptrs) (void)hipFree(p);
  void* sg[] = {f.d_raw, f.d_raws, f.d_cellidx, f.d_segrows, f.d_outliers};
  for (void* p : sg) (void)hipFree(p);
  (void)hipHostFree(f.h_raw);
  (void)hipHostFree(f.h_cloud), (void)hipHostFree(f.h_range), (void)hipHostFree(f.h_col), (void)hipHostFree(f.h_ground);
  f = lins_ctx::Frontend{};
}

// Run fn(k) for k in [0, n) on up to 16 host threads (validation + packing of a batch is memory-bound
// scalar work: 1024 scans = 8 M points); returns the smallest-index non-zero result.
template <class F>
int parallel_scans(int n, F fn) {
  const unsigned hw = std::thread::hardware_concurrency();
  const int T = std::max(1, std::min({16, (int)(hw ? hw : 1), n / 8}));
  std::vector<int> rc(n, 0);
  if (T <= 1) {
    for (int k = 0; k < n; ++k) rc[k] = fn(k);
  } else {
    std::atomic<int> next{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t)
      pool.emplace_back([&] {
        for (int k; (k = next.fetch_add(1)) < n;) rc[k] = fn(k);
      });
    for (auto& th : pool) th.join();
  }
  for (int k = 0; k < n; ++k)
    if (rc[k]) return rc[k];
  return 0;
}

// The pipelined form: a pool of host threads runs fn(k) for k = 0, 1, 2 ... ; as soon as every item of a chunk
// [lo, hi) is done, the CALLING thread runs ready(lo, hi) (queue the chunk's copy, its kernels) while the pool is
// already packing the next chunks.  Chunks are `chunk` items, the last one takes the remainder (< 2 chunks).  Returns
// the first non-zero result of fn (smallest index of the chunk that saw it) or of ready; later chunks are abandoned.
template <class F, class R>
int pack_pipelined(int n, int chunk, F fn, R ready) {
  if (n <= 0) return 0;
  const int n_chunks = std::max(1, n / chunk);
  auto chunk_of = [&](int k) { return std::min(k / chunk, n_chunks - 1); };
  std::vector<int> rcs(n, 0);
  std::unique_ptr<std::atomic<int>[]> done(new std::atomic<int>[n_chunks]);
  for (int c = 0; c < n_chunks; ++c) done[c].store(0);
  std::atomic<int> next{0};
  std::atomic<bool> stop{false};
  const unsigned hw = std::thread::hardware_concurrency();
  const int T = std::max(1, std::min({16, (int)(hw ? hw : 1) - 1, n}));
  std::vector<std::thread> pool;
  for (int t = 0; t < T; ++t)
    pool.emplace_back([&] {
      for (int k; !stop.load(std::memory_order_relaxed) && (k = next.fetch_add(1)) < n;) {
        rcs[k] = fn(k);
        done[chunk_of(k)].fetch_add(1, std::memory_order_release);
      }
    });
  int rc = 0;
  for (int c = 0; c < n_chunks && !rc; ++c) {
    const int lo = c * chunk, hi = c + 1 == n_chunks ? n : lo + chunk;
    while (done[c].load(std::memory_order_acquire) < hi - lo) std::this_thread::yield();
    for (int k = lo; k < hi && !rc; ++k) rc = rcs[k];
    if (!rc) rc = ready(lo, hi);
  }
  stop.store(true);
  for (auto& th : pool) th.join();
  return rc;
}

// stage times of a call on stderr (LINS_ENABLE_DEBUG_KNOBS=1 and LINS_BATCH_TRACE set)
struct CallTrace {
  bool on = false;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  CallTrace() {
    const char* g = std::getenv("LINS_ENABLE_DEBUG_KNOBS");
    on = g && g[0] == '1' && std::getenv("LINS_BATCH_TRACE");
  }
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
  void mark(const char* what) const {
    if (on) std::fprintf(stderr, "  [trace] %-28s %.3f ms\n", what, ms());
  }
};

struct RangeFlags {  // which kernel families the scans of a range can take
  bool lds_ok = true, mr_ok = true, lds3_ok = true;
};

// pass 1 (serial, cheap): argument checks and the arena layout of the whole batch
int layout_batch(lins_ctx* ctx, int n, const lins_scan_pair* in, size_t* arena_used, size_t* slots_used, uint64_t* bytes_iter) {
  if (!ctx || !in || n < 0) return LINS_E_ARG;
  if (n > ctx->max_batch) return LINS_E_CAPACITY;
  size_t off = 0, slots = 0;
  uint64_t bytes = 0;
  for (int s = 0; s < n; ++s) {
    const lins_scan_pair& p = in[s];
    if (p.n_surf_flat < 0 || p.n_corner_sharp < 0 || p.n_surf_last < 0 || p.n_corner_last < 0) return LINS_E_ARG;
    if (p.point_stride_bytes != 0 && p.point_stride_bytes != 16 && p.point_stride_bytes != 32) return LINS_E_ARG;
    if ((p.n_surf_flat && !p.surf_flat) || (p.n_corner_sharp && !p.corner_sharp) ||
        (p.n_surf_last && !p.surf_less_flat_last) || (p.n_corner_last && !p.corner_less_sharp_last))
      return LINS_E_ARG;
    if (p.n_surf_flat > LINS_MAX_QUERY || p.n_corner_sharp > LINS_MAX_QUERY) return LINS_E_CAPACITY;
    if (p.n_surf_last > ctx->max_targets || p.n_corner_last > ctx->max_targets) return LINS_E_CAPACITY;
    ScanDesc& d = ctx->h_desc[s];
    const int cnt[4] = {p.n_surf_flat, p.n_corner_sharp, p.n_surf_last, p.n_corner_last};
    int offs[4];
    for (int c = 0; c < 4; ++c) {
      if (off + align4(cnt[c]) > ctx->arena_cap) return LINS_E_CAPACITY;
      offs[c] = (int)off;
      off += align4(cnt[c]);
    }
    d.off_surf_q = offs[0], d.n_surf_q = cnt[0];
    d.off_corner_q = offs[1], d.n_corner_q = cnt[1];
    d.off_surf_t = offs[2], d.n_surf_t = cnt[2];
    d.off_corner_t = offs[3], d.n_corner_t = cnt[3];
    d.slot_base = (int)slots;
    d.pad = 0;
    slots += cnt[0] + cnt[1];
    if (slots > ctx->slot_cap) return LINS_E_CAPACITY;
    bytes += 16ull * (cnt[0] + cnt[1] + cnt[2] + cnt[3]) + 8 * 19 + 8 * 28;
  }
  *arena_used = off, *slots_used = slots, *bytes_iter = bytes;
  return LINS_OK;
}

// pass 2 for one scan: input contract + packing into the pinned staging arena
int pack_one(lins_ctx* ctx, const lins_scan_pair* in, int s) {
  const lins_scan_pair& p = in[s];
  ScanDesc& d = ctx->h_desc[s];
  bool ss = true, cs = true;
  int r;
  // The clouds go to the pinned staging arena first — a copy for packed points, a gather of the 16 payload bytes for
  // pcl::PointXYZI arrays (point_stride_bytes 32), nothing at all for clouds the caller already wrote there
  // (lins_batch_map) — and are validated where they then lie.
  const lins_point* src[4] = {p.surf_flat, p.corner_sharp, p.surf_less_flat_last, p.corner_less_sharp_last};
  const int cnt[4] = {d.n_surf_q, d.n_corner_q, d.n_surf_t, d.n_corner_t};
  const int offs[4] = {d.off_surf_q, d.off_corner_q, d.off_surf_t, d.off_corner_t};
  for (int c = 0; c < 4; ++c) {
    lins_point* dst = reinterpret_cast<lins_point*>(ctx->h_arena + offs[c]);
    // (a cloud that lies in the staging arena but not where THIS layout wants it was mapped for another batch shape:
    // moving it would race with the packing of its neighbours — refused, lins_batch_map's contract is same n, same sizes)
    if (cnt[c] && src[c] != dst && reinterpret_cast<const float4*>(src[c]) >= ctx->h_arena &&
        reinterpret_cast<const float4*>(src[c]) < ctx->h_arena + ctx->arena_cap)
      return LINS_E_ARG;
    // (a cloud that already lies at its arena slot is packed 16-byte points by construction — lins_batch_map hands out
    // lins_point arrays; a pair that claims the 32-byte stride for it would be misread in silence: refused)
    if (cnt[c] && src[c] == dst && p.point_stride_bytes == 32) return LINS_E_ARG;
    if (cnt[c] && src[c] != dst) {
      if (p.point_stride_bytes == 32)
        for (int i = 0; i < cnt[c]; ++i) dst[i] = lins_point_load(src[c], 32, i);
      else
        std::memcpy(dst, src[c], sizeof(lins_point) * cnt[c]);
    }
    for (size_t k2 = cnt[c]; k2 < align4(cnt[c]); ++k2) ctx->h_arena[offs[c] + k2] = make_float4(0, 0, 0, 0);
  }
  const lins_point* at[4];
  for (int c = 0; c < 4; ++c) at[c] = reinterpret_cast<const lins_point*>(ctx->h_arena + offs[c]);
  if ((r = check_cloud(at[0], cnt[0], nullptr))) return r;
  if ((r = check_cloud(at[1], cnt[1], nullptr))) return r;
  if ((r = check_cloud(at[2], cnt[2], &ss))) return r;
  if ((r = check_cloud(at[3], cnt[3], &cs))) return r;
  d.surf_sorted = ss, d.corner_sorted = cs;
  std::memcpy(ctx->h_state + (size_t)s * 19, p.state, sizeof p.state);
  std::memcpy(ctx->h_cov + (size_t)s * 324, p.cov, sizeof p.cov);
  return 0;
}

// kernel eligibility of the packed scans [lo, hi)
RangeFlags range_flags(const lins_ctx* ctx, int lo, int hi) {
  RangeFlags fl;
  for (int s = lo; s < hi; ++s) {
    const ScanDesc& d = ctx->h_desc[s];
    const bool grid = d.surf_sorted && d.corner_sorted;
    if (!grid || d.n_surf_t + d.n_corner_t > lds_np_cap()) fl.lds_ok = false;
    if (!grid || d.n_surf_t + d.n_corner_t > lds_mr_np_cap()) fl.mr_ok = false;
    if (d.n_surf_q + d.n_corner_q > 336) fl.lds3_ok = false;  // (16 waves x 21 query slots = the VLP-16 caps, 144 flat + 192 sharp)
  }
  return fl;
}

// search index of scans [lo, lo + cnt) of the uploaded descriptors, on the context's stream (grid kernels only: scans
// that cannot take them run the any-size kernel, which bins for itself)
int build_index_range(lins_ctx* ctx, int lo, int cnt, const RangeFlags& fl) {
  if (cnt <= 0 || !(fl.lds_ok || fl.mr_ok)) return LINS_OK;
  launch_grid_index(ctx->stream, cnt, ctx->d_desc + lo, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab + lo);
  HIP_TRY(ctx, hipGetLastError());
  return LINS_OK;
}

// host -> device of scans [lo, hi) (their arena slice is contiguous), asynchronous on `st`
int h2d_range(lins_ctx* ctx, int lo, int hi, size_t arena_end, hipStream_t st) {
  if (hi <= lo) return LINS_OK;
  const size_t a0 = (size_t)ctx->h_desc[lo].off_surf_q;
  if (arena_end > a0)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_arena + a0, ctx->h_arena + a0, (arena_end - a0) * sizeof(float4), hipMemcpyHostToDevice, st));
  if (lo == 0 && hi == ctx->max_batch) {  // the whole context: priors and descriptors are one block (lins_ctx::h_meta)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_meta_in, ctx->h_meta, ctx->meta_in_bytes, hipMemcpyHostToDevice, st));
    return LINS_OK;
  }
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_desc + lo, ctx->h_desc + lo, (size_t)(hi - lo) * sizeof(ScanDesc), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state_in + (size_t)lo * 19, ctx->h_state + (size_t)lo * 19, (size_t)(hi - lo) * 19 * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cov_in + (size_t)lo * 324, ctx->h_cov + (size_t)lo * 324, (size_t)(hi - lo) * 324 * 8, hipMemcpyHostToDevice, st));
  return LINS_OK;
}

// The second launch queue of a context (lins_set_launch_queues): created when a batch beyond the workgroup slots is uploaded —
// not inside the first run that uses it, where the stream and its 2 x 64 timing events cost that run a millisecond or more
// (round 6: the bench's queued stop-rule figure read 1.12 instead of 0.89 ms for it) — and, as a fallback, by that run.
int split_prepare(lins_ctx* ctx) {
  if (ctx->stream2) return LINS_OK;
  // A priority of its own: HIP multiplexes the streams of a process onto a handful of hardware queues (four by default) in
  // creation order, and two streams that share one are served in order — measured: a context whose two streams collided
  // ran its queued steps at 0.646 instead of 0.50 ms, depending on how many other contexts the process had created
  // (gpurun r06w).  Streams of different priority never share a hardware queue.  LOW, so that the work a caller puts on
  // streams of his own is not pushed back by it.
  int pr_least = 0, pr_greatest = 0;
  HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
  HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, pr_least));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  for (int k = 0; k < lins_ctx::kHist; ++k) {
    HIP_TRY(ctx, hipEventCreate(&ctx->hist0b[k]));
    HIP_TRY(ctx, hipEventCreate(&ctx->hist1b[k]));
  }
  return LINS_OK;
}

void set_batch_state(lins_ctx* ctx, int n, const RangeFlags& fl, size_t slots, uint64_t bytes) {
  ctx->n_uploaded = n;
  ctx->lds_ok = fl.lds_ok, ctx->mr_ok = fl.mr_ok, ctx->lds3_ok = fl.lds3_ok;
  ctx->slots_uploaded = slots;
  ctx->ran = false;
  ctx->bytes_per_iter = bytes;
}

// Launch order of a batch on the multi-resident kernel: 1024 workgroups on 512 slots is two "rounds", and the dispatcher
// hands workgroups out in index order — so the launch ends when the slowest pairing of an early and a late workgroup
// does.  Listing the scans longest-expected-first (LPT) lets the short ones fill the end.  What the host knows before
// the launch: cloud sizes (R^2 = 0.004 against measured workgroup times — useless) and the prior; the prior's
// translation |p| (= how far the clouds are apart before the first iteration, hence how many re-searches the first
// iterations need) correlates 0.40.  Measured on the batch workload (tools/wg_cost_model.py, list-scheduling model on
// measured per-workgroup times: as submitted 843 us, by |p| 731 us, by the true durations 726 us, perfectly divisible
// work 583 us).  Results do not depend on the order (one workgroup per scan, no cross-scan state).
void launch_order(lins_ctx* ctx, int n) {
  std::vector<std::pair<double, int>> key(n);
  for (int s = 0; s < n; ++s) {
    const double* st = ctx->h_state + (size_t)s * 19;
    double k2 = -(st[0] * st[0] + st[1] * st[1] + st[2] * st[2]);
    if (!(k2 == k2)) k2 = 0.0;  // (a NaN prior is the caller's business, not a reason to hand std::sort an unordered key)
    key[s] = {k2, s};
  }
  std::sort(key.begin(), key.end());
  for (int s = 0; s < n; ++s) ctx->h_order[s] = key[s].second;
  ctx->relay_list_parts = 0;  // (the item list of the several-part updates is rebuilt by the next run that needs it)
}

// The number of the next launch of an update kernel.  It tags the entries of the walk cache (16 bits of it: an entry of
// any earlier launch — other clouds, other priors — never matches), so the cache is cleared when those 16 bits come round
// again, not per upload or per step (the per-step clear of lins_streams_step was 33 MB per 1024 streams).
int next_run_gen(lins_ctx* ctx) {
  ++ctx->run_gen;
  if ((ctx->run_gen & 0xFFFF) == 0 && ctx->d_walk_cache) (void)hipMemsetAsync(ctx->d_walk_cache, 0xFF, ctx->slot_cap * 32, ctx->stream);
  return ctx->run_gen;
}

// Several-part updates of a launch of n scans on the batch kernel: the cuts, the launch's number, the list of its
// (scan, part) items on the device — every part 0 in launch order, then every part 1, ... — and the ticket counters and
// flags (RelayArgs; ieskf_lds_impl.h "work items").  `listed`: the launch order of these n scans is on the device.
size_t queue_ints(const lins_ctx* ctx) {  // counters, one flag per scan, the debug trace (8 ints per workgroup, <= 15 per scan)
  return (size_t)lds_mr_queue_flags_offset() + (size_t)ctx->max_batch * (1 + 15 * 8);
}
int relay_prepare(lins_ctx* ctx, int n, bool ordered, RelayArgs& ra) {
  ra.at = ctx->relay_at, ra.cuts = ctx->relay_cuts;
  ra.parts = relay_max_parts(ctx->prm.num_iter, ra.at, ra.cuts);
  if (ctx->relay_gen >= (1 << 26)) {  // (flags are 16 gen + part: start over long before the int runs out)
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_queue, 0, queue_ints(ctx) * sizeof(int), ctx->stream));
    ctx->relay_gen = 0;
  }
  if (ctx->relay_list_parts != ra.parts || ctx->relay_list_n != n) {
    int* list = ctx->h_order + ctx->max_batch;
    for (int p = 0; p < ra.parts; ++p)
      for (int k = 0; k < n; ++k) list[p * n + k] = (ordered ? ctx->h_order[k] : k) | (p << 27);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order + ctx->max_batch, list, (size_t)ra.parts * n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ctx->relay_list_parts = ra.parts, ctx->relay_list_n = n;
  }
  ra.gen = ++ctx->relay_gen, ra.spins = ctx->relay_spins, ra.cap = ctx->max_batch, ra.slots = ctx->queue_grid;
  ra.hdr = ctx->d_relay_hdr, ra.lane = ctx->d_relay_lane, ra.queue = ctx->d_queue, ra.err = ctx->h_relay_err;
  return LINS_OK;
}

// (wait = false: the caller synchronises the stream itself before it returns to its own caller — the single-call entry
// points, whose download waits anyway: one host wait per call instead of two)
int upload(lins_ctx* ctx, int n, const lins_scan_pair* in, bool wait = true) {
  {  // (pipelined mode: the side streams may still read the inputs this call replaces)
    int rcj = pipe_join(ctx);
    if (rcj) return rcj;
  }
  const CallTrace tr;  // (stage times on stderr: LINS_ENABLE_DEBUG_KNOBS=1 LINS_BATCH_TRACE=1)
  size_t off = 0, slots = 0;
  uint64_t bytes = 0;
  int rc = layout_batch(ctx, n, in, &off, &slots, &bytes);
  if (rc) return rc;
  tr.mark("upload: layout");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if ((rc = parallel_scans(n, [&](int s) { return pack_one(ctx, in, s); }))) return rc;
  tr.mark("upload: validate + pack");
  const RangeFlags fl = range_flags(ctx, 0, n);
  tr.mark("upload: range flags");
  if ((rc = h2d_range(ctx, 0, n, off, ctx->stream))) return rc;
  tr.mark("upload: copies queued");
  // the target clouds have arrived: their search index (the reference builds its kd-trees where it produces the
  // clouds, SE:1156-1160, not in performIESKF)
  // (timed by its own events for lins_last_index_ms — at the staged lins_batch_upload only: in the single-call entry points,
  // which a live filter waits for, two event records are ~10 us of in-order latency on the stream, tools/experiments/graph_latency.hip)
  if (wait) HIP_TRY(ctx, hipEventRecord(ctx->ev_idx0, ctx->stream));
  if ((rc = build_index_range(ctx, 0, n, fl))) return rc;
  if (wait) HIP_TRY(ctx, hipEventRecord(ctx->ev_idx1, ctx->stream));
  ctx->idx_timed = wait;
  tr.mark("upload: index queued");
  launch_order(ctx, n);
  if (ctx->max_batch > 1)  // (a one-scan context: the order is [0], which is what the array holds since lins_create)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order, ctx->h_order, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (wait) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->split_mode && n > ctx->queue_grid)  // (a batch whose queued runs go out on two launch queues: the second one exists before the first run)
    if (int rcq = split_prepare(ctx)) return rcq;
  set_batch_state(ctx, n, fl, slots, bytes);
  return LINS_OK;
}

// The kernels of scans [lo, lo + cnt) of the uploaded batch on the context's stream (no events, no state)
// (`n_total`: the batch the range belongs to — "auto" picks the kernel family by the batch, so that a scan's bits do
// not depend on how the batch was cut)
int run_range(lins_ctx* ctx, int lo, int cnt, int n_total, const RangeFlags& fl, lins_pose_record* poses, int32_t scan_id_base,
              hipStream_t st = nullptr) {
  if (!st) st = ctx->stream;
  int s = ctx->dprm.search;
  if (s == SEARCH_AUTO) s = n_total > ctx->n_cu ? (int)SEARCH_MR : (int)SEARCH_LDS3;
  if (s == SEARCH_LDS3 && !fl.lds3_ok) s = SEARCH_LDS;
  const bool want_lds = s >= SEARCH_LDS, want_mr = s == SEARCH_MR;
  const bool use_mr = want_mr && fl.mr_ok, use_lds = want_lds && !want_mr && fl.lds_ok;
  ctx->last_search = use_mr ? (int)SEARCH_MR : (use_lds ? s : (want_lds ? (int)SEARCH_BINNED : s));
  const ScanDesc* desc = ctx->d_desc + lo;
  const double *st_in = ctx->d_state_in + (size_t)lo * 19, *cov_in = ctx->d_cov_in + (size_t)lo * 324;
  double *st_out = ctx->d_state_out + (size_t)lo * 19, *cov_out = ctx->d_cov_out + (size_t)lo * 324, *a6 = ctx->d_a6 + (size_t)lo * 21;
  void* out = (char*)ctx->d_out + (size_t)lo * out_rec_size();
  lins_pose_record* ps = poses ? poses + lo : nullptr;
  if (use_mr || use_lds) {
    if (use_mr)
      launch_lds_mr(st, cnt, ctx->dprm, desc, nullptr, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab + lo, st_in, cov_in, st_out, a6, cov_out, out, ctx->d_idx, ps,
                    scan_id_base + lo, nullptr, nullptr, ctx->d_walk_cache, next_run_gen(ctx), ctx->d_relay_lane + (size_t)lo * kLaneIntsPerScan);
    else
      launch_lds(st, cnt, ctx->dprm, s == SEARCH_LDS3 ? 3 : 1, desc, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab + lo, st_in, cov_in, st_out, a6, cov_out, out,
                 ctx->d_idx, ps, scan_id_base + lo, nullptr, ctx->d_relay_lane + (size_t)lo * kLaneIntsPerScan);  // (the Joseph update is the kernels' epilogue)
  } else {
    DevParams dp = ctx->dprm;
    dp.search = want_lds ? (int)SEARCH_BINNED : s;  // a scan does not fit LDS: global-memory grid
    launch_persistent(st, cnt, dp, desc, ctx->d_arena, st_in, cov_in, st_out, cov_out, a6, out, ctx->d_idx, ps,
                      scan_id_base + lo, ctx->d_binned, nullptr);
  }
  HIP_TRY(ctx, hipGetLastError());
  return LINS_OK;
}

// After a host wait that follows a launch of the batch kernel: did a part of a several-part update give up waiting for its
// hand-over (KernelArgs::relay_err)?  Nothing was written for that scan then — its result buffers hold an earlier launch's
// values — so EVERY call that hands results to the caller after a wait checks here (lins_sync, lins_batch_download, the
// streams steps, the single-call updates), not only lins_sync.  The word is cleared: the error is reported once,
// by the call whose launch it belongs to.
int relay_check(lins_ctx* ctx) {
  if (!ctx->h_relay_err || !*ctx->h_relay_err) return LINS_OK;
  ctx->hip_err = "several-part update: a part's wait for its hand-over ran out (a workgroup of the launch was lost)";
  ctx->queue_timeouts += *ctx->h_relay_err;
  *ctx->h_relay_err = 0;
  (void)hipMemset(ctx->d_queue, 0, queue_ints(ctx) * sizeof(int));  // (counters and flags start over)
  ctx->relay_gen = 0;
  return LINS_E_HIP;
}

}  // namespace

extern "C" {

const char* lins_strerror(int code) {
  switch (code) {
    case LINS_OK: return "ok";
    case LINS_E_ARG: return "bad argument";
    case LINS_E_HIP: return "HIP runtime error (see lins_last_hip_error)";
    case LINS_E_CAPACITY: return "batch or cloud exceeds the context capacity";
    case LINS_E_INPUT: return "cloud violates the input contract (non-finite value or ring id out of range)";
    case LINS_E_NODEVICE: return "no usable gfx950 device";
    case LINS_E_STATE: return "call sequence error";
    case LINS_E_UNSUPPORTED: return "input cannot take the requested device path";
    default: return "unknown error";
  }
}

const char* lins_last_hip_error(const lins_ctx* ctx) { return ctx ? ctx->hip_err.c_str() : ""; }

int lins_create(const lins_params* params, int device, int max_batch, int max_targets, lins_ctx** out) {
  if (!params || !out || max_batch < 1 || max_targets < 1) return LINS_E_ARG;
  if (params->num_iter < 1 || params->icp_freq < 1 || !(params->scan_period > 0)) return LINS_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return LINS_E_NODEVICE;
  lins_ctx* ctx = new (std::nothrow) lins_ctx();
  if (!ctx) return LINS_E_ARG;
  ctx->device = device;
  ctx->prm = *params;
  make_dev_params(*params, SEARCH_AUTO, ctx->dprm);  // (ineligible clouds fall back to the exact exhaustive paths)
  if (const char* g = std::getenv("LINS_ENABLE_DEBUG_KNOBS"))
    if (g[0] == '1') {
      if (const char* e = std::getenv("LINS_LAUNCH_ORDER")) ctx->use_order = e[0] != '0';
      if (const char* e = std::getenv("LINS_COMM_PRIO")) ctx->comm_default_prio = std::atoi(e) == 0;
      if (const char* e = std::getenv("LINS_SPLIT_STREAMS")) ctx->split_mode = std::atoi(e) == 0 ? 0 : (std::atoi(e) >= 2 ? 3 : 1);  // (0: one launch; 1: when runs are queued; 2: always)
      if (std::getenv("LINS_RELAY_AT") || std::getenv("LINS_RELAY_MASK") || std::getenv("LINS_RELAY_CUTS")) ctx->split_mode = 0;  // (the one-launch form's knobs)
      if (const char* e = std::getenv("LINS_RELAY_AT")) ctx->relay_at = std::max(0, std::atoi(e));  // (0: whole updates)
      if (const char* e = std::getenv("LINS_RELAY_CUTS")) ctx->relay_cuts = std::max(1, std::min(14, std::atoi(e)));
      if (const char* e = std::getenv("LINS_RELAY_MASK")) {  // (cuts that are not evenly spaced: bit i = a part ends before iteration i)
        const long m = std::strtol(e, nullptr, 0) & 0x7FFFFFFEl;
        if (m && __builtin_popcountl(m) <= 14) ctx->relay_at = -1, ctx->relay_cuts = (int)m;
      }
      if (const char* e = std::getenv("LINS_RELAY_SPINS")) ctx->relay_spins = std::max(0, std::atoi(e));
      if (const char* e = std::getenv("LINS_QUEUE_GRID")) ctx->queue_grid = std::max(1, std::atoi(e));  // (batches beyond this many scans are cut)
      if (const char* e = std::getenv("LINS_STREAMS_FUSE")) ctx->streams_fuse = e[0] != '0';  // (0: re-projection and index build as two kernels)
      if (const char* e = std::getenv("LINS_RUN_GEN0")) ctx->run_gen = std::atoi(e);  // (test aid: the walk cache's 16-bit wrap on a chosen launch)
    }
  ctx->max_batch = max_batch;
  ctx->max_targets = max_targets;
  ctx->arena_cap = (size_t)max_batch * (2 * align4(max_targets) + 2 * LINS_MAX_QUERY);
  ctx->slot_cap = (size_t)max_batch * LINS_MAX_QUERY;
  if (ctx->arena_cap >= (size_t)1 << 31 || ctx->slot_cap >= (size_t)1 << 31) {  // ScanDesc offsets are 32-bit
    delete ctx;
    return LINS_E_CAPACITY;
  }
#define CREATE_TRY(expr)                             \
  do {                                               \
    hipError_t e__ = (expr);                         \
    if (e__ != hipSuccess) {                         \
      fprintf(stderr, "lins_create: %s: %s\n", #expr, hipGetErrorString(e__)); \
      lins_destroy(ctx);                             \
      return LINS_E_HIP;                             \
    }                                                \
  } while (0)
  CREATE_TRY(hipSetDevice(device));
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) ctx->n_cu = ncu;
  }
  CREATE_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  CREATE_TRY(hipEventCreate(&ctx->ev0));
  CREATE_TRY(hipEventCreate(&ctx->ev1));
  CREATE_TRY(hipEventCreate(&ctx->ev2));
  for (int k = 0; k < lins_ctx::kHist; ++k) {
    CREATE_TRY(hipEventCreate(&ctx->hist0[k]));
    CREATE_TRY(hipEventCreate(&ctx->hist1[k]));
  }
  const size_t nb = (size_t)max_batch;
  CREATE_TRY(hipHostMalloc((void**)&ctx->h_arena, ctx->arena_cap * sizeof(float4)));
  const auto up64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
  const size_t m_cov = up64(nb * 19 * 8), m_out = m_cov + up64(nb * 324 * 8), m_desc = m_out + up64(nb * std::max(sizeof(OutRecHost), out_rec_size()));
  ctx->meta_out_bytes = m_desc, ctx->meta_in_bytes = m_desc + up64(nb * sizeof(ScanDesc));
  CREATE_TRY(hipHostMalloc((void**)&ctx->h_meta, ctx->meta_in_bytes));
  ctx->h_state = (double*)ctx->h_meta, ctx->h_cov = (double*)(ctx->h_meta + m_cov);
  ctx->h_out = (OutRecHost*)(ctx->h_meta + m_out), ctx->h_desc = (ScanDesc*)(ctx->h_meta + m_desc);
  CREATE_TRY(hipHostMalloc((void**)&ctx->h_order, 16 * nb * sizeof(int)));  // (n entries: launch order; from max_batch on: parts x n items)
  CREATE_TRY(hipMalloc((void**)&ctx->d_order, 16 * nb * sizeof(int)));
  CREATE_TRY(hipMemsetAsync(ctx->d_order, 0, 16 * nb * sizeof(int), ctx->stream));
  CREATE_TRY(hipMalloc((void**)&ctx->d_arena, ctx->arena_cap * sizeof(float4)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_binned, ctx->arena_cap * sizeof(float4)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_gsorted, ctx->arena_cap * sizeof(float4)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_gridtab, (size_t)ctx->max_batch * sizeof(GridTables)));
  if (ctx->queue_grid <= 0) ctx->queue_grid = lds_mr_resident_workgroups(ctx->n_cu);
  // the carry records of the batch kernel's queries (ieskf_lds_lean.h: tracked candidates and certificates between the
  // iterations of an update; 32 KB per scan): every launch of that kernel uses them, cut into parts or not
  CREATE_TRY(hipMalloc((void**)&ctx->d_relay_lane, (size_t)ctx->max_batch * kLaneIntsPerScan * sizeof(int)));
  CREATE_TRY(hipMemset(ctx->d_relay_lane, 0xFF, (size_t)ctx->max_batch * kLaneIntsPerScan * sizeof(int)));  // (empty records)
  if (ctx->max_batch > ctx->queue_grid && lds_mr_has_parts()) {  // (only batches beyond the device's workgroup slots are cut into parts)
    CREATE_TRY(hipMalloc((void**)&ctx->d_relay_hdr, (size_t)ctx->max_batch * 64 * sizeof(double)));
    CREATE_TRY(hipHostMalloc((void**)&ctx->h_relay_err, sizeof(int)));
    *ctx->h_relay_err = 0;
    CREATE_TRY(hipMalloc((void**)&ctx->d_queue, queue_ints(ctx) * sizeof(int)));
    CREATE_TRY(hipMemset(ctx->d_queue, 0, queue_ints(ctx) * sizeof(int)));
  } else {
    ctx->relay_at = 0;
  }
  CREATE_TRY(hipEventCreate(&ctx->ev_idx0));
  CREATE_TRY(hipEventCreate(&ctx->ev_idx1));
  CREATE_TRY(hipMalloc((void**)&ctx->d_meta_in, ctx->meta_in_bytes));
  CREATE_TRY(hipMalloc((void**)&ctx->d_meta_out, ctx->meta_out_bytes));
  ctx->d_state_in = (double*)ctx->d_meta_in, ctx->d_cov_in = (double*)(ctx->d_meta_in + m_cov), ctx->d_desc = (ScanDesc*)(ctx->d_meta_in + m_desc);
  ctx->d_state_out = (double*)ctx->d_meta_out, ctx->d_cov_out = (double*)(ctx->d_meta_out + m_cov), ctx->d_out = ctx->d_meta_out + m_out;
  CREATE_TRY(hipMalloc((void**)&ctx->d_lin, nb * 19 * 8));
  CREATE_TRY(hipMalloc((void**)&ctx->d_a6, nb * 21 * 8));
  CREATE_TRY(hipMalloc((void**)&ctx->d_idx, ctx->slot_cap * sizeof(int4)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_walk_cache, ctx->slot_cap * 32));
  CREATE_TRY(hipMemset(ctx->d_walk_cache, 0xFF, ctx->slot_cap * 32));
  CREATE_TRY(hipMalloc((void**)&ctx->d_dump, 2 * LINS_MAX_QUERY * sizeof(lins_corr)));
  CREATE_TRY(hipMalloc((void**)&ctx->d_sums, nb * 28 * 8));
  CREATE_TRY(hipMalloc((void**)&ctx->d_counts, nb * 2 * sizeof(int)));
#undef CREATE_TRY
  static_assert(sizeof(OutRecHost) == 48, "OutRec layout");
  *out = ctx;
  return LINS_OK;
}

void lins_destroy(lins_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  (void)hipHostFree(ctx->h_arena);
  (void)hipHostFree(ctx->h_meta);  // (h_state, h_cov, h_out, h_desc)
  (void)hipHostFree(ctx->h_order), (void)hipFree(ctx->d_order);
  (void)hipFree(ctx->d_arena);
  (void)hipFree(ctx->d_binned);
  (void)hipFree(ctx->d_gsorted);
  (void)hipFree(ctx->d_gridtab);
  (void)hipFree(ctx->d_relay_hdr), (void)hipFree(ctx->d_relay_lane), (void)hipFree(ctx->d_queue), (void)hipHostFree(ctx->h_relay_err);
  if (ctx->ev_idx0) (void)hipEventDestroy(ctx->ev_idx0);
  if (ctx->ev_idx1) (void)hipEventDestroy(ctx->ev_idx1);
  (void)hipFree(ctx->d_meta_in), (void)hipFree(ctx->d_meta_out);  // (d_state_in, d_cov_in, d_desc; d_state_out, d_cov_out, d_out)
  (void)hipFree(ctx->d_lin);
  (void)hipFree(ctx->d_a6);
  (void)hipFree(ctx->d_prof);
  (void)hipFree(ctx->d_aux);
  (void)hipFree(ctx->d_jobs);
  fe_free(ctx);
  streams_free(ctx);
  if (ctx->map_state && ctx->map_state_free) ctx->map_state_free(ctx->map_state);
  (void)hipFree(ctx->d_idx);
  (void)hipFree(ctx->d_walk_cache);
  (void)hipFree(ctx->d_dump);
  (void)hipFree(ctx->d_sums);
  (void)hipFree(ctx->d_counts);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
  if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  for (int k = 0; k < lins_ctx::kHist; ++k) {
    if (ctx->hist0b[k]) (void)hipEventDestroy(ctx->hist0b[k]);
    if (ctx->hist1b[k]) (void)hipEventDestroy(ctx->hist1b[k]);
    if (ctx->hist0[k]) (void)hipEventDestroy(ctx->hist0[k]);
    if (ctx->hist1[k]) (void)hipEventDestroy(ctx->hist1[k]);
  }
  pipe_free(ctx);
  rccl_free(ctx);
  if (ctx->ev_copy) (void)hipEventDestroy(ctx->ev_copy);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int lins_set_search(lins_ctx* ctx, const char* mode) {
  if (!ctx || !mode) return LINS_E_ARG;
  if (!std::strcmp(mode, "brute"))
    ctx->dprm.search = SEARCH_BRUTE;
  else if (!std::strcmp(mode, "binned"))
    ctx->dprm.search = SEARCH_BINNED;
  else if (!std::strcmp(mode, "lds"))  // LDS-resident grid, 1024 threads, 3 lanes per query
    ctx->dprm.search = SEARCH_LDS3;
  else if (!std::strcmp(mode, "lds1"))  // LDS-resident grid, 384 threads, 1 lane per query
    ctx->dprm.search = SEARCH_LDS;
  else if (!std::strcmp(mode, "mr"))  // multi-resident: part of the grid in LDS, 2 scans per CU
    ctx->dprm.search = SEARCH_MR;
  else if (!std::strcmp(mode, "auto"))  // "mr" for batches larger than the CU count, "lds" otherwise
    ctx->dprm.search = SEARCH_AUTO;
  else
    return LINS_E_ARG;
  return LINS_OK;
}

/* The kernel family the last batch (or pass) actually ran: the requested mode after "auto" and the eligibility
 * fall-backs were applied; "" before the first run. */
const char* lins_last_search(const lins_ctx* ctx) {
  if (!ctx) return "";
  switch (ctx->last_search) {
    case SEARCH_BRUTE: return "brute";
    case SEARCH_BINNED: return "binned";
    case SEARCH_LDS: return "lds1";
    case SEARCH_LDS3: return "lds";
    case SEARCH_MR: return "mr";
    default: return "";
  }
}

int lins_batch_upload(lins_ctx* ctx, int n, const lins_scan_pair* in) { return upload(ctx, n, in); }

/* The context's pinned staging arena, laid out for a batch of n scans with the given cloud sizes: clouds[4 s + c] is
 * where cloud c (0 surf_flat, 1 corner_sharp, 2 surf_less_flat_last, 3 corner_less_sharp_last) of scan s belongs, as
 * packed 16-byte points.  A caller that WRITES its clouds there (e.g. its feature extraction's output) and passes those
 * very pointers in the lins_scan_pair array of the next lins_batch_upload / lins_ieskf_update(_batch) call skips the
 * library's copy into the staging arena altogether: the points are validated where they lie and sent.                */
int lins_batch_map(lins_ctx* ctx, int n, const int32_t* counts, lins_point** clouds) {
  if (!ctx || n < 0 || (n && (!counts || !clouds))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;  // (nothing to lay out: the header allows n >= 0)
  {  // (the side streams of the pipelined mode / an earlier asynchronous run may still read the arena's device copy — not
     // the pinned one: every upload waits for its own copies; nothing to join here)
  }
  std::vector<lins_scan_pair> shape((size_t)n);
  lins_point* const some = reinterpret_cast<lins_point*>(ctx->h_arena);  // (layout_batch only checks for null)
  for (int s = 0; s < n; ++s) {
    lins_scan_pair& p = shape[s];
    std::memset(&p, 0, offsetof(lins_scan_pair, state));
    p.n_surf_flat = counts[4 * s], p.n_corner_sharp = counts[4 * s + 1], p.n_surf_last = counts[4 * s + 2], p.n_corner_last = counts[4 * s + 3];
    p.surf_flat = p.corner_sharp = p.surf_less_flat_last = p.corner_less_sharp_last = some;
  }
  size_t off = 0, slots = 0;
  uint64_t bytes = 0;
  int rc = layout_batch(ctx, n, shape.data(), &off, &slots, &bytes);
  if (rc) return rc;
  ctx->n_uploaded = 0, ctx->ran = false;  // (the descriptors of whatever was uploaded are gone)
  for (int s = 0; s < n; ++s) {
    const ScanDesc& d = ctx->h_desc[s];
    const int offs[4] = {d.off_surf_q, d.off_corner_q, d.off_surf_t, d.off_corner_t};
    for (int c = 0; c < 4; ++c) clouds[4 * s + c] = reinterpret_cast<lins_point*>(ctx->h_arena + offs[c]);
  }
  return LINS_OK;
}

int lins_last_cut(const lins_ctx* ctx, int* parts, int* queue_timeouts) {
  if (!ctx || !parts || !queue_timeouts) return LINS_E_ARG;
  if (!ctx->ran) return LINS_E_STATE;
  *parts = ctx->last_parts;
  *queue_timeouts = (int)std::min<long long>(ctx->queue_timeouts, 0x7FFFFFFF);
  return LINS_OK;
}

/* HIP-event time (ms) of the search-index build of the last upload (grid_index_kernel over every scan of the batch:
 * the device counterpart of the reference's kd-tree build, setInputCloud in updatePointCloud, SE:1156-1160); 0 when
 * the batch cannot take the grid kernels (nothing was built).                                                       */
int lins_last_index_ms(lins_ctx* ctx, float* ms) {
  if (!ctx || !ms) return LINS_E_ARG;
  *ms = 0.f;
  if (!ctx->idx_timed) return LINS_E_STATE;
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_idx1));
  HIP_TRY(ctx, hipEventElapsedTime(ms, ctx->ev_idx0, ctx->ev_idx1));
  return LINS_OK;
}

int lins_batch_run(lins_ctx* ctx, void* d_poses, int32_t scan_id_base) {
  if (!ctx) return LINS_E_ARG;
  if (ctx->n_uploaded <= 0) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto& q = ctx->pipe;
  const int set = q.on ? (int)(q.runs & 1u) : 0;
  double* const a6 = ctx->d_a6;
  void* const out = ctx->d_out;
  const bool wait_comm = q.on && q.comm_pending[set];
  if (wait_comm) {  // this run rewrites the pose buffer the gather of run k - 2 read
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, q.ev_comm[set], 0));
    q.comm_pending[set] = false;
  }
  if (q.on) q.run_split[set] = false;
  const int h = (int)(ctx->hist_n % lins_ctx::kHist);
  HIP_TRY(ctx, hipEventRecord(ctx->hist0[h], ctx->stream));
  const int search = effective_search(ctx, ctx->n_uploaded);
  const bool want_lds = search >= SEARCH_LDS, want_mr = search == SEARCH_MR;
  const bool use_mr = want_mr && ctx->mr_ok, use_lds = want_lds && !want_mr && ctx->lds_ok;
  ctx->last_search = use_mr ? (int)SEARCH_MR : (use_lds ? search : (want_lds ? (int)SEARCH_BINNED : search));
  // Several-part updates (the kernel's relay + work queue): when the batch has more scans than the device has workgroup
  // slots, a launch of one workgroup per scan ends with slots idle while the last whole updates finish; cut every relay_at
  // iterations the same work is several times as many shorter jobs, pulled from the launch's queue by as many persistent
  // workgroups as are resident at once, and that end shrinks.  Not with the phase profile (one record per scan), and
  // only with ICP_FREQ 1: with a larger one the iterations in between read the triplets an earlier part of the scan left in
  // idx_store — plain stores of another workgroup, possibly on another XCD.
  const bool cut_ok = use_mr && ctx->n_uploaded > ctx->queue_grid && !ctx->d_prof && ctx->prm.icp_freq == 1 && ctx->d_relay_hdr;
  // Two launch queues (lins_ctx::stream2): launches of <= queue_grid scans, whole updates, dealt alternately to the two
  // streams.  Not with the phase profile (one launch) or the pipelined gather mode (its events follow ONE stream);
  // split_mode 0 (lins_set_launch_queues, LINS_SPLIT_STREAMS=0) selects the one-launch form with its several-part updates.
  // ... and in the default mode (2) only when the caller is QUEUING runs — the run before this one is still in flight: a run
  // issued into an idle context is one launch with several-part updates, the shorter of the two forms for a run that is
  // waited for (room batch, 1024 scans x 10 iterations: 0.57 against 0.63 ms; queued back to back: 0.56 against 0.505 ms
  // per run — tools/split_launch_time.py).  Mode 3 (LINS_SPLIT_STREAMS=2) always takes the two queues.
  bool queued = ctx->split_mode >= 3;
  if (!queued && ctx->split_mode && ctx->hist_n > 0 && use_mr && ctx->n_uploaded > ctx->queue_grid) {  // (asked only where the answer matters)
    const int hp = (int)((ctx->hist_n - 1) % lins_ctx::kHist);
    queued = hipEventQuery(ctx->hist1[hp]) == hipErrorNotReady || (ctx->hist_split[hp] && hipEventQuery(ctx->hist1b[hp]) == hipErrorNotReady);
    (void)hipGetLastError();  // (hipErrorNotReady is an answer, not an error to keep)
  }
  const bool split = use_mr && queued && ctx->n_uploaded > ctx->queue_grid && !ctx->d_prof;
  const bool relay = !split && cut_ok && ctx->relay_at != 0 && relay_max_parts(ctx->prm.num_iter, ctx->relay_at, ctx->relay_cuts) > 1;
  RelayArgs ra;
  if (relay) {
    const int rcq = relay_prepare(ctx, ctx->n_uploaded, ctx->use_order, ra);
    if (rcq) return rcq;
  }
  ctx->last_parts = relay ? ra.parts : 1;
  ctx->hist_split[h] = split;
  // (a run that goes out on the context's stream alone after one that used the second queue — lins_set_launch_queues(1) or
  // another kernel family chosen between two queued runs — is ordered behind that queue: same scans, same scratch records)
  if (!split && ctx->split_pending)
    if (int rcs = split_join(ctx)) return rcs;
  if (split) {
    if (int rcq = split_prepare(ctx)) return rcq;
    const int n = ctx->n_uploaded, n_launch = (n + ctx->queue_grid - 1) / ctx->queue_grid, per = (n + n_launch - 1) / n_launch;
    if (ctx->d_walk_cache && (ctx->run_gen & 0xFFFF) + n_launch > 0xFFFF) {
      // the launch numbers of this run would come round in their low 16 bits (the walk cache's tags): next_run_gen's clear on
      // the context's stream would not be ordered against the second queue's launches — the cache is cleared HERE instead,
      // behind both queues and ahead of every launch of the run (the fork below), and the run starts the new round of numbers
      if (int rcs = split_join(ctx)) return rcs;
      HIP_TRY(ctx, hipMemsetAsync(ctx->d_walk_cache, 0xFF, ctx->slot_cap * 32, ctx->stream));
      ctx->run_gen = (ctx->run_gen | 0xFFFF) + 1;
    }
    if (ctx->split_dirty) {  // (uploads, index builds, downloads since the last fork: the second queue starts behind them)
      HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
      ctx->split_dirty = false;
    }
    RangeFlags fl;
    fl.lds_ok = ctx->lds_ok, fl.mr_ok = ctx->mr_ok, fl.lds3_ok = ctx->lds3_ok;
    if (wait_comm) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream2, q.ev_comm[set], 0));  // (the second queue writes that pose buffer too)
    HIP_TRY(ctx, hipEventRecord(ctx->hist0b[h], ctx->stream2));
    for (int c = 0; c < n_launch; ++c) {
      const int lo = c * per, cnt = std::min(per, n - lo);
      const int rcr = run_range(ctx, lo, cnt, n, fl, (lins_pose_record*)d_poses, scan_id_base, (c & 1) ? ctx->stream2 : ctx->stream);
      if (rcr) return rcr;
    }
    ctx->last_parts = 1;
    HIP_TRY(ctx, hipEventRecord(ctx->hist1[h], ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->hist1b[h], ctx->stream2));
    ctx->split_pending = true, ctx->split_h = h;
    if (q.on) q.run_split[set] = true, q.h_of[set] = h;  // (pipelined gather mode: the pose records of this run are complete when BOTH queues are through)
  } else if (use_mr || use_lds) {
    ctx->split_dirty = true;  // (a launch on the context's stream the second queue is not ordered behind)
    if (use_mr)
      launch_lds_mr(ctx->stream, ctx->n_uploaded, ctx->dprm, ctx->d_desc,
                    relay ? ctx->d_order + ctx->max_batch : (ctx->use_order ? ctx->d_order : nullptr), ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab, ctx->d_state_in,
                    ctx->d_cov_in, ctx->d_state_out, a6, ctx->d_cov_out, out, ctx->d_idx, (lins_pose_record*)d_poses,
                    scan_id_base, ctx->d_prof, relay ? &ra : nullptr, ctx->d_walk_cache, next_run_gen(ctx), ctx->d_relay_lane);
    else
      launch_lds(ctx->stream, ctx->n_uploaded, ctx->dprm, search == SEARCH_LDS3 ? 3 : 1, ctx->d_desc,
                 ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab, ctx->d_state_in, ctx->d_cov_in, ctx->d_state_out, a6, ctx->d_cov_out, out, ctx->d_idx,
                 (lins_pose_record*)d_poses, scan_id_base, ctx->d_prof, ctx->d_relay_lane);
    HIP_TRY(ctx, hipEventRecord(ctx->hist1[h], ctx->stream));
    if (q.on) q.h_of[set] = h;  // (the pose records of this run are complete at hist1[h])
    // (The Joseph update, SE:594-598, is the update kernel's epilogue since round 3: ieskf_lds_impl.h joseph_epilogue.
    // Rounds 1-2 launched ieskf_joseph_kernel here, ~20 us + a launch per run; a side stream for it — measured at normal
    // and at lowest stream priority — lets its 1024 small workgroups sit on the LDS and wave slots the NEXT run's update
    // kernel needs for its second resident workgroup: that kernel then takes 0.86 instead of 0.71 ms.)
  } else {
    ctx->split_dirty = true;
    DevParams dp = ctx->dprm;
    dp.search = want_lds ? (int)SEARCH_BINNED : search;  // a scan does not fit LDS: global-memory grid
    launch_persistent(ctx->stream, ctx->n_uploaded, dp, ctx->d_desc, ctx->d_arena, ctx->d_state_in, ctx->d_cov_in,
                      ctx->d_state_out, ctx->d_cov_out, a6, out, ctx->d_idx,
                      (lins_pose_record*)d_poses, scan_id_base, ctx->d_binned, ctx->d_prof);
    HIP_TRY(ctx, hipEventRecord(ctx->hist1[h], ctx->stream));
    if (q.on) q.h_of[set] = h;
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->hist_n++;
  if (q.on) q.runs++;
  ctx->ran = true;
  return LINS_OK;
}

/* Pipelined staged mode (off by default).  With it on, lins_pose_allgather() leaves the exchange of a run's pose
 * records on the context's communication stream, so that it travels beside the kernels of the NEXT lins_batch_run().
 * The caller alternates two pose-record buffers (run k -> buffer k & 1) and may enqueue any number of runs before ONE
 * lins_sync(), which waits for everything.  Only the staged calls (upload / run / pose_allgather / sync / download /
 * total_iters / kernel-time queries) may be used while it is on; each of them re-joins the streams where it must.  */
int lins_set_pipelined(lins_ctx* ctx, int on) {
  if (!ctx) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto& q = ctx->pipe;
  if (on && !q.s_comm) {
    // A priority of its own (the highest; the second launch queue has the lowest, the context's stream the default): streams of
    // one priority may share a hardware queue, and a gather that waits for BOTH launch queues of run k on the queue that also
    // carries run k + 1's first launch holds that launch back until run k is through — the two launch queues then overlap
    // nothing (forced on one GPU: 18.9 M it/s against 19.5 without the gather, gpurun r06p).  The gather is ~10 us of work.
    int pr_least = 0, pr_greatest = 0;
    HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest));
    HIP_TRY(ctx, hipStreamCreateWithPriority(&q.s_comm, hipStreamNonBlocking, (ctx->comm_default_prio ? 0 : pr_greatest)));
    for (int k = 0; k < 2; ++k) {
      HIP_TRY(ctx, hipEventCreateWithFlags(&q.ev_comm[k], hipEventDisableTiming));
    }
  }
  int rc = pipe_join(ctx);
  if (rc) return rc;
  q.on = on != 0;
  return LINS_OK;
}

int lins_set_launch_queues(lins_ctx* ctx, int queues) {
  if (!ctx || (queues != 1 && queues != 2)) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rc = pipe_join(ctx)) return rc;
  ctx->split_mode = queues == 2 ? 1 : 0;
  return LINS_OK;
}

/* GPU time (ms) from the start of the first to the end of the last of the last n lins_batch_run() calls (both launch
 * queues): what n queued runs took on the device, launches overlapping or not.  Waits for the newest of them.        */
int lins_runs_span_ms(lins_ctx* ctx, int n, float* ms) {
  if (!ctx || !ms || n < 1 || n > lins_ctx::kHist || (unsigned)n > ctx->hist_n) return LINS_E_ARG;
  const int h0 = (int)((ctx->hist_n - n) % lins_ctx::kHist);
  float best = 0.f;
  for (int k = 0; k < n; ++k) {  // (ends are not ordered across the two queues: the latest of all)
    const int h = (int)((ctx->hist_n - n + k) % lins_ctx::kHist);
    float t = 0.f;
    HIP_TRY(ctx, hipEventSynchronize(ctx->hist1[h]));
    HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->hist0[h0], ctx->hist1[h]));
    best = std::max(best, t);
    if (ctx->hist_split[h]) {
      HIP_TRY(ctx, hipEventSynchronize(ctx->hist1b[h]));
      HIP_TRY(ctx, hipEventElapsedTime(&t, ctx->hist0[h0], ctx->hist1b[h]));
      best = std::max(best, t);
    }
  }
  *ms = best;
  return LINS_OK;
}

/* per launch of the last n runs: its duration by the events of its own queue (ms; 2 per run with two queues, the second
 * 0 for a one-launch run): out[2 k], out[2 k + 1] */
int lins_launch_ms_history(lins_ctx* ctx, int n, float* ms) {
  if (!ctx || !ms || n < 1 || n > lins_ctx::kHist || (unsigned)n > ctx->hist_n) return LINS_E_ARG;
  for (int k = 0; k < n; ++k) {
    const int h = (int)((ctx->hist_n - n + k) % lins_ctx::kHist);
    HIP_TRY(ctx, hipEventSynchronize(ctx->hist1[h]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms[2 * k], ctx->hist0[h], ctx->hist1[h]));
    ms[2 * k + 1] = 0.f;
    if (ctx->hist_split[h]) {
      HIP_TRY(ctx, hipEventSynchronize(ctx->hist1b[h]));
      HIP_TRY(ctx, hipEventElapsedTime(&ms[2 * k + 1], ctx->hist0b[h], ctx->hist1b[h]));
    }
  }
  return LINS_OK;
}

/* HIP-event times (ms) of the update kernels of the last n lins_batch_run() calls, oldest first (n <= 64 and <= the
 * runs so far); waits for the newest of them.                                                                       */
int lins_kernel_ms_history(lins_ctx* ctx, int n, float* ms) {
  if (!ctx || !ms || n < 0 || n > lins_ctx::kHist || (unsigned)n > ctx->hist_n) return LINS_E_ARG;
  for (int k = 0; k < n; ++k) {
    const int h = (int)((ctx->hist_n - n + k) % lins_ctx::kHist);
    HIP_TRY(ctx, hipEventSynchronize(ctx->hist1[h]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms[k], ctx->hist0[h], ctx->hist1[h]));
    if (ctx->hist_split[h]) {  // (two launch queues: the run = from its first launch's start to its last launch's end)
      float b = 0.f;
      HIP_TRY(ctx, hipEventSynchronize(ctx->hist1b[h]));
      HIP_TRY(ctx, hipEventElapsedTime(&b, ctx->hist0[h], ctx->hist1b[h]));
      ms[k] = std::max(ms[k], b);
    }
  }
  return LINS_OK;
}

/* ---- RCCL pose gather (ncclAllGather of the 192-byte pose records over xGMI) -------------
 * librccl is dlopen()ed on first use — the one already in the process (e.g. PyTorch's) when there is one — and never
 * linked: a build without RCCL still loads, and these calls return LINS_E_UNSUPPORTED.                            */
static int rccl_load(lins_ctx* ctx) {
  auto& r = ctx->rccl;
  if (r.lib) return LINS_OK;
  // The RCCL that belongs to the HIP runtime this library is running on: streams and events are runtime objects, so a
  // librccl bound to ANOTHER copy of libamdhip64 (a Python process may hold PyTorch's bundled ROCm beside the system's)
  // cannot take ours.  Look next to the runtime that resolved our own HIP calls first, then fall back to the loader.
  void* lib = nullptr;
  Dl_info info;
  if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &info) && info.dli_fname) {
    std::string dir(info.dli_fname);
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos) {
      dir.resize(slash + 1);
      lib = dlopen((dir + "librccl.so.1").c_str(), RTLD_NOW | RTLD_LOCAL);
      if (!lib) lib = dlopen((dir + "librccl.so").c_str(), RTLD_NOW | RTLD_LOCAL);
    }
  }
  if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!lib) return LINS_E_UNSUPPORTED;
  r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(dlsym(lib, "ncclGetUniqueId"));
  r.comm_init_rank = reinterpret_cast<decltype(r.comm_init_rank)>(dlsym(lib, "ncclCommInitRank"));
  r.all_gather = reinterpret_cast<decltype(r.all_gather)>(dlsym(lib, "ncclAllGather"));
  r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(lib, "ncclCommDestroy"));
  r.get_error_string = reinterpret_cast<decltype(r.get_error_string)>(dlsym(lib, "ncclGetErrorString"));
  if (!r.get_unique_id || !r.comm_init_rank || !r.all_gather || !r.comm_destroy) {
    (void)dlclose(lib);
    r = lins_ctx::Rccl{};
    return LINS_E_UNSUPPORTED;
  }
  r.lib = lib;
  return LINS_OK;
}
static int rccl_fail(lins_ctx* ctx, ncclResult_t e, const char* what) {
  ctx->hip_err = std::string(what) + ": " + (ctx->rccl.get_error_string ? ctx->rccl.get_error_string(e) : "RCCL error");
  return LINS_E_HIP;
}

/* id128: LINS_RCCL_ID_BYTES bytes, made by ONE rank and handed to the others by whatever bootstrap the application has. */
int lins_rccl_unique_id(lins_ctx* ctx, void* id128) {
  if (!ctx || !id128) return LINS_E_ARG;
  int rc = rccl_load(ctx);
  if (rc) return rc;
  ncclUniqueId id;
  ncclResult_t e = ctx->rccl.get_unique_id(&id);
  if (e != ncclSuccess) return rccl_fail(ctx, e, "ncclGetUniqueId");
  static_assert(sizeof(id) == LINS_RCCL_ID_BYTES, "ncclUniqueId");
  std::memcpy(id128, &id, sizeof id);
  return LINS_OK;
}

int lins_rccl_init(lins_ctx* ctx, const void* id128, int rank, int world) {
  if (!ctx || !id128 || world < 1 || rank < 0 || rank >= world) return LINS_E_ARG;
  if (ctx->rccl.comm) return LINS_E_STATE;
  int rc = rccl_load(ctx);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof id);
  ncclResult_t e = ctx->rccl.comm_init_rank(&ctx->rccl.comm, world, id, rank);
  if (e != ncclSuccess) return rccl_fail(ctx, e, "ncclCommInitRank");
  ctx->rccl.rank = rank, ctx->rccl.world = world;
  return LINS_OK;
}

/* All-gather of fixed-size pieces: every rank contributes n_records pose records at d_local (device), d_all (device)
 * receives world x n_records records in rank order.  Stream-ordered after the last lins_batch_run(): in pipelined mode
 * on the context's communication stream (beside the next run), otherwise on the compute stream.  No host wait.     */
int lins_pose_allgather(lins_ctx* ctx, const void* d_local, int n_records, void* d_all) {
  if (!ctx || !d_local || !d_all || n_records < 0) return LINS_E_ARG;
  if (!ctx->rccl.comm) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  auto& q = ctx->pipe;
  hipStream_t st = ctx->stream;
  int set = 0;
  if (q.on) {
    if (q.runs == 0) return LINS_E_STATE;
    set = (int)((q.runs - 1) & 1u);  // the run whose records these are
    HIP_TRY(ctx, hipStreamWaitEvent(q.s_comm, ctx->hist1[q.h_of[set]], 0));
    if (q.run_split[set]) HIP_TRY(ctx, hipStreamWaitEvent(q.s_comm, ctx->hist1b[q.h_of[set]], 0));  // (both launch queues; the queues themselves are not joined)
    st = q.s_comm;
  } else if (int rcs = split_join(ctx)) {  // (the gather runs on the context's stream: behind the second launch queue too)
    return rcs;
  }
  ncclResult_t e = ctx->rccl.all_gather(d_local, d_all, (size_t)n_records * sizeof(lins_pose_record), ncclChar, ctx->rccl.comm, st);
  if (e != ncclSuccess) return rccl_fail(ctx, e, "ncclAllGather");
  if (q.on) {
    HIP_TRY(ctx, hipEventRecord(q.ev_comm[set], q.s_comm));
    q.comm_pending[set] = true;
  }
  return LINS_OK;
}

int lins_rccl_destroy(lins_ctx* ctx) {
  if (!ctx) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->pipe.s_comm) HIP_TRY(ctx, hipStreamSynchronize(ctx->pipe.s_comm));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  rccl_free(ctx);
  return LINS_OK;
}

/* Debug aid (unit tests of the device math against the oracle; see debug_kernels.hip for the op codes):
 * evaluates op on n items of n_in doubles each, n_out doubles out per item. */
int lins_debug_math(lins_ctx* ctx, int op, int n, const double* in, int n_in, double* out, int n_out) {
  if (ctx && in && out && op >= 100 && op <= 111 && n >= 1 && n_in >= 9 && n_out == 2) {  // cycle microbenchmarks, n blocks
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    double *d_in = nullptr, *d_out = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d_in, 9 * 8));
    HIP_TRY(ctx, hipMalloc((void**)&d_out, (size_t)n * 2 * 8));
    HIP_TRY(ctx, hipMemcpy(d_in, in, 9 * 8, hipMemcpyHostToDevice));
    launch_debug_cycles(ctx->stream, op, n, d_in, d_out);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, d_out, (size_t)n * 2 * 8, hipMemcpyDeviceToHost));
    (void)hipFree(d_in), (void)hipFree(d_out);
    return LINS_OK;
  }
  static const int kIn[20] = {4, 3, 3, 37, 38, 4, 24, 42, 42, 448, 448, 42, 42, 3, 4, 4, 43, 43, 72, 72};
  static const int kOut[20] = {3, 4, 9, 19, 18, 12, 3, 6, 6, 28, 28, 6, 6, 4, 3, 12, 6, 6, 44, 44};
  if (!ctx || !in || !out || op < 0 || op > 19 || n < 0 || n_in != kIn[op] || n_out != kOut[op]) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  double *d_in = nullptr, *d_out = nullptr;
  void* d_lm = nullptr;
  HIP_TRY(ctx, hipMalloc((void**)&d_in, (size_t)n * n_in * 8));
  hipError_t e = hipMalloc((void**)&d_out, (size_t)n * n_out * 8);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, (size_t)n * n_in * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    if (op == 9 || op == 10)
      launch_debug_reduce_rows(ctx->stream, op, n, d_in, d_out);
    else if (op == 8 || op == 12)
      launch_debug_wave_solve(ctx->stream, n, op == 12, d_in, d_out);
    else if (op == 16 || op == 17)
      launch_debug_icp_gn(ctx->stream, n, op == 17, d_in, d_out);
    else if (op == 18 || op == 19) {  // lm_step_from_sums: one thread (lm_math.h) / over a wave (lm_wave.h); 72 in, 44 out
      e = hipMalloc(&d_lm, (size_t)n * map_carry_size());
      if (e == hipSuccess) launch_debug_lm_step(ctx->stream, n, op == 19, d_in, d_out, d_lm);
    }
    else
      launch_debug_math(ctx->stream, op, n, n_in, n_out, d_in, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * n_out * 8, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(d_in), (void)hipFree(d_out), (void)hipFree(d_lm);
  if (e != hipSuccess) return fail_hip(ctx, e, "lins_debug_math");
  return LINS_OK;
}

/* Debug aid (not part of the drop-in surface; tests/test_gpu_context_state.py): read (write = 0) or write (write = 1)
 * `bytes` bytes at `offset_bytes` of the context's scratch state that outlives a run — which = 0: the carry records of
 * the batch kernel (ieskf_lds_lean.h, kLaneIntsPerScan ints per scan), 1: the walk cache (32 B per query slot).
 * Synchronous, ordered behind both launch queues and the gather stream. */
int lins_debug_scratch(lins_ctx* ctx, int which, int write, size_t offset_bytes, size_t bytes, void* host) {
  if (!ctx || !host || (which != 0 && which != 1)) return LINS_E_ARG;
  char* const base = which == 0 ? reinterpret_cast<char*>(ctx->d_relay_lane) : reinterpret_cast<char*>(ctx->d_walk_cache);
  const size_t cap = which == 0 ? (size_t)ctx->max_batch * kLaneIntsPerScan * sizeof(int) : ctx->slot_cap * 32;
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
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_prof, (size_t)ctx->max_batch * 80 * sizeof(long long)));
    HIP_TRY(ctx, hipMemset(ctx->d_prof, 0, (size_t)ctx->max_batch * 80 * sizeof(long long)));
  }
  if (out && ctx->d_prof) {
    if (n_scans > ctx->max_batch) return LINS_E_CAPACITY;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out, ctx->d_prof, (size_t)n_scans * 16 * sizeof(long long), hipMemcpyDeviceToHost));
  }
  if (!enable && ctx->d_prof) {
    (void)hipFree(ctx->d_prof);
    ctx->d_prof = nullptr;
  }
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

// device buffers of the front-end for n scans (inputs, scratch, and the default output buffer d_out)
static int fe_alloc(lins_ctx* ctx, int n) {
  auto& f = ctx->fe;
  if (f.cap >= n) return LINS_OK;
  fe_free(ctx);
  const size_t c = (size_t)n, N = LINS_CLOUD_MAX;
  HIP_TRY(ctx, hipMalloc(&f.d_scans, c * sizeof(FeScanHost)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_cloud, c * N * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_range, c * N * sizeof(float)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_col, c * N * sizeof(unsigned)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_ground, c * N));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_picks, c * fe_pick_stride() * sizeof(int)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_out, c * (192 + 1920 + 384 + N) * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&f.d_counts, c * 4 * sizeof(int)));
  f.cap = n;
  return LINS_OK;
}

static int fe_launch(lins_ctx* ctx, int n, double scan_period, float4* out_base, std::vector<int>& counts, uint64_t bytes);

// Front-end stage shared by lins_extract_features_batch and lins_streams_step: validate, upload the
// segmented scans, launch frontend_kernel with the feature clouds going to out_base + offs[k][0..3]
// (sharp, less sharp, flat, less flat), bring the four counts per scan back (synchronises).
static int fe_run(lins_ctx* ctx, int n, const lins_segmented_scan* in, double scan_period, float4* out_base,
                  const long long (*offs)[4], std::vector<int>& counts) {
  static_assert(sizeof(FeScanHost) == 192, "FeScan layout");
  if (fe_scan_size() != sizeof(FeScanHost)) return LINS_E_STATE;
  const size_t N = LINS_CLOUD_MAX;
  // pass 1 (serial): argument checks, packed layout (each scan's arrays start on a multiple of 4 points)
  std::vector<FeScanHost> hs(n);
  size_t total = 0;
  uint64_t bytes = 0;
  for (int k = 0; k < n; ++k) {
    const lins_segmented_scan& s = in[k];
    if (s.n < 0 || s.n > (int)N || (s.n && (!s.cloud || !s.range || !s.col || !s.ground))) return LINS_E_ARG;
    for (int r = 0; r < LINS_LINE_NUM; ++r)  // a sector must fit the per-wave sort network (a VLP-16 ring: <= 300)
      if ((s.end_ring[r] - s.start_ring[r]) / 6 + 2 > 510) return LINS_E_UNSUPPORTED;
    hs[k].off = (long long)total, hs[k].n = s.n, hs[k].pad = 0;
    for (int r = 0; r < LINS_LINE_NUM; ++r) hs[k].start_ring[r] = s.start_ring[r], hs[k].end_ring[r] = s.end_ring[r];
    hs[k].start_ori = s.start_ori, hs[k].end_ori = s.end_ori, hs[k].ori_diff = s.ori_diff;
    hs[k].o_sharp = offs[k][0], hs[k].o_less_sharp = offs[k][1], hs[k].o_flat = offs[k][2], hs[k].o_less_flat = offs[k][3];
    total += align4(s.n);
    bytes += (uint64_t)s.n * 25;
  }
  int rc0 = fe_alloc(ctx, n);
  if (rc0) return rc0;
  auto& f = ctx->fe;
  if (f.h_cap < total) {
    (void)hipHostFree(f.h_cloud), (void)hipHostFree(f.h_range), (void)hipHostFree(f.h_col), (void)hipHostFree(f.h_ground);
    f.h_cloud = nullptr, f.h_range = nullptr, f.h_col = nullptr, f.h_ground = nullptr, f.h_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_cloud, total * sizeof(float4)));
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_range, total * sizeof(float)));
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_col, total * sizeof(unsigned)));
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_ground, total));
    f.h_cap = total;
  }
  // pass 2 (host pool): input contract + packing into the pinned staging; every complete chunk of scans is sent
  // while the next ones are being packed
  const int rcv = pack_pipelined(
      n, 64,
      [&](int k) -> int {
        const lins_segmented_scan& s = in[k];
        const size_t o = (size_t)hs[k].off;
        for (int i = 0; i < s.n; ++i) {
          const lins_point& p = s.cloud[i];
          if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z) || !std::isfinite(p.intensity) ||
              !std::isfinite(s.range[i]) || s.col[i] >= (uint32_t)LINS_SCAN_NUM)
            return LINS_E_INPUT;
        }
        if (s.n) {
          std::memcpy(f.h_cloud + o, s.cloud, s.n * sizeof(float4));
          std::memcpy(f.h_range + o, s.range, s.n * sizeof(float));
          std::memcpy(f.h_col + o, s.col, s.n * sizeof(unsigned));
          std::memcpy(f.h_ground + o, s.ground, s.n);
        }
        return 0;
      },
      [&](int lo, int hi) -> int {
        const size_t a = (size_t)hs[lo].off, cnt = (hi < n ? (size_t)hs[hi].off : total) - a;
        if (!cnt) return 0;
        HIP_TRY(ctx, hipMemcpyAsync(f.d_cloud + a, f.h_cloud + a, cnt * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(f.d_range + a, f.h_range + a, cnt * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(f.d_col + a, f.h_col + a, cnt * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(f.d_ground + a, f.h_ground + a, cnt, hipMemcpyHostToDevice, ctx->stream));
        return 0;
      });
  if (rcv) {
    (void)hipStreamSynchronize(ctx->stream);  // (copies of earlier chunks may still read the staging)
    return rcv;
  }
  HIP_TRY(ctx, hipMemcpyAsync(f.d_scans, hs.data(), (size_t)n * sizeof(FeScanHost), hipMemcpyHostToDevice, ctx->stream));
  return fe_launch(ctx, n, scan_period, out_base, counts, bytes);
}

// the front-end kernel over the n scans described by f.d_scans (filled by the host path above or by the
// segmentation kernel); brings the four counts per scan back (synchronises)
static int fe_launch(lins_ctx* ctx, int n, double scan_period, float4* out_base, std::vector<int>& counts, uint64_t bytes) {
  auto& f = ctx->fe;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  launch_frontend(ctx->stream, n, f.d_scans, f.d_cloud, f.d_range, f.d_col, f.d_ground, scan_period, f.d_picks, out_base,
                  f.d_counts);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  counts.resize((size_t)n * 4);
  HIP_TRY(ctx, hipMemcpyAsync(counts.data(), f.d_counts, counts.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&f.ms, ctx->ev0, ctx->ev2));
  for (int k = 0; k < n; ++k) {
    if (counts[(size_t)k * 4 + 3] < 0) return LINS_E_UNSUPPORTED;  // a ring beyond the voxel sort network
    bytes += 16ull * (counts[k * 4] + counts[k * 4 + 1] + counts[k * 4 + 2] + counts[k * 4 + 3]);
  }
  f.bytes = bytes;
  return LINS_OK;
}

// image_projection stage on the device: n raw clouds -> the front-end's device input buffers (f.d_cloud /
// d_range / d_col / d_ground at k * LINS_CLOUD_MAX) and the head of each FeScan (n, ring indices, orientations);
// offs = where the front-end will later put the four feature clouds of each scan
static int sg_run(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw, const long long (*offs)[4]) {
  static_assert(sizeof(SgRawHost) == 16, "SgRaw layout");
  if (sg_raw_size() != sizeof(SgRawHost)) return LINS_E_STATE;
  const size_t N = LINS_CLOUD_MAX;
  size_t total = 0;
  std::vector<SgRawHost> hr(n);
  for (int k = 0; k < n; ++k) {
    if (!raw[k] || n_raw[k] < 2 || n_raw[k] > 65536) return LINS_E_ARG;
    hr[k] = SgRawHost{(long long)total, n_raw[k], 0};
    total += align4(n_raw[k]);
  }
  int rc = fe_alloc(ctx, n);
  if (rc) return rc;
  auto& f = ctx->fe;
  if (f.sg_cap < n) {
    void* old[] = {f.d_raws, f.d_cellidx, f.d_segrows, f.d_outliers};
    for (void* p : old) (void)hipFree(p);
    f.d_raws = nullptr, f.d_cellidx = nullptr, f.d_segrows = nullptr, f.d_outliers = nullptr, f.sg_cap = 0;
    const size_t c = (size_t)n;
    HIP_TRY(ctx, hipMalloc(&f.d_raws, c * sizeof(SgRawHost)));
    HIP_TRY(ctx, hipMalloc((void**)&f.d_cellidx, c * N * sizeof(unsigned)));
    HIP_TRY(ctx, hipMalloc((void**)&f.d_segrows, c * N * sizeof(int)));
    HIP_TRY(ctx, hipMalloc((void**)&f.d_outliers, c * sizeof(int)));
    f.sg_cap = n;
  }
  if (f.raw_cap < total) {
    (void)hipFree(f.d_raw);
    f.d_raw = nullptr, f.raw_cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&f.d_raw, total * sizeof(float4)));
    f.raw_cap = total;
  }
  if (f.h_raw_cap < total) {
    (void)hipHostFree(f.h_raw);
    f.h_raw = nullptr, f.h_raw_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&f.h_raw, total * sizeof(float4)));
    f.h_raw_cap = total;
  }
  const int rcv = pack_pipelined(
      n, 64,
      [&](int k) -> int {
        const lins_point* p = raw[k];
        for (int i = 0; i < n_raw[k]; ++i)  // (no-return points may be NaN in a real driver's cloud: they never project)
          if (std::isinf(p[i].x) || std::isinf(p[i].y) || std::isinf(p[i].z)) return LINS_E_INPUT;
        std::memcpy(f.h_raw + hr[k].off, p, (size_t)n_raw[k] * sizeof(float4));
        return 0;
      },
      [&](int lo, int hi) -> int {  // a complete chunk of clouds travels while the next ones are packed
        const size_t a = (size_t)hr[lo].off, cnt = (hi < n ? (size_t)hr[hi].off : total) - a;
        HIP_TRY(ctx, hipMemcpyAsync(f.d_raw + a, f.h_raw + a, cnt * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
        return 0;
      });
  if (rcv) {
    (void)hipStreamSynchronize(ctx->stream);
    return rcv;
  }
  std::vector<FeScanHost> hs(n);
  for (int k = 0; k < n; ++k) {
    std::memset(&hs[k], 0, sizeof hs[k]);
    hs[k].off = (long long)((size_t)k * N);
    hs[k].o_sharp = offs[k][0], hs[k].o_less_sharp = offs[k][1], hs[k].o_flat = offs[k][2], hs[k].o_less_flat = offs[k][3];
  }
  HIP_TRY(ctx, hipMemcpyAsync(f.d_raws, hr.data(), (size_t)n * sizeof(SgRawHost), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(f.d_scans, hs.data(), (size_t)n * sizeof(FeScanHost), hipMemcpyHostToDevice, ctx->stream));
  // segmentAlphaX / Y and segmentTheta as the host restatement forms them (parameters.h:88-92)
  const float ax = (float)(0.2f / 180.0 * M_PI), ay = (float)(2.0f / 180.0 * M_PI);
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  launch_segment(ctx->stream, n, f.d_raws, f.d_raw, std::sin(ax), std::cos(ax), std::sin(ay), std::cos(ay), 1.0472f,
                 f.d_cellidx, f.d_segrows, f.d_scans, f.d_cloud, f.d_range, f.d_col, f.d_ground, f.d_outliers);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  return LINS_OK;
}

int lins_segment_batch(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw, lins_segmented_scan* out) {
  if (!ctx || n < 0 || (n && (!raw || !n_raw || !out))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  for (int k = 0; k < n; ++k)
    if (!out[k].cloud || !out[k].range || !out[k].col || !out[k].ground) return LINS_E_ARG;
  std::vector<long long> offs((size_t)n * 4, 0);
  int rc = sg_run(ctx, n, raw, n_raw, reinterpret_cast<const long long(*)[4]>(offs.data()));
  if (rc) return rc;
  auto& f = ctx->fe;
  std::vector<FeScanHost> hs(n);
  std::vector<int> outl(n);
  HIP_TRY(ctx, hipMemcpyAsync(hs.data(), f.d_scans, (size_t)n * sizeof(FeScanHost), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(outl.data(), f.d_outliers, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&f.sg_ms, ctx->ev0, ctx->ev2));
  const size_t N = LINS_CLOUD_MAX;
  for (int k = 0; k < n; ++k) {
    lins_segmented_scan& o = out[k];
    o.n = hs[k].n;
    for (int r = 0; r < LINS_LINE_NUM; ++r) o.start_ring[r] = hs[k].start_ring[r], o.end_ring[r] = hs[k].end_ring[r];
    o.start_ori = hs[k].start_ori, o.end_ori = hs[k].end_ori, o.ori_diff = hs[k].ori_diff;
    o.n_outlier = outl[k];
    const size_t b = (size_t)k * N;
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<lins_point*>(o.cloud), f.d_cloud + b, o.n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<float*>(o.range), f.d_range + b, o.n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint32_t*>(o.col), f.d_col + b, o.n * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(const_cast<uint8_t*>(o.ground), f.d_ground + b, o.n, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

int lins_last_segment_ms(lins_ctx* ctx, float* kernel_ms) {
  if (!ctx || !kernel_ms) return LINS_E_ARG;
  *kernel_ms = ctx->fe.sg_ms;
  return LINS_OK;
}

int lins_extract_features_batch(lins_ctx* ctx, int n, const lins_segmented_scan* in, double scan_period,
                                lins_features* out) {
  if (!ctx || n < 0 || (n && (!in || !out))) return LINS_E_ARG;
  if (n == 0) return LINS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  for (int k = 0; k < n; ++k)
    if (!out[k].corner_sharp || !out[k].corner_less_sharp || !out[k].surf_flat || !out[k].surf_less_flat)
      return LINS_E_ARG;
  const long long per = 192 + 1920 + 384 + LINS_CLOUD_MAX;
  std::vector<long long> offs((size_t)n * 4);
  for (int k = 0; k < n; ++k) {
    long long* o = &offs[(size_t)k * 4];
    o[0] = k * per, o[1] = o[0] + 192, o[2] = o[1] + 1920, o[3] = o[2] + 384;
  }
  std::vector<int> counts;
  int rc = fe_alloc(ctx, n);  // (first, so that the default output buffer exists)
  if (rc) return rc;
  rc = fe_run(ctx, n, in, scan_period, ctx->fe.d_out, reinterpret_cast<const long long(*)[4]>(offs.data()), counts);
  if (rc) return rc;
  auto& f = ctx->fe;
  for (int k = 0; k < n; ++k) {
    const int* c = &counts[(size_t)k * 4];
    const long long* o = &offs[(size_t)k * 4];
    lins_features& ft = out[k];
    ft.n_corner_sharp = c[0], ft.n_corner_less_sharp = c[1], ft.n_surf_flat = c[2], ft.n_surf_less_flat = c[3];
    ft.n_segmented = in[k].n, ft.n_outlier = in[k].n_outlier;
    HIP_TRY(ctx, hipMemcpyAsync(ft.corner_sharp, f.d_out + o[0], c[0] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ft.corner_less_sharp, f.d_out + o[1], c[1] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ft.surf_flat, f.d_out + o[2], c[2] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ft.surf_less_flat, f.d_out + o[3], c[3] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

// ---- device-resident streams: front-end -> IESKF update -> re-projection without the clouds leaving HBM ----
namespace {
// slot layout (points): [flat 512 | sharp 256 | less flat LINS_CLOUD_MAX | less sharp 1920]; the less-sharp cloud
// follows the less-flat one so that the multi-resident kernel's sorted copy (positions 0 .. n_all) stays in the slot
constexpr long long kSlotFlat = 0, kSlotSharp = 512, kSlotLessFlat = 768, kSlotLessSharp = 768 + LINS_CLOUD_MAX;
constexpr long long kSlotSize = kSlotLessSharp + 1920;
inline long long slot_base(int stream, int slot) { return ((long long)stream * 2 + slot) * kSlotSize; }
}  // namespace

int lins_streams_init(lins_ctx* ctx, int n_streams) {
  if (!ctx || n_streams < 1) return LINS_E_ARG;
  if (n_streams > ctx->max_batch) return LINS_E_CAPACITY;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  streams_free(ctx);
  auto& t = ctx->st;
  const size_t pts = (size_t)n_streams * 2 * kSlotSize;
  if (pts >= (1ull << 31)) return LINS_E_CAPACITY;  // ScanDesc offsets are ints
  HIP_TRY(ctx, hipMalloc((void**)&t.d_arena, pts * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_sorted, pts * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_gsorted, pts * sizeof(float4)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_gridtab, (size_t)n_streams * sizeof(GridTables)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_desc, (size_t)n_streams * sizeof(ScanDesc)));
  HIP_TRY(ctx, hipMalloc((void**)&t.d_desc_next, (size_t)n_streams * sizeof(ScanDesc)));
  t.index_ready = false;
  HIP_TRY(ctx, hipMalloc(&t.d_jobs, (size_t)n_streams * 2 * sizeof(StreamCloudHost)));
  t.n = n_streams, t.cur = 0;
  t.last_counts.assign((size_t)n_streams * 2, -1);
  return LINS_OK;
}

static int streams_step_impl(lins_ctx* ctx, const lins_segmented_scan* scans, const lins_point* const* raw,
                             const int32_t* n_raw, const double* prior_state, const double* prior_cov, double scan_period,
                             lins_result* out, int32_t* feature_counts);

int lins_streams_step(lins_ctx* ctx, const lins_segmented_scan* scans, const double* prior_state, const double* prior_cov,
                      double scan_period, lins_result* out, int32_t* feature_counts) {
  if (!scans) return LINS_E_ARG;
  return streams_step_impl(ctx, scans, nullptr, nullptr, prior_state, prior_cov, scan_period, out, feature_counts);
}

int lins_streams_step_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const double* prior_state,
                          const double* prior_cov, double scan_period, lins_result* out, int32_t* feature_counts) {
  if (!raw || !n_raw) return LINS_E_ARG;
  return streams_step_impl(ctx, nullptr, raw, n_raw, prior_state, prior_cov, scan_period, out, feature_counts);
}

static int streams_step_impl(lins_ctx* ctx, const lins_segmented_scan* scans, const lins_point* const* raw,
                             const int32_t* n_raw, const double* prior_state, const double* prior_cov, double scan_period,
                             lins_result* out, int32_t* feature_counts) {
  if (!ctx || !prior_state || !prior_cov || !out) return LINS_E_ARG;
  auto& t = ctx->st;
  if (t.n <= 0 || t.failed) return LINS_E_STATE;  // (after a failed step: lins_streams_init again)
  if (stream_cloud_size() != sizeof(StreamCloudHost)) return LINS_E_STATE;
  // A step either completes for every stream — slots flipped, resident clouds re-projected — or marks the streams
  // context failed: no half-advanced state survives an early return.
  struct Guard {
    bool& failed;
    bool done = false;
    ~Guard() {
      if (!done) failed = true;
    }
  } guard{t.failed};
  const CallTrace trace;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  const int n = t.n, cur = t.cur, last = cur ^ 1;
  ctx->n_uploaded = 0, ctx->ran = false;  // the batch buffers are reused below
  // 1. feature front-end, straight into this scan's slots
  std::vector<long long> offs((size_t)n * 4);
  for (int k = 0; k < n; ++k) {
    long long* o = &offs[(size_t)k * 4];
    const long long b = slot_base(k, cur);
    o[0] = b + kSlotSharp, o[1] = b + kSlotLessSharp, o[2] = b + kSlotFlat, o[3] = b + kSlotLessFlat;
  }
  std::vector<int> counts;
  int rc;
  if (scans) {
    rc = fe_run(ctx, n, scans, scan_period, t.d_arena, reinterpret_cast<const long long(*)[4]>(offs.data()), counts);
  } else {  // raw clouds: the image_projection stage on the device feeds the front-end where its output lies
    rc = sg_run(ctx, n, raw, n_raw, reinterpret_cast<const long long(*)[4]>(offs.data()));
    if (rc) {
      guard.done = rc != LINS_E_HIP;  // (a rejected input has advanced nothing: only this scan's own slots were touched)
      return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipEventElapsedTime(&ctx->fe.sg_ms, ctx->ev0, ctx->ev2));
    rc = fe_launch(ctx, n, scan_period, t.d_arena, counts, 0);
  }
  if (rc) {
    guard.done = rc != LINS_E_HIP;
    return rc;
  }
  t.frontend_ms = ctx->fe.ms;
  trace.mark("front-end done (synced)");
  // 2. IESKF update of every stream against its resident last scan (a stream's first scan: an update
  //    with no rows, which leaves the given state — the bootstrap pose — untouched)
  bool lds_ok = true, mr_ok = true, lds3_ok = true;
  for (int k = 0; k < n; ++k) {
    const int* c = &counts[(size_t)k * 4];  // sharp, less sharp, flat, less flat
    const bool has_last = t.last_counts[(size_t)k * 2] >= 0;
    ScanDesc& d = ctx->h_desc[k];
    const long long bq = slot_base(k, cur), bt = slot_base(k, last);
    d.off_surf_q = (int)(bq + kSlotFlat), d.n_surf_q = has_last ? c[2] : 0;
    d.off_corner_q = (int)(bq + kSlotSharp), d.n_corner_q = has_last ? c[0] : 0;
    d.off_surf_t = (int)(bt + kSlotLessFlat), d.n_surf_t = has_last ? t.last_counts[(size_t)k * 2 + 1] : 0;
    d.off_corner_t = (int)(bt + kSlotLessSharp), d.n_corner_t = has_last ? t.last_counts[(size_t)k * 2] : 0;
    d.surf_sorted = d.corner_sorted = 1;  // the front-end emits ring-major clouds with ring ids < 16
    d.slot_base = k * LINS_MAX_QUERY, d.pad = 0;
    const int n_all = d.n_surf_t + d.n_corner_t;
    if (n_all > lds_np_cap()) lds_ok = false;
    if (n_all > lds_mr_np_cap()) mr_ok = false;
    if (d.n_surf_q + d.n_corner_q > 336) lds3_ok = false;
  }
  ctx->lds_ok = lds_ok, ctx->mr_ok = mr_ok, ctx->lds3_ok = lds3_ok;
  std::memcpy(ctx->h_state, prior_state, (size_t)n * 19 * 8);
  std::memcpy(ctx->h_cov, prior_cov, (size_t)n * 324 * 8);
  HIP_TRY(ctx, hipMemcpyAsync(t.d_desc, ctx->h_desc, (size_t)n * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state_in, ctx->h_state, (size_t)n * 19 * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cov_in, ctx->h_cov, (size_t)n * 324 * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  bool idx_ready = false;
  {
    const int search = effective_search(ctx, n);
    const bool want_lds = search >= SEARCH_LDS, want_mr = search == SEARCH_MR;
    const bool use_mr = want_mr && mr_ok, use_lds = want_lds && !want_mr && lds_ok;
    if (use_mr || use_lds) {
      idx_ready = true;
      // the search index of the last scan's clouds: left by the step before, which re-projected and indexed them in one
      // kernel (step 3 below) — built here only when that step could not (its first scan, another search mode)
      if (!t.index_ready) launch_grid_index(ctx->stream, n, t.d_desc, t.d_arena, t.d_gsorted, t.d_gridtab);
      if (use_mr) {
        // several-part updates as in lins_batch_run (the relay + work queue): more streams than workgroup slots
        RelayArgs ra;
        const bool relay = n > ctx->queue_grid && ctx->prm.icp_freq == 1 && ctx->d_relay_hdr && ctx->relay_at != 0 && relay_max_parts(ctx->prm.num_iter, ctx->relay_at, ctx->relay_cuts) > 1;
        // launch order as in the batch calls: longest-expected-first by the prior's translation (launch_order above;
        // h_state holds this step's priors)
        const bool ordered = ctx->use_order && n > ctx->queue_grid;
        if (ordered) {
          launch_order(ctx, n);
          HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order, ctx->h_order, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        }
        if (relay) {
          const int rcq = relay_prepare(ctx, n, ordered, ra);
          if (rcq) return rcq;
        }
        launch_lds_mr(ctx->stream, n, ctx->dprm, t.d_desc, relay ? ctx->d_order + ctx->max_batch : (ordered ? ctx->d_order : nullptr), t.d_arena, t.d_gsorted, t.d_gridtab, ctx->d_state_in,
                      ctx->d_cov_in, ctx->d_state_out, ctx->d_a6, ctx->d_cov_out, ctx->d_out, ctx->d_idx, nullptr, 0, nullptr, relay ? &ra : nullptr,
                      ctx->d_walk_cache, next_run_gen(ctx), ctx->d_relay_lane);
      } else
        launch_lds(ctx->stream, n, ctx->dprm, search == SEARCH_LDS3 ? 3 : 1, t.d_desc, t.d_arena, t.d_gsorted, t.d_gridtab, ctx->d_state_in,
                   ctx->d_cov_in, ctx->d_state_out, ctx->d_a6, ctx->d_cov_out, ctx->d_out, ctx->d_idx, nullptr, 0, nullptr, ctx->d_relay_lane);
    } else {
      DevParams dp = ctx->dprm;
      dp.search = want_lds ? (int)SEARCH_BINNED : search;
      launch_persistent(ctx->stream, n, dp, t.d_desc, t.d_arena, ctx->d_state_in, ctx->d_cov_in, ctx->d_state_out,
                        ctx->d_cov_out, ctx->d_a6, ctx->d_out, ctx->d_idx, nullptr, 0, t.d_sorted, nullptr);
    }
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state_out, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cov, ctx->d_cov_out, (size_t)n * 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRecHost), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (int rc = relay_check(ctx)) return rc;  // (the guard marks the streams context failed: no stale posterior is re-projected)
  HIP_TRY(ctx, hipEventElapsedTime(&t.update_ms, ctx->ev0, ctx->ev1));
  trace.mark("update done (synced)");
  for (int k = 0; k < n; ++k) {
    lins_result& r = out[k];
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.state, ctx->h_state + (size_t)k * 19, sizeof r.state);
    std::memcpy(r.cov, ctx->h_cov + (size_t)k * 324, sizeof r.cov);
    const OutRecHost& o = ctx->h_out[k];
    const bool has_last = t.last_counts[(size_t)k * 2] >= 0;
    r.residual_norm = o.residual_norm, r.update_norm = o.update_norm;
    r.iters = has_last ? o.iters : 0, r.converged = has_last ? o.converged : 0, r.diverged = has_last ? o.diverged : 0;
    r.m_surf = o.m_surf, r.m_corner = o.m_corner;
    if (!has_last) {  // a stream's first scan: the given state and covariance, bit for bit (also as re-projection pose)
      std::memcpy(r.state, prior_state + (size_t)k * 19, sizeof r.state);
      std::memcpy(r.cov, prior_cov + (size_t)k * 324, sizeof r.cov);
      HIP_TRY(ctx, hipMemcpyAsync(ctx->d_state_out + (size_t)k * 19, ctx->d_state_in + (size_t)k * 19, 19 * 8,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  // 2b. diverged filters: the ICP fallback (SE:585-592) on the same resident clouds, pose into the state row
  for (int k = 0; k < n; ++k) {
    if (!out[k].diverged) continue;
    if (!mr_ok || ctx->prm.icp_freq != 1) {
      // this stream's clouds cannot take the device fallback: it keeps the un-updated filter (what performIESKF
      // holds before SE:585), flagged per stream — the other streams' step is not thrown away
      out[k].reserved[0] = LINS_E_UNSUPPORTED;
      continue;
    }
    if (!idx_ready) {  // (the update ran on the any-size kernel: no index yet)
      launch_grid_index(ctx->stream, n, t.d_desc, t.d_arena, t.d_gsorted, t.d_gridtab);
      idx_ready = true;
    }
    launch_lds_mr_icp(ctx->stream, 1, ctx->dprm, t.d_desc + k, t.d_arena, t.d_gsorted, t.d_gridtab + k, ctx->d_state_in + (size_t)k * 19,
                      ctx->d_state_out + (size_t)k * 19, (char*)ctx->d_out + (size_t)k * sizeof(OutRecHost), ctx->d_idx);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out[k].state, ctx->d_state_out + (size_t)k * 19, 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(out[k].cov, prior_cov + (size_t)k * 324, 324 * 8);  // Pk_ un-updated
  }
  // 3. updatePointCloud: this scan's less-sharp / less-flat clouds to the scan end with the final pose
  //    (device-resident state rows), in place — they are the next step's targets
  std::vector<StreamCloudHost> jobs((size_t)n * 2);
  int max_n = 1;
  for (int k = 0; k < n; ++k) {
    const int* c = &counts[(size_t)k * 4];
    const long long b = slot_base(k, cur);
    jobs[(size_t)k * 2] = StreamCloudHost{b + kSlotLessSharp, c[1], k};
    jobs[(size_t)k * 2 + 1] = StreamCloudHost{b + kSlotLessFlat, c[3], k};
    max_n = std::max(max_n, std::max(c[1], c[3]));
    t.last_counts[(size_t)k * 2] = c[1], t.last_counts[(size_t)k * 2 + 1] = c[3];
    if (feature_counts) std::memcpy(feature_counts + (size_t)k * 4, c, 4 * sizeof(int));
  }
  // ... and, when the next step's update will search through the LDS grid, their search index in the same pass
  // (grid_index_kernel<true>: one read of the new clouds for the re-projected arena copy, the grid-sorted copy and the
  // tables; SURVEY f-2 "re-projection + target binning build")
  bool fuse = ctx->streams_fuse && effective_search(ctx, n) >= SEARCH_LDS;
  for (int k = 0; k < n && fuse; ++k) {
    const int* c = &counts[(size_t)k * 4];
    if (c[1] + c[3] > kGridNpMax || c[1] + c[3] > (effective_search(ctx, n) == SEARCH_MR ? lds_mr_np_cap() : lds_np_cap())) fuse = false;
  }
  if (fuse) {
    for (int k = 0; k < n; ++k) {
      const int* c = &counts[(size_t)k * 4];
      ScanDesc& d = ctx->h_desc[k];  // (the update's descriptors have been consumed: its kernel has finished)
      const long long b = slot_base(k, cur);
      d.off_surf_t = (int)(b + kSlotLessFlat), d.n_surf_t = c[3];
      d.off_corner_t = (int)(b + kSlotLessSharp), d.n_corner_t = c[1];
    }
    HIP_TRY(ctx, hipMemcpyAsync(t.d_desc_next, ctx->h_desc, (size_t)n * sizeof(ScanDesc), hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(t.d_jobs, jobs.data(), jobs.size() * sizeof(StreamCloudHost), hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  if (fuse)
    launch_reproject_and_index(ctx->stream, n, t.d_desc_next, t.d_arena, t.d_gsorted, t.d_gridtab, ctx->d_state_out, (double)(1.f / (float)scan_period));
  else
    launch_reproject_in_place(ctx->stream, 2 * n, max_n, t.d_jobs, ctx->d_state_out, t.d_arena, (double)(1.f / (float)scan_period));
  t.index_ready = fuse;
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipEventElapsedTime(&t.reproject_ms, ctx->ev0, ctx->ev2));
  trace.mark("re-projection done (synced)");
  t.cur = last;
  guard.done = true;
  return LINS_OK;
}

int lins_streams_stats(lins_ctx* ctx, float* frontend_ms, float* update_ms, float* reproject_ms) {
  if (!ctx) return LINS_E_ARG;
  if (frontend_ms) *frontend_ms = ctx->st.frontend_ms;
  if (update_ms) *update_ms = ctx->st.update_ms;
  if (reproject_ms) *reproject_ms = ctx->st.reproject_ms;
  return LINS_OK;
}

/* test aid: one resident cloud of a stream back to the host (which: 0 less sharp, 1 less flat of the LAST scan) */
int lins_streams_peek(lins_ctx* ctx, int stream, int which, lins_point* out, int cap) {
  if (!ctx || !out || stream < 0 || stream >= ctx->st.n || which < 0 || which > 1) return LINS_E_ARG;
  auto& t = ctx->st;
  const int cnt = t.last_counts[(size_t)stream * 2 + which];
  if (cnt < 0) return LINS_E_STATE;
  if (cnt > cap) return LINS_E_CAPACITY;
  const long long b = slot_base(stream, t.cur ^ 1) + (which ? kSlotLessFlat : kSlotLessSharp);
  HIP_TRY(ctx, hipMemcpy(out, t.d_arena + b, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost));
  return cnt;
}

int lins_last_frontend_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* bytes) {
  if (!ctx) return LINS_E_ARG;
  if (kernel_ms) *kernel_ms = ctx->fe.ms;
  if (bytes) *bytes = ctx->fe.bytes;
  return LINS_OK;
}

int lins_transform_to_end_batch(lins_ctx* ctx, int n_jobs, const lins_reproject_job* jobs) {
  if (!ctx || n_jobs < 0 || (n_jobs && !jobs)) return LINS_E_ARG;
  if (n_jobs == 0) return LINS_OK;
  static_assert(sizeof(ReprojectJobHost) == 80, "ReprojectJob layout");
  if (reproject_job_size() != sizeof(ReprojectJobHost)) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;
  std::vector<ReprojectJobHost> hj(n_jobs);
  size_t off = 0;
  int max_n = 0;
  bool any_yzx = false;
  for (int k = 0; k < n_jobs; ++k) {
    const lins_reproject_job& j = jobs[k];
    if (j.n < 0 || (j.n && (!j.in || !j.out_xyz))) return LINS_E_ARG;
    if (off + align4(j.n) > ctx->arena_cap) return LINS_E_CAPACITY;
    for (int i = 0; i < j.n; ++i)
      if (!std::isfinite(j.in[i].x) || !std::isfinite(j.in[i].y) || !std::isfinite(j.in[i].z) ||
          !std::isfinite(j.in[i].intensity))
        return LINS_E_INPUT;
    if (j.n) std::memcpy(ctx->h_arena + off, j.in, sizeof(lins_point) * j.n);
    hj[k].off = (long long)off, hj[k].n = j.n, hj[k].has_yzx = j.out_yzx != nullptr;
    std::memcpy(hj[k].t, j.t, sizeof j.t);
    std::memcpy(hj[k].q, j.q, sizeof j.q);
    hj[k].inv_period = (double)(1.f / ctx->prm.scan_period);
    any_yzx = any_yzx || j.out_yzx;
    max_n = j.n > max_n ? j.n : max_n;
    off += align4(j.n);
  }
  if (any_yzx && !ctx->d_aux) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_aux, ctx->arena_cap * sizeof(float4)));
  (void)hipFree(ctx->d_jobs);
  ctx->d_jobs = nullptr;
  HIP_TRY(ctx, hipMalloc(&ctx->d_jobs, (size_t)n_jobs * sizeof(ReprojectJobHost)));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_jobs, hj.data(), (size_t)n_jobs * sizeof(ReprojectJobHost), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_arena, ctx->h_arena, off * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  launch_transform_to_end(ctx->stream, n_jobs, max_n, ctx->d_jobs, ctx->d_arena, ctx->d_binned, ctx->d_aux);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  ctx->n_uploaded = 0;  // the arenas no longer hold an IESKF batch
  ctx->ran = false;
  uint64_t bytes = 0;
  for (int k = 0; k < n_jobs; ++k) bytes += (uint64_t)jobs[k].n * (jobs[k].out_yzx ? 48 : 32);
  for (int pass = 0; pass < (any_yzx ? 2 : 1); ++pass) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_arena, pass == 0 ? ctx->d_binned : ctx->d_aux, off * sizeof(float4),
                                hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n_jobs; ++k) {
      lins_point* dst = pass == 0 ? jobs[k].out_xyz : jobs[k].out_yzx;
      if (dst && jobs[k].n) std::memcpy(dst, ctx->h_arena + hj[k].off, sizeof(lins_point) * jobs[k].n);
    }
  }
  HIP_TRY(ctx, hipEventElapsedTime(&ctx->reproject_ms, ctx->ev0, ctx->ev2));
  ctx->reproject_bytes = bytes;
  return LINS_OK;
}

int lins_last_reproject_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* bytes) {
  if (!ctx) return LINS_E_ARG;
  if (kernel_ms) *kernel_ms = ctx->reproject_ms;
  if (bytes) *bytes = ctx->reproject_bytes;
  return LINS_OK;
}

int lins_sync(lins_ctx* ctx) {
  if (!ctx) return LINS_E_ARG;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = pipe_join(ctx);  // (side streams of the pipelined mode: ordered before the wait below)
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return relay_check(ctx);
}

int lins_batch_download(lins_ctx* ctx, int n, lins_result* out) {
  if (!ctx || !out || n < 0) return LINS_E_ARG;
  if (!ctx->ran || n > ctx->n_uploaded) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  {
    int rc = pipe_join(ctx);
    if (rc) return rc;
  }
  if (n == ctx->max_batch) {  // the whole context: posteriors and out records are one block (lins_ctx::h_meta)
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_meta, ctx->d_meta_out, ctx->meta_out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state_out, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_cov, ctx->d_cov_out, (size_t)n * 324 * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRecHost), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (int rc = relay_check(ctx)) return rc;  // (a scan whose hand-over never arrived holds an earlier launch's values)
  uint64_t tot = 0;
  for (int s = 0; s < n; ++s) {
    lins_result& r = out[s];
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.state, ctx->h_state + (size_t)s * 19, sizeof r.state);
    std::memcpy(r.cov, ctx->h_cov + (size_t)s * 324, sizeof r.cov);
    const OutRecHost& o = ctx->h_out[s];
    r.residual_norm = o.residual_norm, r.update_norm = o.update_norm;
    r.iters = o.iters, r.converged = o.converged, r.diverged = o.diverged;
    r.m_surf = o.m_surf, r.m_corner = o.m_corner;
    r.reserved[0] = o.pad[0], r.reserved[1] = o.pad[1], r.reserved[2] = o.pad[2];
    tot += (uint64_t)o.iters;
  }
  if (n == ctx->n_uploaded) ctx->total_iters = tot;
  return LINS_OK;
}

int lins_last_kernel_ms(lins_ctx* ctx, float* ms) {
  if (!ctx || !ms) return LINS_E_ARG;
  if (!ctx->ran || ctx->hist_n == 0) return LINS_E_STATE;
  return lins_kernel_ms_history(ctx, 1, ms);
}

int lins_batch_bytes_per_iter(lins_ctx* ctx, uint64_t* bytes) {
  if (!ctx || !bytes) return LINS_E_ARG;
  *bytes = ctx->bytes_per_iter;
  return LINS_OK;
}

int lins_batch_total_iters(lins_ctx* ctx, uint64_t* iters) {
  if (!ctx || !iters) return LINS_E_ARG;
  if (!ctx->ran) return LINS_E_STATE;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (int rcs = split_join(ctx)) return rcs;  // (results of the second launch queue: ordered before what follows)
  int n = ctx->n_uploaded;
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRecHost), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t tot = 0;
  for (int s = 0; s < n; ++s) tot += (uint64_t)ctx->h_out[s].iters;
  *iters = ctx->total_iters = tot;
  return LINS_OK;
}

int lins_ieskf_update_batch(lins_ctx* ctx, int n, const lins_scan_pair* in, lins_result* out) {
  if (!ctx || n < 0 || (n && (!in || !out))) return LINS_E_ARG;
  // Host buffers in and out: the whole call is bounded by validation + packing and PCIe, not by the kernels.  Large
  // batches are therefore PIPELINED: a pool of host threads validates and packs scan after scan into the pinned
  // staging arena; as soon as a chunk of scans is complete, the calling thread sends it (copy stream) and queues its
  // kernels behind the copy (compute stream) while the pool is already packing the next chunks.  (The
  // the phase profile stay on the staged API: lins_batch_upload / _run.)
  int kChunk = 256;  // (measured: 4.6 / 4.2 / 4.1 / 5.7 ms per 1024 scans with chunks of 512 / 256 / 128 / 64)
  bool trace = false;
  if (const char* g = std::getenv("LINS_ENABLE_DEBUG_KNOBS"))
    if (g[0] == '1') {
      if (const char* e = std::getenv("LINS_BATCH_CHUNK")) kChunk = std::max(64, std::atoi(e));
      trace = std::getenv("LINS_BATCH_TRACE") != nullptr;  // stage times on stderr (and two extra syncs)
    }
  const auto t_begin = std::chrono::steady_clock::now();
  auto now_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
  if (n < 2 * kChunk || ctx->d_prof) {
    const CallTrace tr;
    int rc = upload(ctx, n, in, /*wait*/ false);  // (lins_batch_download below waits for the whole chain)
    if (rc) return rc;
    if (n == 0) return LINS_OK;
    tr.mark("update: uploaded");
    if ((rc = lins_batch_run(ctx, nullptr, 0))) return rc;
    tr.mark("update: run queued");
    rc = lins_batch_download(ctx, n, out);
    tr.mark("update: downloaded");
    return rc;
  }
  size_t arena_used = 0, slots = 0;
  uint64_t bytes = 0;
  int rc = layout_batch(ctx, n, in, &arena_used, &slots, &bytes);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->copy_stream) {
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_copy, hipEventDisableTiming));
  }
  ctx->n_uploaded = 0, ctx->ran = false;
  // the uploads below overwrite the inputs of whatever is still queued on the compute stream (an earlier asynchronous
  // lins_batch_run, the side streams of the pipelined mode): order the copy stream behind it
  if ((rc = pipe_join(ctx))) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev_copy, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_copy, 0));

  // (kernel family per CHUNK: a scan that cannot take the grid kernels sends its own chunk of 256, not the whole batch,
  // to the any-size kernel — every family returns the same results, so a scan's bits do not depend on the cut)
  RangeFlags all;
  rc = pack_pipelined(
      n, kChunk, [&](int s) { return pack_one(ctx, in, s); },
      [&](int lo, int hi) -> int {
        if (trace) std::fprintf(stderr, "scans %d..%d packed at %.3f ms\n", lo, hi, now_ms());
        const RangeFlags fl = range_flags(ctx, lo, hi);
        const size_t arena_end = hi < n ? (size_t)ctx->h_desc[hi].off_surf_q : arena_used;
        int r = h2d_range(ctx, lo, hi, arena_end, ctx->copy_stream);
        if (r) return r;
        hipError_t e = hipEventRecord(ctx->ev_copy, ctx->copy_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_copy, 0);
        if (e == hipSuccess && lo == 0) e = hipEventRecord(ctx->hist0[ctx->hist_n % lins_ctx::kHist], ctx->stream);
        if (e != hipSuccess) return fail_hip(ctx, e, "chunk hand-over (event record / stream wait)");
        if ((r = build_index_range(ctx, lo, hi - lo, fl))) return r;
        if ((r = run_range(ctx, lo, hi - lo, n, fl, nullptr, 0))) return r;
        all.lds_ok = all.lds_ok && fl.lds_ok, all.mr_ok = all.mr_ok && fl.mr_ok, all.lds3_ok = all.lds3_ok && fl.lds3_ok;
        return 0;
      });
  if (rc) {
    (void)hipStreamSynchronize(ctx->copy_stream), (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  if (trace) {
    std::fprintf(stderr, "all issued at %.3f ms (arena %.1f MB)\n", now_ms(), arena_used * 16e-6);
    (void)hipStreamSynchronize(ctx->copy_stream);
    std::fprintf(stderr, "copies done at %.3f ms\n", now_ms());
    (void)hipStreamSynchronize(ctx->stream);
    std::fprintf(stderr, "kernels done at %.3f ms\n", now_ms());
  }
  // (the history entry of this call spans the whole pipelined region: the kernels of all chunks AND the copy waits
  // between them — lins_last_kernel_ms() after lins_ieskf_update_batch() is an upper bound of the kernel time)
  HIP_TRY(ctx, hipEventRecord(ctx->hist1[ctx->hist_n % lins_ctx::kHist], ctx->stream));
  ctx->hist_split[ctx->hist_n % lins_ctx::kHist] = false;  // (one queue: the slot's second-queue events are another run's)
  ctx->hist_n++;
  // the batch stays resident (inputs, search index): a later lins_batch_run finds its launch order too
  launch_order(ctx, n);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order, ctx->h_order, (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  ctx->idx_timed = false;  // (the index was built chunk by chunk between the copies: no single time to report)
  set_batch_state(ctx, n, all, slots, bytes);
  ctx->ran = true;
  return lins_batch_download(ctx, n, out);
}

/* The ICP / Gauss-Newton fallback of SE:585-592 (estimateTransform, SE:1163-1320) on the device:
 * n scans from the poses in in[].state, out[].state = that state with position and attitude
 * replaced, out[].cov = in[].cov (un-updated), out[].iters / converged = rounds run / stop rule hit.
 * LINS_E_UNSUPPORTED (nothing run) when a scan cannot take the grid kernels (unsorted rings, ring
 * ids >= 16, > 12288 target points): lins_host_perform_ieskf() then falls back to the host
 * Gauss-Newton step over lins_correspondences().                                                */
int lins_icp_update_batch(lins_ctx* ctx, int n, const lins_scan_pair* in, lins_result* out) {
  if (!ctx || n < 0 || (n && (!in || !out))) return LINS_E_ARG;
  int rc = upload(ctx, n, in);
  if (rc) return rc;
  ctx->n_uploaded = 0;  // not an IESKF batch
  if (n == 0) return LINS_OK;
  if (!ctx->mr_ok) return LINS_E_UNSUPPORTED;
  if (ctx->prm.icp_freq != 1) {
    // stored triplets are reused between searches: a scan starts with empty ones, as the oracle does (the
    // reference's arrays keep whatever the previous scan left, SE:206-211), and the deferred corner commit
    // needs every query of a scan in one round of the 512-lane kernel
    for (int s = 0; s < n; ++s)
      if (in[s].n_surf_flat + in[s].n_corner_sharp > 512) return LINS_E_UNSUPPORTED;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_idx, 0xFF, ctx->slot_cap * sizeof(int4), ctx->stream));
  }
  launch_lds_mr_icp(ctx->stream, n, ctx->dprm, ctx->d_desc, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab, ctx->d_state_in,
                    ctx->d_state_out, ctx->d_out, ctx->d_idx);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state_out, (size_t)n * 19 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_out, (size_t)n * sizeof(OutRecHost), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < n; ++s) {
    lins_result& r = out[s];
    std::memset(&r, 0, sizeof r);
    std::memcpy(r.state, ctx->h_state + (size_t)s * 19, sizeof r.state);
    std::memcpy(r.cov, in[s].cov, sizeof r.cov);
    const OutRecHost& o = ctx->h_out[s];
    r.iters = o.iters, r.converged = o.converged, r.m_surf = o.m_surf, r.m_corner = o.m_corner;
  }
  return LINS_OK;
}

int lins_ieskf_update(lins_ctx* ctx, const lins_scan_pair* in, lins_result* out) {
  return lins_ieskf_update_batch(ctx, 1, in, out);
}

static int run_pass(lins_ctx* ctx, const lins_scan_pair* in, const double* lin_state, int iter, bool dump,
                    bool sums) {
  int rc = upload(ctx, 1, in);
  if (rc) return rc;
  ctx->n_uploaded = 0;  // the single-pass calls do not leave a runnable batch behind
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_lin, lin_state, 19 * 8, hipMemcpyHostToDevice, ctx->stream));
  const int search = effective_search(ctx, 1);
  const bool want_lds = search >= SEARCH_LDS, want_mr = search == SEARCH_MR;
  if (want_mr && ctx->mr_ok) {
    launch_lds_mr_pass(ctx->stream, 1, ctx->dprm, ctx->d_desc, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab, ctx->d_lin,
                       ctx->d_state_in, iter, ctx->d_idx, dump ? ctx->d_dump : nullptr, sums ? ctx->d_sums : nullptr,
                       sums ? ctx->d_counts : nullptr);
  } else if (want_lds && !want_mr && ctx->lds_ok) {
    launch_lds_pass(ctx->stream, 1, ctx->dprm, search == SEARCH_LDS3 ? 3 : 1, ctx->d_desc, ctx->d_arena, ctx->d_gsorted, ctx->d_gridtab, ctx->d_lin, ctx->d_state_in, iter,
                    ctx->d_idx, dump ? ctx->d_dump : nullptr, sums ? ctx->d_sums : nullptr,
                    sums ? ctx->d_counts : nullptr);
  } else {
    DevParams dp = ctx->dprm;
    dp.search = want_lds ? (int)SEARCH_BINNED : search;
    launch_pass(ctx->stream, 1, dp, ctx->d_desc, ctx->d_arena, ctx->d_lin, ctx->d_state_in, iter, ctx->d_idx,
                dump ? ctx->d_dump : nullptr, sums ? ctx->d_sums : nullptr, sums ? ctx->d_counts : nullptr,
                ctx->d_binned);
  }
  HIP_TRY(ctx, hipGetLastError());
  return LINS_OK;
}

int lins_correspondences(lins_ctx* ctx, const lins_scan_pair* in, const double* lin_state, int iter,
                         lins_corr* surf, lins_corr* corner) {
  if (!ctx || !in || !lin_state) return LINS_E_ARG;
  int rc = run_pass(ctx, in, lin_state, iter, true, false);
  if (rc) return rc;
  if (surf && in->n_surf_flat)
    HIP_TRY(ctx, hipMemcpyAsync(surf, ctx->d_dump, sizeof(lins_corr) * in->n_surf_flat, hipMemcpyDeviceToHost, ctx->stream));
  if (corner && in->n_corner_sharp)
    HIP_TRY(ctx, hipMemcpyAsync(corner, ctx->d_dump + in->n_surf_flat, sizeof(lins_corr) * in->n_corner_sharp,
                                hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return LINS_OK;
}

int lins_reduce_pass(lins_ctx* ctx, const lins_scan_pair* in, const double* lin_state, int iter, double* sums28,
                     int32_t* m_surf, int32_t* m_corner) {
  if (!ctx || !in || !lin_state || !sums28) return LINS_E_ARG;
  int rc = run_pass(ctx, in, lin_state, iter, false, true);
  if (rc) return rc;
  int counts[2];
  HIP_TRY(ctx, hipMemcpyAsync(sums28, ctx->d_sums, 28 * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->d_counts, sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (m_surf) *m_surf = counts[0];
  if (m_corner) *m_corner = counts[1];
  return LINS_OK;
}

}  // extern "C"
