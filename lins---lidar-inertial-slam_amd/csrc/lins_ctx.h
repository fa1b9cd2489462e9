// lins_ctx.h — the context of the C ABI (include/lins_ieskf.h) and what the C API files share: the struct itself, the
// error macro, and the helpers more than one of lins_capi.hip / lins_capi_dist.hip / lins_capi_frontend.hip /
// lins_capi_streams.hip / lins_capi_debug.hip needs.  (The scan-to-map files see a context through lins_ctx_priv.h only;
// lins_streams_slam_capi.hip, which joins the streams' filter to their mapping step, includes this header.)
#pragma once

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
#include "../../include/lins_streams_filter.h"
#include "../../include/lins_streams_map.h"
#include "../../include/lins_streams_slam.h"
#include "ieskf_device.h"
#include "ieskf_grid.h"
#include "lins_ctx_priv.h"
#include "lins_launch.h"
#include "lins_records.h"

using namespace lins;  // (a header of the C API files only)

namespace lins {
struct RangeFlags {  // which kernel families the scans of a range can take
  bool lds_ok = false;   // every scan fits the LDS-resident kernel
  bool mr_ok = false;    // ... the multi-resident (hybrid LDS / global) kernel
  bool lds3_ok = false;  // ... has at most kLds3QueryMax queries (one round of the 3-lane shape)
};
}  // namespace lins

struct lins_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;  // IESKF kernel start / end, Joseph kernel end
  hipStream_t copy_stream = nullptr;  // lins_ieskf_update_batch: uploads of the next chunk beside the running one
  Event ev_copy;  // (created with copy_stream)
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
  OutRec* h_out = nullptr;
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
  DevBuf<float4> d_aux;     // third point arena (YZX copies of the re-projection), lazily allocated
  DevBuf<ReprojectJob> d_jobs;  // the jobs of the last lins_transform_to_end_batch
  float reproject_ms = 0.f;
  uint64_t reproject_bytes = 0;
  // feature front-end (lins_extract_features_batch): device buffers, allocated on first use, for the largest batch so far
  struct Frontend {
    DevBuf<FeScan> d_scans;  // (its capacity: the scans the group below is allocated for)
    DevBuf<float4> d_cloud, d_out;  // d_out: kFeStride points per scan
    DevBuf<float> d_range;
    DevBuf<unsigned> d_col;
    DevBuf<unsigned char> d_ground;
    DevBuf<int> d_picks, d_counts;
    // pinned host staging of the packed inputs (one group, grow-only; h_cloud answers, in points)
    PinBuf<float4> h_cloud;
    PinBuf<float> h_range;
    PinBuf<unsigned> h_col;
    PinBuf<unsigned char> h_ground;
    float ms = 0.f;
    uint64_t bytes = 0;
    // image_projection stage (lins_segment_batch / the raw-cloud streams path): raw points + per-cell scratch
    DevBuf<float4> d_raw;
    PinBuf<float4> h_raw;
    DevBuf<SgRaw> d_raws;  // (d_raws, d_cellidx, d_segrows, d_outliers: one group, d_raws answers, in scans)
    DevBuf<unsigned> d_cellidx;
    DevBuf<int> d_segrows, d_outliers;
    DevBuf<float4> d_outl;  // lins_segment_batch_outliers: the outlier clouds, LINS_OUTLIER_MAX points per scan
    float sg_ms = 0.f;
  } fe;
  // device-resident streams (lins_streams_step): per stream two feature slots (this scan's / the last
  // scan's clouds) inside one arena, so that ScanDesc offsets address both
  struct Streams {
    int n = 0;
    std::vector<int> cur;         // per stream: slot the NEXT scan's features go to (a gated scan does not flip its stream's)
    DevBuf<float4> d_arena, d_sorted, d_gsorted;
    DevBuf<GridTables> d_gridtab;
    DevBuf<ScanDesc> d_desc;
    DevBuf<ScanDesc> d_desc_next;  // the clouds of the scan just taken in as the NEXT step's targets (fused re-projection + index)
    bool index_ready = false;         // d_gsorted / d_gridtab hold the index of the resident last scans (built by the step before)
    DevBuf<StreamCloud> d_jobs;
    std::vector<int> last_counts;  // per stream: less sharp, less flat of the resident last scan (-1: none yet)
    // the outlier clouds (lins_streams_map_cloud, lins_local_map_build_streams): two slots of LINS_OUTLIER_MAX points per
    // stream, flipped with the feature slots — a raw step's segmentation writes slot cur, lins_streams_put_outliers too
    DevBuf<float4> d_outl;
    std::vector<int> outl_counts;  // [stream][slot]
    std::vector<int> outl_put;     // per stream: the count lins_streams_put_outliers left for the next segmented step
    bool outl_pending = false;
    bool failed = false;           // a step stopped half way (HIP error): the resident clouds are not trustworthy any more
    float update_ms = 0.f, frontend_ms = 0.f, reproject_ms = 0.f;
    // the streams' filter (lins_streams_filter_*, lins_streams_step_imu*; lins_capi_filter.hip): what lins_filter holds
    // and globalState_, one row per stream in the layout of d_state_in / d_cov_in — the update kernels read the predicted
    // prior where it lies.  Allocated by the first lins_streams_filter_set.
    struct Filter {
      DevBuf<double> d_state, d_cov, d_noise, d_aux, d_gstate;  // n x 19 / 324 / 144 / kAux / 19
      DevBuf<double> d_imu;  // this call's IMU rows, packed (n x LINS_STREAMS_IMU_MAX x 7 at most; h_: pinned)
      PinBuf<double> h_imu;
      DevBuf<int> d_ints;    // [n_imu | row offset | finish mode] x n (h_: pinned)
      PinBuf<int> h_ints;
      std::vector<char> set;                      // per stream: a filter has been loaded
      std::vector<lins_filter_params> prm;        // ... and its parameters (lins_streams_filter_get returns them)
      Event ev[4];                                // predict start / end, finish start / end
      bool predict_timed = false, finish_timed = false;
      float predict_ms = 0.f, finish_ms = 0.f;
    } f;
    // the streams' state machine (lins_streams_machine_init, lins_streams_process*; lins_capi_boot.hip): the reference's
    // status_ per stream and what the two-scan bootstrap keeps on the device
    struct Boot {
      bool on = false;
      lins_boot_params prm{};
      std::vector<int> status;       // LINS_STREAM_INIT / _FIRST_SCAN / _RUNNING
      std::vector<char> imu_seen;    // the stream has been given an IMU row (or a scan_imu)
      std::vector<double> imu_last;  // ... the newest one: n x 6 (acc, gyr)
      std::vector<double> h_tmpl;    // host copy of the template (lins_boot::kTmpl doubles)
      DevBuf<double> d_tmpl, d_pre;  // the template; n x lins_boot::kPre pre-integration records
      DevBuf<double> d_rows;         // this call's rows of the FIRST_SCAN streams, component-major (h_: pinned)
      PinBuf<double> h_rows;
      DevBuf<double> d_scan;         // n x 8: imu_last_ and time of this call's scans
      PinBuf<double> h_scan;
      DevBuf<int> d_ints;            // [rows per stream | finish mode | ICP slot | ICP list] x n
      PinBuf<int> h_ints;
      // the batched ICP of the second scans: compact descriptors, index tables, start / result rows, out records
      DevBuf<ScanDesc> d_desc;
      DevBuf<GridTables> d_tab;
      DevBuf<double> d_icp_in, d_icp_out;
      DevBuf<OutRec> d_out;
      PinBuf<OutRec> h_out;
      Event ev[6];  // pre-integration, ICP, finish: start / end
      bool pre_timed = false, icp_timed = false, finish_timed = false;
      float pre_ms = 0.f, icp_ms = 0.f, finish_ms = 0.f;
    } b;
    // streams end to end (lins_streams_slam.h; lins_streams_slam_capi.hip): the odometry records derived from d_gstate and
    // the staging of the fusion.  Allocated by the first call that derives the records.
    struct Slam {
      DevBuf<lins_stream_odom> d_odom;  // n records (h_: pinned)
      PinBuf<lins_stream_odom> h_odom;
      DevBuf<int> d_ints;               // [stream has a globalState_ | fusion list] x n (h_: pinned)
      PinBuf<int> h_ints;
      DevBuf<lins_fused_pose> d_fused;  // n fused poses (h_: pinned)
      PinBuf<lins_fused_pose> h_fused;
      bool have = false;                                      // the records have been derived at least once
    } s;
  } st;
  // stream snapshots (include/lins_snapshot.h; lins_snapshot_capi.hip): the staging buffer of a pack / unpack — the
  // device part of the call's blobs — with its pinned mirror, the table (bases | segments | tiles), the last call's figures
  struct Snap {
    DevBuf<char> d_stage, d_tab;  // (bytes)
    PinBuf<char> h_stage, h_tab;
    float pack_ms = 0.f, unpack_ms = 0.f;
    uint64_t bytes = 0;
    int segments = 0;
  } snap;
  void* map_state = nullptr;  // scan-to-map row (lins_map_capi.hip), freed through map_state_free
  void (*map_state_free)(void*) = nullptr;
  DevBuf<long long> d_prof;  // optional per-workgroup phase profile (lins_debug_phase_profile)
  double* d_a6 = nullptr;  // upper triangle of the last iteration's H^T H, per scan
  OutRec* d_out = nullptr;
  int4* d_idx = nullptr;
  lins_corr* d_dump = nullptr;
  double* d_sums = nullptr;
  int* d_counts = nullptr;
  int n_uploaded = 0;
  RangeFlags fl;        // what the uploaded scans can take
  int n_cu = 256;       // compute units of the device ("auto": batches beyond this take the mr kernel)
  int last_search = -1; // kernel family the last batch actually ran
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

inline size_t align4(size_t n) { return (n + 3) & ~size_t(3); }

// the front-end's default output buffer (lins_ctx::Frontend::d_out), points per scan: [sharp | less sharp | flat | less flat]
constexpr long long kFeSharp = 192, kFeLessSharp = 1920, kFeFlat = 384, kFeLessFlat = LINS_CLOUD_MAX;
constexpr long long kFeStride = kFeSharp + kFeLessSharp + kFeFlat + kFeLessFlat;
// queries of a scan the 3-lane shape of the full-residency kernel takes: one round, 16 waves x 21 query slots = the
// VLP-16 caps (144 flat + 192 sharp)
constexpr int kLds3QueryMax = 336;

// ---- lins_capi.hip
int split_join(lins_ctx* ctx);  // the context's stream behind the second launch queue
int pipe_join(lins_ctx* ctx);   // ... and behind the gather stream of the pipelined mode
struct Family {
  int search;            // the requested mode after "auto" and the 3-lane fall-back
  bool use_mr, use_lds;  // the batch kernel / the full-residency kernel; neither: the any-size kernel
  int ran;               // what lins_last_search reports (a scan that does not fit LDS: global-memory grid)
};
RangeFlags range_flags(const ScanDesc* desc, int n);
Family pick_family(const lins_ctx* ctx, int n_total, const RangeFlags& fl);
// where an update launch reads and writes: the uploaded batch's buffers (lins_capi.hip batch_io) or the streams' (lins_capi_streams.hip)
struct UpdateIo {
  const ScanDesc* desc;
  const float4 *arena, *gsorted;  // the clouds and their grid-sorted copy (tables: gridtab)
  const GridTables* gridtab;
  float4* binned;  // the any-size kernel's (ring x column)-sorted scratch
  const double *state_in, *cov_in;
  double *state_out, *cov_out, *a6;
  OutRec* out;
  int* relay_lane;
  lins_pose_record* poses;  // null, or the pose record of the first scan launched (its scan id: scan_id_base)
  int32_t scan_id_base;
  long long* prof;
};
void run_family(lins_ctx* ctx, const Family& fam, hipStream_t st, const UpdateIo& io, int cnt, const int* order, const RelayArgs* relay);
void launch_order(lins_ctx* ctx, int n);
int next_run_gen(lins_ctx* ctx);
int relay_prepare(lins_ctx* ctx, int n, bool ordered, RelayArgs& ra);
int relay_check(lins_ctx* ctx);
// ---- lins_capi_dist.hip / lins_capi_frontend.hip / lins_capi_streams.hip: what lins_destroy frees
void rccl_free(lins_ctx* ctx);
void fe_free(lins_ctx* ctx);
void streams_free(lins_ctx* ctx);
// ---- lins_capi_frontend.hip: the stages in front of the update, as the streams step calls them (described there)
int fe_run(lins_ctx* ctx, int n, const lins_segmented_scan* in, double scan_period, float4* out_base, const long long (*offs)[4], std::vector<int>& counts);
int fe_launch(lins_ctx* ctx, int n, double scan_period, float4* out_base, std::vector<int>& counts, uint64_t bytes);
int sg_run(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw, const long long (*offs)[4], float4* outl = nullptr, const int* o_slots = nullptr);
// ---- lins_capi_filter.hip
void streams_filter_free(lins_ctx* ctx);
int streams_filter_alloc(lins_ctx* ctx);
// queue the predict kernel over this call's IMU rows on the context's stream (arguments checked by the caller:
// streams_filter_check); no synchronisation
int streams_filter_check(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu);
int streams_filter_predict_queue(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu);
// queue the finish kernel (mode per stream as launch_filter_finish) behind the update
int streams_filter_finish_queue(lins_ctx* ctx, const int* mode);

// ---- lins_capi_streams.hip: the step every lins_streams_step* / lins_streams_process* call ends in
// what lins_streams_process* adds to a step: imu_last_ (n x 6, resolved by the caller) and time of each scan
struct StepMachine {
  const double* scan_imu;
  const double* scan_time;
  const char* imu_seen;  // per stream: scan_imu[k] is valid (a RUNNING stream needs none)
  int32_t* status_out;
};
struct StepImu {  // the prior comes from the streams' device filter (lins_streams_step_imu*)
  const int32_t* n_imu;
  const double* const* rows;
  double* global_state_out;
};
struct StepScans {  // this call's scans: segmented by the caller, or (segmented == null) raw clouds
  const lins_segmented_scan* segmented;
  const lins_point* const* raw;
  const int32_t* n_raw;
  double scan_period;
};
struct StepPrior {  // the caller's priors (n x 19, n x 324), or (imu != null) the device filter's; mach (with imu): the state machine's step
  const double *state, *cov;
  const StepImu* imu;
  const StepMachine* mach;
};
int streams_step_impl(lins_ctx* ctx, const StepScans& scans, const StepPrior& prior, lins_result* out, int32_t* feature_counts);
// ---- lins_capi_boot.hip: the streams' state machine around that step
void streams_boot_free(lins_ctx* ctx);
void streams_slam_free(lins_ctx* ctx);  // lins_streams_slam_capi.hip
// argument check of a machine-mode call's IMU rows (as streams_filter_check, without the need of a loaded filter)
int streams_boot_check(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu);
// queue the pre-integration kernel over the rows of the streams in FIRST_SCAN
int streams_boot_preintegrate_queue(lins_ctx* ctx, const int32_t* n_imu, const double* const* imu);
// queue start rows, index, the batched ICP and the finish kernel: mode[k] 0 / 1 first scan / 2 second scan; descs: the
// ICP descriptor of every mode-2 stream, in stream order.  Fills out[k] of the mode 1 / 2 streams (synchronises).
int streams_boot_finish(lins_ctx* ctx, const int* mode, const std::vector<ScanDesc>& descs, const StepMachine& mach, lins_result* out);

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

}  // namespace lins
