/*
 * lins_host.h — host-side (CPU, C++ behind a C ABI) pieces that sit either
 * side of the IESKF hot path.  None of this touches the GPU except
 * lins_host_perform_ieskf(), which drives liblins_ieskf.so.
 *
 *   lins_filter_*            mirrors filter::StatePredictor
 *                            (lins/include/KalmanFilter.hpp:118-380): IMU
 *                            propagation + reset(1); produces the prior (x,P)
 *                            performIESKF() starts from.
 *   lins_frontend_*          mirrors image_projection_node's projection /
 *                            ground / segmentation (lins/src/image_projection_node.cpp:191-415)
 *                            and StateEstimator's feature front-end
 *                            (StateEstimator.hpp:619-827); produces the four
 *                            feature clouds performIESKF() reads.
 *   lins_transform_to_end    StateEstimator::transformToEnd (SE:1083-1101), the
 *                            re-projection updatePointCloud() applies to make
 *                            the next scan's target clouds (SE:1116-1139).
 *   lins_synth_*             seeded synthetic VLP-16 scan pairs.
 *   lins_host_perform_ieskf  StateEstimator::performIESKF() as the node sees it
 *                            (SE:465-600): GPU IESKF loop, and on divergence the
 *                            ICP fallback estimateTransform (SE:585-592,
 *                            1163-1320) with GPU correspondences + host 6x6 GN.
 */
#ifndef LINS_HOST_H_
#define LINS_HOST_H_

#include "lins_ieskf.h"
#include "lins_map.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LINS_LINE_NUM 16   /* LINE_NUM  (exp_port.yaml:9)  */
#define LINS_SCAN_NUM 1800 /* SCAN_NUM  (exp_port.yaml:10) */
#define LINS_CLOUD_MAX (LINS_LINE_NUM * LINS_SCAN_NUM)
/* most points of an outlier cloud (IP:300-303): rows above groundScanInd = 5, every fifth column */
#define LINS_OUTLIER_MAX ((LINS_LINE_NUM - 6) * (LINS_SCAN_NUM / 5))

/* ---- StatePredictor ------------------------------------------------------ */
typedef struct lins_filter_params {
  double acc_n, gyr_n, acc_w, gyr_w;                   /* yaml:29-32           */
  double init_pos_std[3], init_vel_std[3], init_att_std[3]; /* yaml:34-50      */
  double init_acc_std[3], init_gyr_std[3];             /* yaml:52-62           */
} lins_filter_params;

typedef struct lins_filter {
  double state[LINS_STATE_DIM];
  double cov[LINS_ERR_DIM * LINS_ERR_DIM];
  double noise[12 * 12];
  double acc_last[3], gyr_last[3];
  double time;
  int32_t has_imu;
  int32_t pad;
  lins_filter_params prm;
} lins_filter;

void lins_filter_default_params(lins_filter_params* p);           /* exp_port.yaml */
/* StatePredictor::initialization-like start: identity state with given v, ba,
 * bw, gravity (0,0,-9.81), covariance = initializeCovariance(0) (KF:247-311).  */
void lins_filter_init(lins_filter* f, const lins_filter_params* p, const double* vn,
                      const double* ba, const double* bw);
void lins_filter_predict(lins_filter* f, double dt, const double* acc,
                         const double* gyr);                      /* KF:125-186  */
void lins_filter_reset1(lins_filter* f);                          /* KF:320-352  */
/* What processScan does after performIESKF (SE:443-453), on the filter and on globalState_ (19 doubles, the layout of a
 * state): filter_->update(posterior) — with used_prior_cov the state only: a diverged update hands over the ICP pose
 * with Pk_ un-updated (SE:585-592), which is the covariance the filter holds —, integrateTransformation (SE:608-617),
 * reset(1), calculateRPfromGravity + correctRollPitch (SE:602-605, 427-431).  The CPU restatement of the streams'
 * finish kernel (csrc/filter_math.h is the arithmetic of both).                                                     */
void lins_filter_finish(lins_filter* f, double* global_state, const lins_result* posterior, int used_prior_cov);

/* ---- the two-scan bootstrap (SE:331-425; on the device: lins_streams_filter.h) ---- */
typedef struct lins_boot_params {
  lins_filter_params filter;
  double init_ba[3], init_bw[3]; /* INIT_BA, INIT_BW (exp_port.yaml:65-76) */
} lins_boot_params;
/* the IMU pre-integration between a stream's first and second scan (IB:179-187; delta_q: w x y z) */
typedef struct lins_preintegration {
  double sum_dt, delta_p[3], delta_q[4], delta_v[3], acc_0[3], gyr_0[3];
} lins_preintegration;
/* ---- CPU restatement of the bootstrap's arithmetic (liblins_host.so, csrc/host/boot.cpp; csrc/boot_math.h is the text
 * of both sides).  The ICP itself is not restated: its pose is an input.                                            */
void lins_host_preintegrate(lins_preintegration* pre, int n_rows, const double* rows /* n_rows x 7: dt, acc, gyr */,
                            const double* init_ba, const double* init_bw);
/* the pose estimateTransform starts from (SE:392-396): t[3], q[4] (w x y z) */
void lins_host_boot_start(const lins_preintegration* pre, double* t, double* q);
/* processFirstScan (SE:339-361): f = the zero initialisation, lin_state19 = identity, pre reset with imu_last;
 * global_state is left as it is (the reference does not touch globalState_ here)                                   */
void lins_host_boot_first(lins_filter* f, double* global_state, double* lin_state19, lins_preintegration* pre,
                          const double imu_last[6], double time, const lins_boot_params* prm);
/* processSecondScan behind estimateTransform (SE:401-415) */
void lins_host_boot_second(lins_filter* f, double* global_state, double* lin_state19, const lins_preintegration* pre,
                           const double icp_t[3], const double icp_q[4], const double imu_last[6], double time,
                           const lins_boot_params* prm);

/* ---- front-end ------------------------------------------------------------ */
typedef struct lins_features {
  lins_point* corner_sharp;      int32_t n_corner_sharp;      /* cap 192  */
  lins_point* corner_less_sharp; int32_t n_corner_less_sharp; /* cap 1920 */
  lins_point* surf_flat;         int32_t n_surf_flat;         /* cap 1024 */
  lins_point* surf_less_flat;    int32_t n_surf_less_flat;    /* cap LINS_CLOUD_MAX */
  int32_t n_segmented;           /* size of the segmented cloud              */
  int32_t n_outlier;
} lins_features;

/* raw: unorganised cloud in firing order (what /velodyne_points carries).
 * Caller allocates the four output arrays with the capacities noted above.   */
int lins_frontend_extract(const lins_point* raw, int n_raw, double scan_period,
                          lins_features* out);

/* ---- front-end, in the reference's two stages ------------------------------ */
/* What image_projection_node publishes and StateEstimator::processPCL consumes: the segmented
 * cloud (sensor_msgs/PointCloud2 of PointXYZI, ring-major, ascending column, intensity =
 * row + col / 10000, IP:234) + cloud_msgs/cloud_info (cloud_info.msg:1-12).                  */
typedef struct lins_segmented_scan {
  const lins_point* cloud;
  const float* range;       /* segmentedCloudRange      */
  const uint32_t* col;      /* segmentedCloudColInd     */
  const uint8_t* ground;    /* segmentedCloudGroundFlag */
  int32_t n;
  int32_t start_ring[LINS_LINE_NUM], end_ring[LINS_LINE_NUM];  /* startRingIndex / endRingIndex */
  float start_ori, end_ori, ori_diff;                          /* startOrientation, ...         */
  int32_t n_outlier;
} lins_segmented_scan;

/* image_projection_node (IP:191-415) on the host: caller-allocated arrays of LINS_CLOUD_MAX
 * entries, `out` is pointed at them.
 * Non-finite returns (here, lins_segment_batch, lins_streams_step_raw): a point with a non-finite x, y or z behaves
 * exactly as if it were not in the cloud (removeNaNFromPointCloud, IP:176) — not projected, not read for the start /
 * end orientation.  Fewer than two finite points: LINS_E_INPUT.  The device entry points accept NaN only: an
 * infinite coordinate is LINS_E_INPUT there (nothing is run).                                                      */
int lins_frontend_segment(const lins_point* raw, int n_raw, lins_point* cloud, float* range, uint32_t* col,
                          uint8_t* ground, lins_segmented_scan* out);
/* The same stage on the device (csrc/segment_kernels.hip): n raw clouds in firing order; out[k]'s four array
 * pointers must point at caller-allocated arrays of LINS_CLOUD_MAX entries (they are written).  Identical
 * to lins_frontend_segment() — the BFS labelling is restated as an order-free min-label propagation.    */
int lins_segment_batch(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw,
                       lins_segmented_scan* out);
int lins_last_segment_ms(lins_ctx* ctx, float* kernel_ms);
/* The third cloud image_projection_node publishes, /outlier_cloud (IP:300-303): the cells of the segments that fail the
 * validity test, in rows above groundScanInd and in every fifth column, in raster order (ring-major, ascending column),
 * as fullCloud points — x, y, z of the cell's owning point, intensity = row + col / 10000 (IP:234).  outlier: caller-
 * allocated, LINS_OUTLIER_MAX entries.  Input contract of lins_frontend_segment.  Returns the count (what
 * lins_frontend_segment reports as n_outlier) or an error.                                                          */
int lins_frontend_segment_outliers(const lins_point* raw, int n_raw, lins_point* outlier);
/* The same cloud from the device's segmentation stage (lins_segment_batch_outliers), and what the streams keep of it for
 * the mapping node (lins_streams_put_outliers, lins_streams_map_cloud), are declared in lins_streams_map.h.            */
/* StateEstimator's feature stage (undistortPcl .. extractFeatures, SE:619-827) on the host — the
 * CPU restatement the device version is checked against.                                      */
int lins_frontend_extract_segmented(const lins_segmented_scan* in, double scan_period, lins_features* out);
/* The same stage on the device (csrc/frontend_kernels.hip): n scans, one
 * workgroup each; out[k]'s four arrays are caller-allocated with the capacities of lins_features.
 * Identical picks and clouds (the relative-time tag within 1 ulp of f32 where atan2f differs).   */
int lins_extract_features_batch(lins_ctx* ctx, int n, const lins_segmented_scan* in, double scan_period,
                                lins_features* out);
/* HIP-event time (ms) of the front-end kernel of the last call and its algorithmic bytes
 * (25 B read per segmented point + 16 B per emitted feature point).                            */
int lins_last_frontend_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* bytes);

/* ---- device-resident streams: front-end -> IESKF update -> re-projection, the clouds never leave HBM ----
 * n independent streams (sensors / robots / replayed logs) advance one scan per call:
 *   1. the feature stage (SE:619-827) of every stream's new segmented scan, into device slots;
 *   2. performIESKF (SE:465-600) of the new sharp / flat clouds against the stream's RESIDENT less-sharp /
 *      less-flat clouds of the previous scan, from the prior (state, covariance) the caller's StatePredictor
 *      supplies; diverged filters take the device ICP fallback (SE:585-592);
 *   3. updatePointCloud (SE:1116-1139): the new less-sharp / less-flat clouds re-projected to the scan end
 *      with the final pose, in place — the next call's targets.
 * A stream's first scan has nothing to match against: no update is run (out[k].iters = 0, state / covariance
 * returned as given) and its clouds are re-projected with the pose in prior_state[k] (the caller's bootstrap
 * guess, SE:331-425 uses the IMU-integrated one).  prior_state: n x 19, prior_cov: n x 324, feature_counts
 * (optional): n x 4 = sharp, less sharp, flat, less flat.
 * A step completes for EVERY stream or not at all: a diverged stream whose clouds cannot take the device ICP
 * fallback (ICP_FREQ != 1, or clouds beyond the grid kernels' limits) keeps its un-updated filter — out[k].diverged
 * set and out[k].reserved[0] = LINS_E_UNSUPPORTED — while the other streams advance normally; a rejected input
 * (LINS_E_INPUT / _ARG / _CAPACITY) advances nothing; a HIP error (LINS_E_HIP) leaves the resident clouds in an
 * unknown state, every later step then returns LINS_E_STATE until lins_streams_init is called again.       */
int lins_streams_init(lins_ctx* ctx, int n_streams);   /* n_streams <= the context's max_batch */
int lins_streams_step(lins_ctx* ctx, const lins_segmented_scan* scans, const double* prior_state,
                      const double* prior_cov, double scan_period, lins_result* out, int32_t* feature_counts);
/* the same step from RAW clouds (firing order): the image_projection stage (IP:191-415) runs on the device
 * too (lins_last_segment_ms reports its kernel time) and hands the segmented scan to the front-end in HBM */
int lins_streams_step_raw(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const double* prior_state,
                          const double* prior_cov, double scan_period, lins_result* out, int32_t* feature_counts);
/* HIP-event times (ms) of the three stages of the last step */
int lins_streams_stats(lins_ctx* ctx, float* frontend_ms, float* update_ms, float* reproject_ms);
/* test aid: a resident cloud of the last scan back to the host (which: 0 less sharp, 1 less flat);
 * returns the point count                                                                            */
int lins_streams_peek(lins_ctx* ctx, int stream, int which, lins_point* out, int cap);

/* The streams' filter on the device — IMU propagation, update from the resident prior, reset, global pose per stream
 * (lins_streams_filter_*, lins_streams_step_imu*) — is declared in lins_streams_filter.h.                            */

/* the front-end's atan2 (csrc/lins_math.h: a fixed f32 operation sequence shared bit for bit by the host
 * restatement and the device kernels; within 2 ulp(pi/4) of the true value).
 * KNOWN DEVIATION from the reference, which calls libm's atan2 where points are BINNED by angle (image row / column
 * IP:217-225, ground angle IP:262, segmentation angle IP:381, relative time SE:630): a point whose angle lies within
 * the last bit of a bin edge may fall into the neighbouring bin.  Measured against an independent glibc-based checker
 * (oracle/frontend_oracle.cpp, tools/frontend_vs_libm.py, profiles/r02_frontend_vs_libm.txt): on clouds with generic
 * azimuths 0 of 18.4 M cells, 0 picks and 0 coordinates differ, 0.8 % of the relative-time tags differ by at most two
 * f32 roundings; on clouds whose every firing sits exactly ON a column edge (the stock synthetic sensor), 22 % of the
 * cells differ — between any two atan2f implementations.                                               */
float lins_host_atan2f(float y, float x);

/* transformToEnd for every point, with the scan's final relative pose
 * (t = linState_.rn_, q = linState_.qbn_ as w,x,y,z). In-place allowed.       */
void lins_transform_to_end(const double* t, const double* q_wxyz, double scan_period,
                           const lins_point* in, int n, lins_point* out);

/* ---- synthetic scan pairs -------------------------------------------------- */
typedef struct lins_synth_pair {
  /* caller-allocated, capacities as in lins_features */
  lins_point* surf_flat;      int32_t n_surf_flat;
  lins_point* corner_sharp;   int32_t n_corner_sharp;
  lins_point* surf_last;      int32_t n_surf_last;
  lins_point* corner_last;    int32_t n_corner_last;
  double state[LINS_STATE_DIM];            /* prior x for performIESKF          */
  double cov[LINS_ERR_DIM * LINS_ERR_DIM]; /* prior P                            */
  double true_t[3], true_q[4];             /* ground-truth relative pose (w,x,y,z) */
  double speed, yaw_rate;
  int32_t n_raw_last, n_raw_new;
} lins_synth_pair;

#define LINS_SYNTH_SEED 0x4C494E53u /* "LINS" */
int lins_synth_generate(uint32_t seed, uint32_t scan_index, lins_synth_pair* out);
/* raw distorted cloud of one synthetic scan (k = 0 or 1), firing order        */
int lins_synth_raw_scan(uint32_t seed, uint32_t scan_index, int k, lins_point* out,
                        int cap);
/* The same for a scene FAMILY: 0 = the room of SURVEY.md section 8d (what the two calls above generate); 1 = "open":
 * open ground to the range limit, ~60 trunks, six far wall segments, 30 % of the returns lost, one box that moves at
 * up to 5 m/s (csrc/host/synth.cpp) — the second workload the parity sweeps and the bench line's scene_b block run.   */
int lins_synth_generate_scene(int scene, uint32_t seed, uint32_t scan_index, lins_synth_pair* out);
int lins_synth_raw_scan_scene(int scene, uint32_t seed, uint32_t scan_index, int k, lins_point* out, int cap);

/* A SEQUENCE of scans along one seeded trajectory (a circle inside the synthetic room) with its IMU: what a
 * lins_fusion_node would receive over any number of consecutive sweeps — the input of the in-situ test of the drop-in
 * boundary (tests/test_gpu_sequence.py).  Sweep k covers [0.1 k, 0.1 (k + 1)) s; 40 IMU samples per sweep.       */
int lins_synth_seq_raw_scan(uint32_t seed, int k, lins_point* out, int cap);
int lins_synth_seq_imu(uint32_t seed, int k, double* acc /* 40 x 3 */, double* gyr /* 40 x 3 */);
int lins_synth_seq_truth(uint32_t seed, double tau, double* xyyaw, double* speed, double* yaw_rate);

/* ---- performIESKF as the node sees it -------------------------------------- */
int lins_host_perform_ieskf(lins_ctx* ctx, const lins_params* prm,
                            const lins_scan_pair* in, lins_result* out,
                            int32_t* used_icp_fallback);

/* ---- the mapping node's local map on the CPU (host/local_map.cpp) ------------
 * The restatement lins_local_map_build is checked against, bit for bit: the last min(window, n_frames) of `frames`
 * (oldest first) moved into the map frame and VoxelGrid-filtered, and the scan's four VoxelGrid passes
 * (LM:1201-1349; include/lins_map.h).  out[c] holds at least as many points as cloud c reads: the window's corner
 * points / surf + outlier points, the scan's corner / surf / outlier / surf + outlier points.  sizes: as
 * lins_local_map_build reports them.  Returns LINS_E_INPUT for a scan / frame / pose outside the input contract
 * (nothing written), else LINS_OK (the entry's own status in sizes->status). */
int lins_host_local_map(const lins_keyframe* frames, int n_frames, int window, const lins_local_scan* scan,
                        lins_point* const* out, lins_local_map_sizes* sizes);

/* ---- the key-frame archive on the CPU (host/keyframe_archive.cpp) ------------
 * The restatements lins_archive_select_radius / _find_loop / _assemble are checked against, bit for bit
 * (include/lins_map.h; the selection is the same inline code in both libraries, host/keyframe_select.h).  poses / times:
 * the key poses of one slot by frame id.  Both return LINS_E_INPUT for a pose outside the local map's input contract. */
/* returns the count of selected frame ids (LINS_E_CAPACITY beyond cap) */
int lins_host_select_radius(const lins_key_pose* poses, int n, const float centre[3], float radius, float pose_leaf,
                            int32_t* ids, int cap);
int lins_host_find_loop(const lins_key_pose* poses, const double* times, int n, const float centre[3], float radius,
                        double now, double min_gap_s, int32_t* closest);
/* one lins_submap_spec over `frames` (frame id = index): out holds at least the points the spec reads (the chosen clouds
 * of the chosen frames, repeats counted).  LINS_E_ARG for a bad id / mask / flag as lins_archive_assemble, LINS_E_INPUT
 * for a chosen frame outside the input contract (nothing written), else LINS_OK (the cloud's own status in info->status). */
int lins_host_submap(const lins_keyframe* frames, int n_frames, const int32_t* ids, int n_ids, int clouds, float leaf,
                     int flags, lins_point* out, lins_submap_info* info);
/* extractSurroundingKeyFrames with the loop closure off (LM:1247-1315; lins_streams_map_surround in lins_streams_map.h).
 * The list rule (LM:1261-1308, host/keyframe_select.h surround_update — the text the step compiles too): entries of
 * `list` (surroundingExistingKeyPosesID, n_list ids, room for cap) whose id is not among ds are erased, the survivors
 * keep their order; then each ds[i], in order, is appended unless the list holds it already (an id ds names twice enters
 * once).  An id of ds is taken as it is.  Returns the new length; LINS_E_CAPACITY (list untouched) when it would exceed
 * cap. */
int lins_host_surround_update(int32_t* list, int n_list, int cap, const int32_t* ds, int n_ds);
/* CPU restatement of lins_local_map_build_surround for one entry, a composition of the two restatements above: the map
 * clouds are lins_host_submap(list, CORNER, 0.2) and lins_host_submap(list, SURF | OUTLIER, 0.4), the four scan clouds
 * lins_host_local_map's.  out / sizes: as lins_host_local_map (out[0], out[1]: room for the points the list's frames
 * hold); sizes->frames = n_list.  LINS_E_ARG for an id outside [0, n_frames). */
int lins_host_surround_map(const lins_keyframe* frames, int n_frames, const int32_t* list, int n_list,
                           const lins_local_scan* scan, lins_point* const* out, lins_local_map_sizes* sizes);

/* ---- the team map on the CPU: the selection over the slots of a team and the surround map over (slot, id) pairs ---------
 * lins_keyposes_team_select_batch's definition (csrc/host/team_select.h, the same inline code in both libraries; the
 * contract is in lins_map.h).  Target t is slot slots[t] with the counts[t] key poses at poses[t], by frame id; pairs gets
 * the survivors as (slot, id), ascending.  Returns their count; LINS_E_ARG for a slot named twice or negative,
 * LINS_E_INPUT for a pose outside the input contract, LINS_E_CAPACITY for a cell box of more than 2^31 cells or more than
 * cap survivors (nothing written). */
int lins_host_team_select(int n_targets, const int32_t* slots, const lins_key_pose* const* poses, const int32_t* counts,
                          const float centre[3], float radius, float pose_leaf, int32_t* pairs, int cap);
/* CPU restatement of lins_local_map_build_team for one entry: lins_host_surround_map over the frames the n_pairs
 * (slot, id) pairs name, in list order (frames[s]: the n_frames[s] frames of slot s by id).  sizes->frames = n_pairs.
 * LINS_E_ARG for a pair whose slot or id does not exist. */
int lins_host_team_map(int n_slots, const lins_keyframe* const* frames, const int32_t* n_frames, const int32_t* pairs, int n_pairs,
                       const lins_local_scan* scan, lins_point* const* out, lins_local_map_sizes* sizes);

/* ---- the loop-closure ICP on the CPU (host/loop_icp.cpp) ---------------------
 * The restatement lins_loop_icp_batch / lins_loop_icp_correspondences are checked against (include/lins_map.h has the
 * contract; the arithmetic is csrc/loop_icp_math.h in both libraries, the search here is the exhaustive one).  Clouds:
 * finite, |coord| <= 1e6 (LINS_E_INPUT).  lins_loop_icp_default_params is exported by this library too. */
typedef struct lins_loop_icp_round { /* one round of the loop, for the trace */
  double T_in[16];  /* T entering the round */
  double delta[16]; /* the round's fit (identity when it stopped for too few correspondences) */
  double T_out[16]; /* T leaving it */
  double mse;
  double stop[4];   /* 0.5 (trace R_delta - 1), |t_delta|^2, |mse - mse_prev|, |mse - mse_prev| / mse_prev */
  int32_t n_corr;
  int32_t reason;   /* LINS_ICP_NONE: the loop went on */
} lins_loop_icp_round;
/* max_rounds: 0, or the loop stops after that many rounds as under lins_debug_loop_icp_rounds */
int lins_host_loop_icp(const lins_point* source, int n_source, const lins_point* target, int n_target, const lins_loop_icp_params* prm,
                       int max_rounds, lins_loop_icp_result* out);
/* the same with every round recorded (the first cap_rounds of them); returns the number of rounds run or an error */
int lins_host_loop_icp_trace(const lins_point* source, int n_source, const lins_point* target, int n_target, const lins_loop_icp_params* prm,
                             lins_loop_icp_round* rounds, int cap_rounds, lins_loop_icp_result* out);
/* steps 1-2 at T by exhaustive search (cap <= 0: none): index (-1: none) and d (0 where none) per source point */
int lins_host_loop_icp_correspondences(const lins_point* source, int n_source, const lins_point* target, int n_target, const double T[16],
                                       float cap, int32_t* idx, float* sqdist);
/* One problem between two rounds, as the step takes and leaves it (csrc/loop_icp_math.h State without its device-only words):
 * a fresh problem has T = identity, mse_prev = DBL_MAX, mse = 0, fitness = DBL_MAX, the counts 0 and active = 1. */
typedef struct lins_loop_icp_state {
  double T[16];
  double mse_prev, mse, fitness;
  float move[12]; /* out only: the upper three rows of T rounded to f32, the next round's M */
  int32_t iterations, converged, reason, n_corr, n_fitness, active;
} lins_loop_icp_state;
/* Steps 3-6 of ONE round from its 17 sums (0: count  1-3: S x'  4-6: S g  7-15: S x'_i g_j at 7 + 3 i + j  16: S d), handed
 * over instead of found by the search — the test entry of the fit and the stop rule (tests/test_loop_fit_inputs.py; the
 * device's is lins_debug_loop_icp_step).  mode 0: the round — a state with active = 0 is left as it is, as the device's
 * step kernel leaves it; delta (the round's fit; identity when it stopped for too few correspondences) and stop (the four
 * quantities of lins_loop_icp_round.stop; zeros then) are written.  mode 1: the fitness pass, n_fitness and fitness =
 * sums[16] / sums[0] (DBL_MAX at a count of 0), whatever `active` says; delta and stop are not touched and may be null. */
int lins_host_loop_icp_step(const double sums[17], const lins_loop_icp_params* prm, int mode, lins_loop_icp_state* state,
                            double delta[16], double stop[4]);
/* LM:1156-1166, all f32: T -> (x, y, z, roll, pitch, yaw) by roll = atan2(T21, T22), pitch = asin(-T20), yaw =
 * atan2(T10, T00); correctionLidar = getTransformation(z, x, y, yaw, roll, pitch); tWrong = getTransformation(wrong.z,
 * wrong.x, wrong.y, wrong.yaw, wrong.roll, wrong.pitch); pose_from = the same extraction of correctionLidar * tWrong.
 * getTransformation(x, y, z, roll, pitch, yaw) = Rz(yaw) Ry(pitch) Rx(roll) with translation (x, y, z).  The factor
 * graph stays with the caller. */
int lins_host_loop_pose_from(const double T[16], const lins_key_pose* wrong, lins_key_pose* pose_from);
/* What the loop thread decides between its device stages (csrc/host/loop_step.h: the text lins_loop_step compiles too;
 * DESIGN.md §5.3 "Loop thread's step").
 * window (LM:1087-1098): the ids closest - search_num .. closest + search_num clipped to [0, latest], ascending — it may
 * contain `latest`; returns the count (0 for latest < 0, a closest outside [0, latest] or search_num < 0), LINS_E_CAPACITY
 * beyond cap.
 * candidate: LINS_LOOP_NONE for closest < 0 or closest == latest (a frame is no loop with itself), LINS_LOOP_REPEAT when
 * (latest, closest) is the pair of the slot's most recent loop factor (-1, -1: none yet), else -1: the pair is aligned.
 * accept (LM:1140-1141): converged && !(fitness > (double)max_fitness), 1 or 0.  A NaN passes, as in the reference's
 * expression; the variance stops it.
 * variance (LM:1171-1175): *variance = (double)(float)fitness; returns 1 when it is finite and > 0, else 0 — a rejection.
 * choose (lins_loop_step_place): among k verified candidates the rank with the smallest fitness of those `accept`
 * accepts, the lower rank at a tie; -1 when none is accepted (k <= 0 included). */
int lins_host_loop_window(int latest, int closest, int search_num, int32_t* ids, int cap);
int lins_host_loop_candidate(int latest, int closest, int last_latest, int last_closest);
int lins_host_loop_accept(int converged, double fitness, float max_fitness);
int lins_host_loop_variance(double fitness, double* variance);
int lins_host_loop_choose(int k, const int32_t* converged, const double* fitness, float max_fitness);

/* ---- the mapping node's own pose arithmetic (csrc/map_pose_math.h; the CPU restatement of lins_streams_map_step's two
 * kernels, lins_streams_map.h).  Pose vectors are (rx, ry, rz, tx, ty, tz) as transformTobeMapped; all f32.
 * transformAssociateToMap (LM:411-536): transformTobeMapped from transformBefMapped, transformAftMapped, transformSum.
 * |rx| of the result near pi / 2 is outside the contract (the reference divides by its cosine).                      */
void lins_host_map_associate(const float bef[6], const float aft[6], const float sum[6], float tobe[6]);
/* the tail of transformUpdate (LM:567-576): with has_imu the blend tobe[0] <- 0.998 tobe[0] + 0.002 imu_pitch, tobe[2]
 * <- 0.998 tobe[2] + 0.002 imu_roll (f64, rounded once to f32); then bef <- sum, aft <- tobe.  imu_roll / imu_pitch
 * are imuHandler's interpolation (LM:539-565), the caller's.                                                        */
void lins_host_map_transform_update(float tobe[6], int has_imu, float imu_roll, float imu_pitch, const float sum[6], float bef[6], float aft[6]);
/* the key-frame rule (LM:1655-1671): returns 1 when the scan becomes a key frame — the f32 distance of prev
 * (previousRobotPosPoint) to aft[3..5] is not < 0.3, or have_frames == 0 — and then sets prev to aft[3..5]          */
int lins_host_map_key_rule(float prev[3], const float aft[6], int have_frames);

/* ---- the seam between the filter and the mapping node on the CPU (host/odom.cpp) ------------------------------------
 * The restatement the odometry and fusion kernels are checked against (csrc/odom_math.h in both libraries; the entry
 * points for streams: lins_streams_slam.h).  tf's arithmetic is stated there, in f64.                                 */
typedef struct lins_stream_odom {   /* /laser_odom_to_init of one stream + the mapping node's transformSum */
  double position[3], orientation[4];   /* globalStateYZX_: rn_, qbn_ as (x, y, z, w) */
  float transform_sum[6];               /* transformSum (LM:711-724) */
  int32_t valid, reserved;              /* valid 0: the stream has no globalState_ yet, or it is not finite */
} lins_stream_odom;
typedef struct lins_fused_pose {    /* /integrated_to_init (TF:217-254) */
  float transform_mapped[6];            /* transformMapped (TF:91-215) */
  double orientation[4];                /* (x, y, z, w) as laserOdometry2 */
} lins_fused_pose;
/* globalState_ (19 doubles: rn_ 0-2, qbn_ 6-9 as w, x, y, z) to the record: the exact axis permutation of SE:1152-1154,
 * then laserOdometryHandler (LM:711-724).  A non-finite rn_ / qbn_ or transformSum: valid = 0, everything else zero.  */
void lins_host_odom_from_global(const double* gs19, lins_stream_odom* out);
/* the orientation published with a pose (rx, ry, rz, tx, ty, tz): tf's setRPY(t[2], -t[0], -t[1]) sent as (-y, -z, x, w) */
void lins_host_pose_quat(const float* t6, double* q4);
/* the transform fusion node: transformMapped = lins_host_map_associate(bef, aft, sum), orientation = lins_host_pose_quat */
void lins_host_fuse(const float* bef6, const float* aft6, const float* sum6, lins_fused_pose* out);

/* ---- the pose graph on the CPU (host/pose_graph.cpp) ---------------------------------------------------------------
 * The restatement lins_pose_graph_* is checked against (include/lins_map.h has the contract; the arithmetic is
 * csrc/pose_graph_math.h and the solve csrc/pose_graph.h in both libraries: the same phases in the same order, so host
 * and device differ only where libm does).  One graph per handle; the calls and their errors are the device's.
 * lins_pose_graph_default_params is exported by this library too. */
typedef struct lins_host_pose_graph lins_host_pose_graph;
lins_host_pose_graph* lins_host_pose_graph_create(int max_frames, int max_loops);
void lins_host_pose_graph_destroy(lins_host_pose_graph* g);
int lins_host_pose_graph_push(lins_host_pose_graph* g, const float last6[6], const float aft6[6]);
int lins_host_pose_graph_add_loop(lins_host_pose_graph* g, int latest_id, int closest_id, const lins_key_pose* pose_from, double fitness);
int lins_host_pose_graph_solve(lins_host_pose_graph* g, const lins_pose_graph_params* prm, lins_pose_graph_result* out);
int lins_host_pose_graph_poses(lins_host_pose_graph* g, int first_id, int n, lins_key_pose* out);
int lins_host_pose_graph_count(lins_host_pose_graph* g, int32_t* n_loops);
int lins_host_pose_graph_poses_f64(lins_host_pose_graph* g, int first_id, int n, double* out); /* n x 12: R row-major, t */
int lins_host_pose_graph_loop_z(lins_host_pose_graph* g, int loop, double z[12]);
/* The rebase of include/lins_team.h lins_pose_graph_rebase_batch on the CPU, through the same csrc/pose_graph.h text:
 * Z[0] <- X Z[0] by one product, every pose formed again by the solve's phase_poses from the increments as they stand.  X: 4 x 4
 * row-major f64 in the archive's axes.  LINS_E_ARG for a graph without frames, LINS_E_INPUT for an X that lins_team.h refuses;
 * a refused call changes nothing. */
int lins_host_pose_graph_rebase(lins_host_pose_graph* g, const double X[16]);
/* The linearisation at given absolute poses (N x 12; NULL: the estimate), for the finite-difference test: per odometry
 * factor k = 1 .. N - 1 the residual r_odo[6 (k - 1)], the Hessian block D[36 (k - 1)] = J^T Sigma^-1 J and the gradient
 * g[6 (k - 1)] = J^T Sigma^-1 r with respect to the right perturbation of the increment T_{k-1}^-1 T_k; per loop l the
 * residual r_loop[6 l] and M[36 l], the loop's rows being J_{l,k} = M_l Ad(T_k) for min(b, a) < k <= max(b, a).  Any
 * output may be NULL. */
int lins_host_pose_graph_linearize(lins_host_pose_graph* g, const double* poses, double* r_odo, double* D, double* gvec, double* r_loop, double* M);
/* six floats (pitch, yaw, roll, y, z, x) <-> pose (12 doubles) */
void lins_host_pose_from6(const float p[6], double T[12]);
void lins_host_pose_to6(const double T[12], float p[6]);

/* ---- the team graph on the CPU (host/team_graph.cpp) -----------------------------------------------------------------
 * The restatement lins_team_graph_solve is checked against (include/lins_team.h has the contract; the text of the solve
 * is csrc/pose_graph_team.h in both libraries).  The records are the device call's. */
typedef struct lins_team_factor {
  int32_t slot_b, id_b, slot_a, id_a;
  double Z[12]; /* the measurement T_b^-1 T_a as a pose in the graph's axes: R row-major, then t */
  double var;
} lins_team_factor;
typedef struct lins_team_member {
  int32_t slot, reserved;
  double root_variance[6]; /* rotation first; ignored for a group's first member */
} lins_team_member;
typedef struct lins_team_graph_result {
  lins_pose_graph_result solve;
  int32_t n_frames, n_loops, n_factors, reserved; /* of the group: frames of all members, their own loops, its factors */
} lins_team_graph_result;
/* out->Z = (X Tb)^-1 Ta, out->var = (double)(float)fitness, the slots and ids zero.  Tb, Ta: poses of 12 doubles in the
 * graph's axes; X: 4 x 4 row-major f64 in the archive's axes, NULL: the identity.  LINS_E_INPUT for an X that
 * lins_host_pose_graph_rebase refuses or a fitness that is not finite and > 0. */
int lins_host_team_factor(const double Tb[12], const double Ta[12], const double* X, double fitness, lins_team_factor* out);
/* ONE group: graphs[0] is the anchor; root_variance holds 6 doubles per member (member 0's are not read); a factor's
 * slot_b / slot_a are member indices.  Refusals and what the solve leaves in every graph: lins_team_graph_solve's (the
 * capacity asked against min(64, the sum of the graphs' max_loops)). */
int lins_host_team_graph_solve(int n_members, lins_host_pose_graph* const* graphs, const double* root_variance, int n_factors,
                               const lins_team_factor* factors, const lins_pose_graph_params* prm, lins_team_graph_result* out);
/* The linearisation of what a team adds, at given absolute poses of all members back to back (sum of N_m x 12; NULL: the
 * estimates), for the finite-difference test: per team factor its residual r_factor[6 i] and M[36 i] (the factor's rows
 * are + M Ad(T_k) over chain a up to id_a and - M Ad(T_k) over chain b up to id_b); per non-anchor member m = 1 .. the
 * root factor's residual r_root[6 (m - 1)], Hessian block H_root[36 (m - 1)] and gradient g_root[6 (m - 1)] with respect
 * to the right perturbation of T_0.  Any output may be NULL. */
int lins_host_team_graph_linearize(int n_members, lins_host_pose_graph* const* graphs, const double* root_variance, int n_factors,
                                   const lins_team_factor* factors, const double* poses, double* r_factor, double* M, double* r_root,
                                   double* H_root, double* g_root);

/* ---- pairwise-consistent team factors on the CPU (host/team_pcm.cpp): the DEFINITION of include/lins_team.h's
 * lins_team_factors_consistent_batch --------------------------------------------------------------------------------
 * Per pair of members, the largest set of a group's team factors that agree with each other TWO BY TWO (pairwise
 * consistency maximisation; DESIGN.md §5.3 "Pairwise-consistent team factors"; the scalar text is csrc/host/team_pcm.h,
 * the same inline code in both libraries).  f64, products and sums in the order written, contraction off, no libm.
 *   record      of a factor: u < v its two members, iu, iv its frames on them; Zn = Z where slot_b is u, else inverse(Z);
 *               X = compose(compose(Tu, Zn), inverse(Tv)), the transform from v's map frame to u's that the factor claims
 *               (Tu, Tv: the two frames' f64 estimates); p = the translation of Tv.  X depends on the two chains' relative
 *               poses only: it can be asked before any rebase.
 *   consistent  l != m: the same (u, v), NOT the same (iu, iv) — two factors on one frame pair witness nothing for each
 *               other —, sum_ij Rl[i][j] Rm[i][j] >= 1 + 2 min_cos_rotation and, for p in {p_l, p_m}, |X_l p - X_m p|^2 <=
 *               t^2, t = max_translation + translation_per_frame (|iu_l - iu_m| + |iv_l - iv_m|); the sums as
 *               lins_host_rendezvous_consensus forms them.  Symmetric by construction.
 *   search      per factor s, in index order, the best clique whose smallest member is s: depth first, candidates in
 *               ascending index order, cut where |R| + |P| cannot beat the best; its own node counter (a node is a call
 *               of the recursive statement), stopped beyond max_nodes with the best so far.  A pair's clique is the
 *               subproblem result of largest size, then smallest s: where nothing ran out, the maximum clique with the
 *               lexicographically smallest ascending index list.  A caller who prefers some factors lists them first.
 *   kept        a pair's clique is kept iff its size >= min_support; a group's kept set is the union over its pairs */
#define LINS_TEAM_PCM_MAX_FACTORS 64
typedef struct lins_team_pcm_params {
  double max_translation;       /* 1.0 m (finite, >= 0) */
  double min_cos_rotation;      /* 0.99619469809174555 = cos 5 degrees, as lins_consensus_params (not a NaN) */
  double translation_per_frame; /* 0.0 (finite, >= 0): metres the bar grows per frame between two factors, for drift */
  int32_t min_support;          /* 3 (>= 1) */
  int32_t max_nodes;            /* 65536 per subproblem (>= 1) */
} lins_team_pcm_params;
void lins_team_pcm_default_params(lins_team_pcm_params* p); /* exported by both libraries */

typedef struct lins_team_pcm_result {
  int32_t n_factors, n_kept, n_pairs, n_pairs_kept; /* pairs: member pairs with a factor; kept: with a kept clique */
  int32_t exact;      /* 1 iff no subproblem ran out of nodes */
  uint32_t nodes_max; /* the largest subproblem's node counter (max_nodes + 1 where it ran out) */
  uint32_t kept[2];   /* factor f is bit f % 32 of kept[f / 32] */
} lins_team_pcm_result; /* 32 bytes */

/* ONE group of n_factors in [0, LINS_TEAM_PCM_MAX_FACTORS] factors whose slot_b / slot_a are member indices; Tb, Ta: 12
 * doubles per factor, the f64 estimates of frame id_b of slot_b and of frame id_a of slot_a (R row-major, t).
 * LINS_E_ARG: a null pointer, n_factors < 0, max_translation not finite or < 0, a NaN min_cos_rotation,
 * translation_per_frame not finite or < 0, min_support or max_nodes < 1, a factor naming one member twice, a negative slot
 * or id.  LINS_E_INPUT: a Z lins_host_team_graph_solve refuses (an entry that is not finite, no rotation), a pose entry that is
 * not finite, a var that is not finite and > 0 — a kept list is one the solve takes.  LINS_E_CAPACITY: more than
 * LINS_TEAM_PCM_MAX_FACTORS factors.  A refused call writes nothing. */
int lins_host_team_factors_consistent(int n_factors, const lins_team_factor* factors, const double* Tb, const double* Ta,
                                      const lins_team_pcm_params* prm, lins_team_pcm_result* out);
/* The search and the winners alone, on n in [0, 64] vertices: adj[a] bit b = a and b are consistent, pair[a] = any key of
 * a's member pair.  Of prm min_support and max_nodes are read.  LINS_E_ARG: a null pointer, n out of range, parameters as
 * above, a row with a bit at or beyond n or at its own index, rows that are not symmetric, an edge between two keys. */
int lins_host_team_pcm_clique(int n, const uint64_t* adj, const int32_t* pair, const lins_team_pcm_params* prm, lins_team_pcm_result* out);

/* ---- place recognition on the CPU (host/place.cpp) -----------------------------------------------------------------
 * The DEFINITION the device calls of include/lins_place.h are held to, bit for bit (the scalar text is
 * csrc/host/place_math.h in both libraries; DESIGN.md §5.3 "Place recognition").  A descriptor is LINS_PLACE_CELLS f32,
 * D[ring][sector] row-major.  Clouds: finite, |coord| <= 1e6 (LINS_E_INPUT). */
#define LINS_PLACE_RINGS 20
#define LINS_PLACE_SECTORS 60
#define LINS_PLACE_CELLS (LINS_PLACE_RINGS * LINS_PLACE_SECTORS)
typedef struct lins_place_params {
  float r_max;     /* 80 m: points at or beyond it are dropped */
  float lift;      /* 2 m: added to every height */
  int32_t up_axis; /* 1: index of the vertical coordinate of the stored clouds (0, 1 or 2) */
  int32_t clouds;  /* LINS_SUBMAP_CORNER | _SURF | _OUTLIER: the clouds of a frame that are described */
} lins_place_params;
void lins_place_default_params(lins_place_params* p); /* exported by both libraries */
/* the descriptor of one frame; the frame's pose is not read; the clouds outside prm->clouds are skipped */
int lins_host_place_descriptor(const lins_keyframe* frame, const lins_place_params* prm, float out[LINS_PLACE_CELLS]);
/* one pair under every shift: d[k], k < LINS_PLACE_SECTORS */
int lins_host_place_distance(const float* query, const float* candidate, float d[LINS_PLACE_SECTORS]);
/* the minimum of (d, id, shift) over the n candidates (descs: n x LINS_PLACE_CELLS) with fabs(times[c] - now) >
 * min_gap_s and c != skip_id (-1: skip none); *id = -1 without one (then *shift = 0, *distance = 1).  candidates (may
 * be NULL): how many were admissible.  LINS_E_INPUT for a NaN gap or a now that is not finite. */
int lins_host_place_search(const float* query, const float* descs, const double* times, int n, int skip_id, double now, double min_gap_s,
                           int32_t* id, int32_t* shift, float* distance, int32_t* candidates);
/* The k best SEPARATED candidates of the same search (the definition of lins_place_topk_batch).  A candidate's row key
 * is the minimum of (d, id, shift) over its shifts.  Rank 0 is the minimum row key — lins_host_place_search's answer;
 * rank j the minimum among the candidates c with |c - ids[i]| > min_sep for every earlier rank i; the ranks end at k or
 * when no admissible candidate is left.  Returns the number of ranks filled (>= 0); the k - filled entries behind them
 * are id -1, shift 0, distance 1.  LINS_E_ARG for k outside [1, LINS_PLACE_MAX_K] or min_sep < 0. */
#define LINS_PLACE_MAX_K 8
int lins_host_place_topk(const float* query, const float* descs, const double* times, int n, int skip_id, double now, double min_gap_s, int k,
                         int min_sep, int32_t* ids, int32_t* shifts, float* distances, int32_t* candidates);
/* T0 = M_c R_up(shift 2 pi / LINS_PLACE_SECTORS) M_q^-1 in f64, row-major: the start transform of an ICP whose source is
 * the query frame assembled at its stored pose and whose target lies around the candidate's.  M: a key pose as the
 * archive's assembly applies it, R = Ry(pitch) Rx(roll) Rz(yaw) with translation (x, y, z).  Shift k: what the query
 * sees at azimuth phi the candidate sees at phi + k 2 pi / LINS_PLACE_SECTORS, azimuth growing from axis (up + 1) % 3
 * towards axis (up + 2) % 3.  LINS_E_ARG for a bad axis or shift. */
int lins_host_place_guess(const lins_key_pose* pose_q, const lins_key_pose* pose_c, int shift, int up_axis, double T0[16]);
/* lins_host_loop_icp with T_0 given instead of the identity (LINS_E_INPUT when it is not finite) */
int lins_host_loop_icp_from(const lins_point* source, int n_source, const lins_point* target, int n_target, const double T0[16],
                            const lins_loop_icp_params* prm, int max_rounds, lins_loop_icp_result* out);

/* ---- team search on the CPU (host/place.cpp): the DEFINITION of include/lins_team.h's lins_place_team_topk_batch -----
 * One query frame against the frames of MANY slots (DESIGN.md §5.3 "Rendezvous"; the scalar text is the lower part of
 * csrc/host/place_math.h).  Ring key of a frame: occ[r] = the number of sectors with D[r][s] > 0 — it does not change
 * when the frame turns about the vertical.  Key distance dk = the sum over the rings of (occ_q[r] - occ_c[r])^2, an
 * integer.  A candidate (s, c) is admissible iff s != query_slot, or c != query_id and fabs(time_c - now) > min_gap_s:
 * the time gate holds inside the query's own slot only.
 *   shortlist  the `shortlist` smallest (dk, slot, id) over the admissible candidates of the target slots (fewer when
 *              fewer exist): a total order, so the list does not depend on the order of the targets
 *   row key    of the candidate at shortlist position m: the minimum of (d, m, shift) over the shifts, d as
 *              lins_host_place_distance gives it — equal distances resolve by dk, then slot, then id
 *   top-K      rank 0 = the minimum row key; rank j = the minimum among the shortlisted candidates that are not in
 *              conflict with an earlier rank: same slot and |id - id_i| <= min_sep */
#define LINS_PLACE_MAX_SHORTLIST 64
#define LINS_PLACE_MAX_TEAM_SLOTS 65536 /* slot numbers a shortlist key holds */
typedef struct lins_place_team_params {
  int32_t shortlist; /* 32: candidates that reach the full comparison, in [1, LINS_PLACE_MAX_SHORTLIST] */
  int32_t k;         /* 4: ranks returned, in [1, LINS_PLACE_MAX_K] */
  int32_t min_sep;   /* 0: two ranks of one slot lie more than this many ids apart (>= 0) */
  int32_t reserved;
} lins_place_team_params;
void lins_place_team_default_params(lins_place_team_params* p); /* exported by both libraries */

typedef struct lins_place_team_result {
  int32_t slot, id;   /* -1, -1: the rank is not filled (then shift 0, distance 1, dk -1) */
  int32_t shift;
  float distance;
  int32_t dk;         /* the key distance that shortlisted it */
  int32_t candidates; /* admissible candidates of the entry, over every target slot */
  int32_t status;
  int32_t reserved;
} lins_place_team_result;

/* query: the descriptor of frame query_id of slot query_slot.  Target t is slot target_slots[t] (each in [0,
 * LINS_PLACE_MAX_TEAM_SLOTS), no slot twice: LINS_E_ARG) with counts[t] frames, descriptors descs[t] (counts[t] x
 * LINS_PLACE_CELLS) and times times[t]; counts[t] = 0 is allowed.  out: prm->k records.  Returns the ranks filled (>= 0);
 * LINS_E_ARG for parameters out of range, LINS_E_INPUT for a NaN gap or a now that is not finite. */
int lins_host_place_team_topk(const float* query, int query_slot, int query_id, double now, double min_gap_s, int n_targets,
                              const int32_t* target_slots, const float* const* descs, const double* const* times, const int32_t* counts,
                              const lins_place_team_params* prm, lins_place_team_result* out);
/* lins_host_place_guess's formula for lins_rendezvous_step, the poses taken from two slots: T0 takes the query slot's map
 * frame into the candidate's.  Every sine and cosine comes from one sincos call, so that both libraries form the same
 * bits whatever their compilers make of adjacent sin and cos calls (lins_host_place_guess's bits differ by an ulp
 * between the two libraries at some angles, e.g. shift 8). */
int lins_host_place_team_guess(const lins_key_pose* pose_q, const lins_key_pose* pose_c, int shift, int up_axis, double T0[16]);
/* the ring key of a descriptor: occ[LINS_PLACE_RINGS] and the sum of their squares */
int lins_host_place_ring_key(const float* desc, uint8_t occ[LINS_PLACE_RINGS], uint32_t* sumsq);

/* ---- rendezvous over a window on the CPU: the DEFINITION of include/lins_team.h's lins_rendezvous_consensus_batch -------
 * Which of the alignments of several query frames agree on one transform (DESIGN.md §5.3 "Rendezvous over a window"; the
 * scalar text is csrc/host/rendezvous_consensus.h, the same inline code in both libraries).  f64, products and sums in
 * the order written, contraction off.
 *   consistent  a != b are consistent iff both are admissible, name the same target_slot, come from different `query`,
 *               sum_ij Ra[i][j] Rb[i][j] >= 1 + 2 min_cos_rotation (the trace of Ra^T Rb, row-major from the left) and,
 *               for p in {p_a, p_b}, d = Xa p - Xb p has (dx dx + dy dy) + dz dz <= max_translation^2; a coordinate of
 *               X p is ((r0 px + r1 py) + r2 pz) + t.  Symmetric by construction.
 *   support     of a: the number of distinct `query` among a and the hypotheses consistent with a (0 when a is not
 *               admissible)
 *   winner      the admissible hypothesis with the largest support, then the smallest fitness, then the largest `query`
 *               (the more recent frame), then the smallest rank; its members are itself and the hypotheses consistent
 *               with it — a star: two members may differ from each other by up to twice the bars */
#define LINS_RENDEZVOUS_MAX_WINDOW 16
#define LINS_RENDEZVOUS_MAX_HYP (LINS_RENDEZVOUS_MAX_WINDOW * LINS_PLACE_MAX_K) /* 128 */
typedef struct lins_consensus_hyp {
  double X[16];        /* row-major, as lins_loop_icp_result.transform: the asking slot's map frame to target_slot's */
  double p[3];         /* the stored key-pose position of its query frame, in the archive's axes */
  double fitness;
  int32_t query;       /* which frame of the window it came from, in [0, LINS_RENDEZVOUS_MAX_WINDOW) */
  int32_t rank;        /* in [0, LINS_PLACE_MAX_K); no (query, rank) twice in one table */
  int32_t target_slot;
  int32_t admissible;  /* 0 or 1 */
} lins_consensus_hyp;  /* 176 bytes */

typedef struct lins_consensus_params {
  int32_t window;          /* 5: frames asked, in [1, LINS_RENDEZVOUS_MAX_WINDOW] */
  int32_t stride;          /* 1: the queries are the frames latest - j stride (>= 1) */
  int32_t min_support;     /* 3: frames that must agree, in [1, window] */
  int32_t reserved;
  double max_translation;  /* 1.0 m (finite, >= 0) */
  double min_cos_rotation; /* 0.99619469809174555 = cos 5 degrees (not a NaN): there is no libm on the device, the caller passes the cosine */
} lins_consensus_params;
void lins_rendezvous_consensus_default_params(lins_consensus_params* p); /* exported by both libraries */

typedef struct lins_consensus_result {
  int32_t winner;       /* its index in the table, -1 when nothing is admissible (then support 0, no member) */
  int32_t support;
  int32_t n_admissible;
  int32_t reserved;
  uint32_t members[4];  /* hypothesis h is bit h % 32 of members[h / 32] */
} lins_consensus_result; /* 32 bytes */

/* One table of n_hyp hypotheses in [0, LINS_RENDEZVOUS_MAX_HYP].  Of prm only max_translation and min_cos_rotation are
 * read.  LINS_E_ARG for a null pointer, n_hyp out of range, a bar out of range, a query or rank out of range, an
 * `admissible` other than 0 or 1 or a (query, rank) named twice; LINS_E_INPUT for an admissible hypothesis with an entry
 * of X or p that is not finite or a fitness that is not finite or < 0 (an inadmissible one is not read beyond its four
 * integers).  A refused call writes nothing. */
int lins_host_rendezvous_consensus(const lins_consensus_hyp* hyp, int n_hyp, const lins_consensus_params* prm, lins_consensus_result* out);

#ifdef __cplusplus
}
#endif
#endif
