/*
 * lins_streams_slam.h — streams end to end: the filter's global pose feeds the mapping step on the device (entry points
 * of liblins_ieskf.so; csrc/lins_streams_slam_capi.hip, kernels csrc/odom_kernels.hip, scalar text csrc/odom_math.h; the
 * host restatement lins_host_odom_from_global / lins_host_pose_quat / lins_host_fuse and the record types
 * lins_stream_odom / lins_fused_pose are in lins_host.h).
 *
 * What a caller of lins_streams_process_raw + lins_streams_map_step had to write per scan and per stream —
 * updatePointCloud's XYZ -> YZX change of globalState_ and publishOdometryYZX (SE:1150-1154, EC:294-305), the mapping
 * node's laserOdometryHandler (LM:711-724) and the transform fusion node (TF:91-254) — with the global states downloaded
 * and the rows uploaded again in between.  Here globalState_ is read where the filter leaves it and the map pose where
 * the mapping step leaves it.
 *
 * tf is not part of the reference's text: the arithmetic of tf::Matrix3x3::setRotation / getRPY and
 * tf::Quaternion::setRPY is stated in csrc/odom_math.h, in f64 (DESIGN.md section 5.3 "Streams end to end").  The YZX
 * change is the exact axis permutation; Eigen's quaternion products differ from it by their f64 rounding only.
 */
#ifndef LINS_STREAMS_SLAM_H_
#define LINS_STREAMS_SLAM_H_

#include "lins_streams_filter.h"
#include "lins_streams_map.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lins_slam_imu { /* imuHandler's output for one scan of one stream (LM:539-565), as lins_map_odom */
  float roll, pitch;           /* imuRollLast, imuPitchLast; read with has_imu */
  int32_t has_imu, reserved;
} lins_slam_imu;

/* One kernel derives every stream's record from the resident globalState_ (after lins_streams_init; n_streams of it).
 * The records stay resident — lins_streams_map_step_resident and lins_streams_fuse read them — and out (optional,
 * n_streams records) receives them.  A stream without a globalState_ (no filter loaded; in machine mode: not
 * LINS_STREAM_RUNNING — not yet BOOTED, thrown back to INIT) has valid = 0 and zeros.  A non-finite globalState_ can
 * be reached through the ABI — lins_streams_filter_set does not look at the 19 numbers it is given — and gives
 * valid = 0 as well.  Synchronises.                                                                                  */
int lins_streams_odometry(lins_ctx* ctx, lins_stream_odom* out);

/* lins_streams_map_step (lins_streams_map.h) with transformSum read from the resident record of each entry's stream:
 * the records are derived anew from globalState_ as it lies (lins_streams_odometry's kernel), then gate, associate,
 * build, rounds, finish, pushes and loop-mode graph pushes as there, time[k] in the place of odom[k].time and imu[k] in
 * the place of its IMU fields (imu NULL: no entry has IMU angles).  Results are bit for bit those of
 * lins_streams_map_step given the rows lins_streams_odometry returns.  An entry whose record is not valid gets status
 * LINS_E_INPUT for that entry alone, in front of the interval gate: nothing of its stream changes, and the others
 * proceed.  Non-finite time / imu values: LINS_E_INPUT for the whole call; the other refusals as
 * lins_streams_map_step.  This call and lins_streams_fuse: LINS_E_STATE when lins_streams_init has since been called
 * with fewer streams than lins_streams_map_init knows.                                                               */
int lins_streams_map_step_resident(lins_ctx* ctx, int n, const int32_t* streams, const double* time, const lins_slam_imu* imu,
                                   lins_map_step_result* out);

/* The transform fusion node for the n streams named (each in range; n <= n_streams of lins_streams_map_init, else
 * LINS_E_ARG): transformMapped = transformAssociateToMap (TF:91-215) of the resident transformBefMapped /
 * transformAftMapped and the resident record's transformSum, and the orientation laserOdometry2 carries (TF:235-242).
 * One kernel, one download.  It changes no state: call it any number of times between map steps.  The records are the
 * ones the last lins_streams_odometry / lins_streams_map_step_resident / lins_streams_slam_step left; LINS_E_STATE
 * before any of them — lins_streams_init, lins_streams_machine_init and lins_streams_map_init drop the records of an
 * earlier run — or before lins_streams_map_init, LINS_E_INPUT (nothing written) when a named stream's record is not
 * valid.  The node reads transformAftMapped back through the quaternion of /aft_mapped_to_init (TF:256-268); here
 * it is the resident one, a departure.                                                                               */
int lins_streams_fuse(lins_ctx* ctx, int n, const int32_t* streams, lins_fused_pose* out);

/* One scan of every stream, from the raw sweep and the IMU rows to the fused map pose.  Machine mode only
 * (lins_streams_machine_init) and after lins_streams_map_init over all the streams: LINS_E_STATE otherwise, nothing run.
 *   1. lins_streams_process_raw(raw, n_raw, n_imu, imu, scan_imu, scan_time, scan_period) -> results, status (both
 *      n_streams; status: each stream's state after the call)
 *   2. the records (lins_streams_odometry's kernel)
 *   3. lins_streams_map_step_resident for exactly the streams whose status is LINS_STREAM_RUNNING — the ones the
 *      reference publishes for: from the second scan on (EC:254-273 with SE:233) —, time = scan_time[k], imu_rp[k] (or
 *      NULL).  A gated running scan takes part with the clouds as they lie.  map[k] of the other streams: status
 *      LINS_MAP_STEP_SKIPPED, ring_age = archive_id = -1, zeros.
 *   4. the fusion (lins_streams_fuse's kernel) for those same streams -> fused[k]; zeros for the others and for a stream
 *      whose record is not valid.  It runs behind the map step: a stream whose entry the interval gate skipped is
 *      fused with its older transformBefMapped / transformAftMapped, as the node does between two mapping results.
 * Departures: a stream thrown back to INIT by its second scan, or held at LINS_E_UNSUPPORTED, publishes nothing, where
 * the reference publishes its stale clouds and pose again.  With lins_streams_map_loop on, the graph is fed as by
 * lins_streams_map_step; lins_loop_step (lins_map.h) runs beside it unchanged.  An error of step 1 returns before
 * anything of steps 2-4; an error of step 3 leaves the filter advanced (as the explicit calls would).               */
int lins_streams_slam_step(lins_ctx* ctx, const lins_point* const* raw, const int32_t* n_raw, const int32_t* n_imu,
                           const double* const* imu, const double* scan_imu, const double* scan_time, double scan_period,
                           const lins_slam_imu* imu_rp, lins_result* results, int32_t* status, lins_map_step_result* map,
                           lins_fused_pose* fused);

#ifdef __cplusplus
}
#endif
#endif
