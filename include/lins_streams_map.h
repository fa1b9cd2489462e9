/*
 * lins_streams_map.h — the outlier cloud on the device and the hand-over of a stream's clouds to the mapping node
 * (entry points of liblins_ieskf.so; the host restatement lins_frontend_segment_outliers and LINS_OUTLIER_MAX are in
 * lins_host.h, lins_local_map_build_streams in lins_map.h), and the mapping node's run() for streams: per-stream map
 * poses resident on the device, one call per scan (lins_streams_map_step).
 */
#ifndef LINS_STREAMS_MAP_H_
#define LINS_STREAMS_MAP_H_

#include "lins_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lins_segment_batch plus that cloud: outlier[k] is caller-allocated with LINS_OUTLIER_MAX entries and receives
 * out[k].n_outlier points, identical to lins_frontend_segment_outliers().  (lins_segment_batch runs the same kernel
 * without the emission.)                                                                                            */
int lins_segment_batch_outliers(lins_ctx* ctx, int n, const lins_point* const* raw, const int32_t* n_raw,
                                lins_segmented_scan* out, lins_point* const* outlier);

/* What the mapping node reads of a stream.  The raw-cloud steps (lins_streams_step_raw, lins_streams_step_imu_raw) keep
 * the outlier cloud (lins_frontend_segment_outliers) of the scan just taken in resident beside the feature clouds.  The
 * segmented-input steps have no outlier cloud in their input: lins_streams_put_outliers uploads one per stream
 * (n_outlier[k] <= LINS_OUTLIER_MAX points; outlier[k] may be null where n_outlier[k] is 0) for the NEXT step, which
 * consumes it; a segmented step without it leaves the stream's outlier cloud EMPTY.  A raw step ignores (and drops) a
 * pending upload.  A scan the feature gate stops (LINS_STREAMS_GATED) leaves all three clouds the last accepted scan's.
 * Clouds: finite, else LINS_E_INPUT.                                                                                  */
int lins_streams_put_outliers(lins_ctx* ctx, const lins_point* const* outlier, const int32_t* n_outlier);
/* The clouds StateEstimator::publishTopics would publish after the last step (SE:1125-1147), in the mapping node's axes
 * (x, y, z) <- (y, z, x), intensity kept: which = 0 the re-projected less-sharp cloud (laser_cloud_corner_last), 1 the
 * re-projected less-flat cloud (laser_cloud_surf_last), 2 the outlier cloud, NOT re-projected (outlier_cloud_last).
 * Returns the count; LINS_E_STATE before the stream's first step or on a failed streams context, LINS_E_CAPACITY when
 * cap is too small.  lins_local_map_build_streams (lins_map.h) reads the same clouds where they lie.                  */
int lins_streams_map_cloud(lins_ctx* ctx, int stream, int which, lins_point* out, int cap);

/* ---- the mapping node's run() for streams (LM:1821-1836): one call per scan ------------------------------------------
 * Each stream's map pose lives on the device: transformBefMapped, transformAftMapped, transformTobeMapped, transformLast
 * (rx, ry, rz, tx, ty, tz), previousRobotPosPoint and the number of key frames the stream has saved; timeLastProcessing
 * is kept beside it on the host.  Zero at init, last_time = -1, as allocateMemory leaves them (LM:305-409).  The
 * arithmetic is csrc/map_pose_math.h (host restatement: lins_host_map_* in lins_host.h).
 *
 * iSAM2 stays with the caller.  The step treats it as the identity, a departure from the node: the first key frame of a
 * stream takes transformTobeMapped (LM:1676-1686), every later one transformAftMapped (LM:1699-1704), and for every key
 * frame after the first transformLast = transformTobeMapped = transformAftMapped (LM:1737-1749).  GTSAM's RzRyRx /
 * pitch() / yaw() / roll() round trip of those six numbers is not imitated.  A caller with iSAM2 writes its estimate
 * back with lins_streams_map_set_pose (+ lins_local_map_set_pose, lins_archive_set_poses for the stored frames).     */
typedef struct lins_map_pose_state {
  float bef[6], aft[6], tobe[6], last[6], prev[3];
  int32_t n_frames;  /* cloudKeyPoses3D->points.size() of this stream */
  double last_time;  /* timeLastProcessing */
} lins_map_pose_state;

typedef struct lins_map_odom { /* laserOdometryHandler's and imuHandler's outputs for one scan of one stream */
  float transform_sum[6];      /* transformSum (LM:711-724) */
  float imu_roll, imu_pitch;   /* imuRollLast, imuPitchLast (LM:539-565); read with has_imu */
  int32_t has_imu;             /* imuPointerLast >= 0 */
  int32_t reserved;
  double time;                 /* timeLaserOdometry */
} lins_map_odom;

#define LINS_MAP_STEP_SKIPPED 1 /* lins_map_step_result.status: the interval gate of LM:1821 stopped the entry */

typedef struct lins_map_step_result {
  float tobe_start[6]; /* transformTobeMapped as transformAssociateToMap left it */
  float transform[6];  /* transformAftMapped after the step */
  float key_pose[6];   /* the pose the key frame was stored with (key_frame == 1), same order */
  int32_t iters, converged, degenerate, n_sel; /* as lins_map_result */
  int32_t status;      /* LINS_OK | LINS_MAP_STEP_SKIPPED | LINS_E_INPUT | LINS_E_CAPACITY (the build entry's status) */
  int32_t key_frame;   /* 1: the scan became a key frame of its stream's slot (and of the archive) */
  int32_t ring_age;    /* the age lins_local_map_set_pose addresses the stored frame by (0: the newest); -1: none stored */
  int32_t archive_id;  /* the id lins_archive_push_scans gave it; -1 without an archive or a key frame */
} lins_map_step_result;

/* map_associate_kernel on caller data: tobe6[6 k ..] = transformAssociateToMap of row k of bef6 / aft6 / sum6 (n x 6
 * floats each).  A row's result bits do not depend on n or on its position.  Non-finite input: LINS_E_INPUT.          */
int lins_map_associate_batch(lins_ctx* ctx, int n, const float* bef6, const float* aft6, const float* sum6, float* tobe6);
/* After lins_streams_init and lins_local_map_init with n_slots >= n_streams (else LINS_E_STATE); stream k uses slot k
 * of the local map, and of the archive if lins_archive_init has been called by then.  process_interval:
 * mappingProcessInterval, 0.3 (LM:1821); >= 0.  A second call starts every stream anew.                              */
int lins_streams_map_init(lins_ctx* ctx, int n_streams, double process_interval);
int lins_streams_map_get_pose(lins_ctx* ctx, int stream, lins_map_pose_state* out);
/* what a caller's iSAM2 writes back (LM:1737-1749), or a start pose; finite values, n_frames >= 0 (LINS_E_INPUT)      */
int lins_streams_map_set_pose(lins_ctx* ctx, int stream, const lins_map_pose_state* in);
/* run() for the n streams named (each at most once; n <= n_streams), in the order of LM:1821-1836:
 *   gate        odom[k].time - last_time >= process_interval (f64), else status LINS_MAP_STEP_SKIPPED, nothing changes;
 *               the other entries form the batch, last_time <- time
 *   associate   transformAssociateToMap on the device from the resident pose
 *   local map   lins_local_map_build_streams for the batch (entry <-> stream, slot = stream); with
 *               lins_streams_map_surround on, the surrounding key frames of the archive instead of the ring; with
 *               lins_streams_map_team on, the selected key frames of every slot of the stream's group
 *   scan2map    lins_scan2map_batch's rounds with LINS_MAP_LOCAL, started where the associate kernel left the transform
 *   finish      transformUpdate if the precondition of LM:1636 held, the key-frame rule, the key pose; one download
 *   key frames  lins_local_map_push_scans and lins_archive_push_scans for the entries with key_frame set, with
 *               lins_key_pose{t[3], t[4], t[5], t[0], t[1], t[2]} of key_pose and odom[k].time
 * A build entry with a status (LINS_E_INPUT / LINS_E_CAPACITY) reports it, keeps its pose state (last_time included) and
 * stores nothing; the others proceed.  Non-finite transform_sum / imu values / time: LINS_E_INPUT; a stream named twice,
 * a bad index, n > n_streams: LINS_E_ARG — for the whole call, before anything is queued.  LINS_E_STATE before
 * lins_streams_map_init.  The local map's build and the resident maps of lins_scan2map_batch are this call's afterwards,
 * as after the explicit calls.                                                                                       */
int lins_streams_map_step(lins_ctx* ctx, int n, const int32_t* streams, const lins_map_odom* odom, lins_map_step_result* out);
/* on != 0: every later step also makes saveKeyFramesAndFactor's factor (LM:1673-1705) for each key frame it stores —
 * lins_pose_graph_push(slot = stream, transformLast as the finish kernel found it, key_pose), the prior for a stream's
 * first frame — so that lins_loop_step (lins_map.h) finds graph and archive in step; the id the graph returns is the
 * step's archive_id (LINS_E_STATE otherwise; a graph without room for a key frame of the batch: LINS_E_CAPACITY before
 * anything is stored).  transformLast is read from a host mirror, kept in step with the finish kernel's rule,
 * lins_streams_map_set_pose and lins_pose_graph_apply / _apply_batch; switching on downloads it once.  After
 * lins_streams_map_init with an archive (lins_archive_init before it) and lins_pose_graph_init, the graph with at least
 * n_streams slots and every stream's graph and archive holding the same frame count: LINS_E_STATE otherwise.  Off — the
 * default, and again after lins_streams_map_init — the step does not touch a graph that happens to be initialised.
 * Either way the step remembers currentRobotPosPoint per stream: transform[3..5] of its last entry with status LINS_OK
 * (LM:1655-1658), which LINS_LOOP_CENTRE_STREAM reads.                                                                */
int lins_streams_map_loop(lins_ctx* ctx, int on);
/* on != 0: later steps build each entry's local map from the surrounding key frames — the mapping node with
 * loopClosureEnableFlag off (LM:1247-1315) — with radius (surroundingKeyframeSearchRadius, 50) and pose_leaf (1.0,
 * LM:288).  The "local map" stage of an entry then is: the archive of the stream's slot empty (LM:1202) -> the list is
 * empty; else ds = lins_archive_select_radius(slot, centre = the remembered currentRobotPosPoint (zero before the
 * stream's first completed step, as allocateMemory leaves it), radius, pose_leaf), and the stream's list
 * (surroundingExistingKeyPosesID) goes through lins_host_surround_update's rule; one
 * lins_local_map_build_surround_streams call serves the batch.  A selection whose box has more than 2^31 cells gives the
 * entry status LINS_E_CAPACITY: it is left out of the batch, list and pose state as they were.  A build entry with a
 * status keeps its list too.  Gate, associate, rounds, finish, the pushes to ring and archive and the result record are
 * unchanged: the ring keeps being fed, so switching the mode off continues with the recent-frame map.
 * One departure: the node keeps the transformed clouds of listed frames (surrounding*CloudKeyFrames); the step moves
 * them anew from the archive's current poses.  In this mode the node never rewrites a key pose, so the bits are the
 * same; after a caller's lins_archive_set_poses the next step uses the new poses.
 * Off by default and again after lins_streams_map_init; switching on clears every list.  Needs lins_streams_map_init with
 * an archive (LINS_E_STATE), and is exclusive with lins_streams_map_loop — the node's flag selects one of the two:
 * whichever is asked for second gets LINS_E_STATE.  radius finite and >= 0, pose_leaf > 0 (LINS_E_ARG).                  */
int lins_streams_map_surround(lins_ctx* ctx, int on, float radius, float pose_leaf);
/* the stream's surroundingExistingKeyPosesID as the last step left it; returns the count, LINS_E_CAPACITY beyond cap   */
int lins_streams_map_surround_list(lins_ctx* ctx, int stream, int32_t* ids, int cap);
/* ---- the team map: scan-to-map over the key frames of every robot met -------------------------------------------------
 * Slots whose maps share a frame are a group; the caller names the groups after lins_team_rebase (lins_team.h) has moved
 * one robot's history into the other's frame.  on != 0: the "local map" stage of every gated entry becomes
 *   targets    the slots of the stream's group (group -1, the default: the slot alone), as many as the archive holds
 *   centre     the remembered currentRobotPosPoint, as the surround mode takes it
 *   selection  the team selection's rule (lins_map.h lins_keyposes_team_select_batch: per pose cell of pose_leaf the
 *              nearest hit within radius, ties by (slot, id)) — one selection for the batch, the batched device call
 *              under LINS_KEYPOSES_DEVICE, the host text otherwise, the same bits either way
 *   build      one lins_local_map_build_team_streams over the selected (slot, id) pairs; sizes->frames is the list length
 * and everything else in the step is unchanged: gate, associate, rounds, finish, the pushes to ring, archive and pose
 * graph, the result record.  The project's own rule, not the node's (DESIGN.md §5.3 "Team map"): there is no list that
 * persists between steps — the selection is a pure function of the key poses and the centre — and listed frames are moved
 * anew from the archive's current poses every step, so a loop closure or a rebase shows in the next map.  A selection
 * whose box has more than 2^31 cells gives the entry status LINS_E_CAPACITY: it is left out of the batch, its state as it
 * was.  A slot of the group whose archive holds no frames (never fed, or released) contributes none.
 * Off by default and again after lins_streams_map_init.  Needs lins_streams_map_init with an archive (LINS_E_STATE).
 * Exclusive with lins_streams_map_surround (whichever is asked for second gets LINS_E_STATE); compatible with
 * lins_streams_map_loop — the graph must keep being fed, or there is nothing to rebase.  radius finite and >= 0,
 * pose_leaf > 0 with a finite inverse (LINS_E_ARG).  lins_streams_map_step_resident and lins_streams_slam_step share the
 * step's body and get the mode with it.  Mode and groups are context settings, like lins_keyposes_set_mode: they are not
 * in a snapshot's blob, and the caller repeats them on the destination (lins_snapshot.h). */
int lins_streams_map_team(lins_ctx* ctx, int on, float radius, float pose_leaf);
/* slots[k] joins group groups[k] (>= 0), or stands alone again (-1).  lins_streams_map_release, and so
 * lins_streams_retire, puts a released slot's group back to -1.  LINS_E_ARG for a slot that is no stream or a group < -1
 * (nothing changes); the mode need not be on. */
int lins_streams_map_team_groups(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* groups);
int lins_streams_map_team_group(lins_ctx* ctx, int slot, int32_t* group);
/* the (slot, id) pairs the stream's last completed team build listed (a record for the caller; an input to nothing);
 * returns the count of pairs, LINS_E_CAPACITY beyond cap */
int lins_streams_map_team_list(lins_ctx* ctx, int stream, int32_t* pairs, int cap);
/* HIP-event times (ms) of the associate and finish kernels of the last step (0 when the step queued none)            */
int lins_last_streams_map_ms(lins_ctx* ctx, float* associate_ms, float* finish_ms);

#ifdef __cplusplus
}
#endif
#endif
