/* lins_map.h — C ABI of the scan-to-map correspondence / optimisation row.
 *
 * Replaces, in the reference's mapping node (src/lidar_mapping_node.cpp, "LM"):
 *   cornerOptimization  LM:1351-1453   5-NN in the local corner map, 3x3 covariance eigen-fit,
 *                                      point-to-line coefficients
 *   surfOptimization    LM:1455-1521   5-NN in the local surf map, 5-point plane fit, point-to-plane
 *   LMOptimization      LM:1523-1633   6-DoF Gauss-Newton step on (rx, ry, rz, tx, ty, tz) with the
 *                                      degeneracy projection of iteration 0
 *   scan2MapOptimization LM:1635-1652  up to 10 rounds of the three
 * with pointAssociateToMap (LM:579-607).  All arithmetic is f32 as in the reference; its third-party
 * pieces (FLANN 5-NN, cv::eigen, cv::solve(DECOMP_QR), cv::Mat::inv) are restated with fixed
 * operation sequences — exact 5-NN ordered by (distance, index), cyclic-Jacobi eigen-decomposition,
 * Householder QR — see DESIGN.md; parity is against oracle/map_oracle.cpp (unpinned like the rest:
 * the reference cannot be built here).
 */
#ifndef LINS_MAP_H_
#define LINS_MAP_H_

#include "lins_ieskf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lins_map_problem {
  const lins_point* map_corner; /* laserCloudCornerFromMapDS */
  const lins_point* map_surf;   /* laserCloudSurfFromMapDS   */
  const lins_point* scan_corner; /* laserCloudCornerLastDS    */
  const lins_point* scan_surf;   /* laserCloudSurfTotalLastDS */
  int32_t n_map_corner, n_map_surf, n_scan_corner, n_scan_surf;
  float transform[6]; /* transformTobeMapped: rx, ry, rz, tx, ty, tz */
  int32_t reserved[2]; /* [0]: flags (LINS_MAP_REUSE or LINS_MAP_LOCAL), [1]: 0 */
} lins_map_problem;

/* reserved[0] flag: the two map clouds of this problem are the ones of the previous call at the same batch index
 * (the mapping node's local map only changes with its key frames): when EVERY problem of a batch says so and the
 * sizes match, the maps already resident on the device — uploaded and bucketed into 1 m cells by the last call —
 * are used as they are; map_corner / map_surf are not read.  "The previous call" is the last one that succeeded AND
 * no call failed since: a call that returns an error other than LINS_E_ARG / LINS_E_STATE leaves nothing resident, so
 * a LINS_MAP_REUSE call behind it uploads its own maps.                                                            */
#define LINS_MAP_REUSE 1
/* reserved[0] flag: problem k is entry k of the last lins_local_map_build — maps and queries are the clouds that call
 * built on the device (laserCloudCornerFromMapDS / SurfFromMapDS, laserCloudCornerLastDS / SurfTotalLastDS) and are
 * read where they lie; map_* / scan_* / n_* are not read.  Every problem of the batch carries it (else LINS_E_ARG), it
 * is not combined with LINS_MAP_REUSE (LINS_E_ARG), and the batch has the size of the last build (else LINS_E_STATE). */
#define LINS_MAP_LOCAL 2

/* one query of cornerOptimization / surfOptimization */
typedef struct lins_map_corr {
  int32_t ind[5];   /* the 5 nearest map points, ascending (distance, index); -1 when fewer than 5 lie within 1 m */
  int32_t accepted; /* row pushed to laserCloudOri / coeffSel (LM:1446-1449, 1514-1517) */
  float coeff[4];   /* (s la, s lb, s lc, s ld2) / (s pa, s pb, s pc, s pd2) */
  float sel[3];     /* pointSel = pointAssociateToMap(pointOri) */
  float sq5;        /* pointSearchSqDis[4] (inf when fewer than 5 within 1 m) */
} lins_map_corr;

typedef struct lins_map_result {
  float transform[6];
  int32_t iters;      /* rounds run (<= 10) */
  int32_t converged;  /* LMOptimization returned true (deltaR < 0.05 deg && deltaT < 0.05 cm) */
  int32_t degenerate; /* isDegenerate after round 0 */
  int32_t n_sel;      /* rows selected in the last round */
} lins_map_result;

/* Input contract of the two calls below.  Map points: finite, |coord| <= 1e6 (LINS_E_INPUT), at most 2^26 cells of
 * 1 m in a cloud's box (LINS_E_CAPACITY).  Scan points: finite (LINS_E_INPUT), of any magnitude.  transform: finite
 * (LINS_E_INPUT).  A call that fails this way changes no result, leaves no map resident and the context usable.  Where a query's
 * associated point lands is NOT part of the contract: far from the map, beyond the range of an int, or non-finite (the
 * transform of a later round is the optimisation's own), it has no fifth neighbour within 1 m and gets ind = -1,
 * accepted = 0, sq5 = inf — the device clamps the point to +-2^30 in float before it takes its cell, so the cell
 * arithmetic is defined for every float and the other queries of the batch are not affected.                      */
/* one correspondence pass at in->transform: n_scan_corner + n_scan_surf records */
int lins_map_correspondences(lins_ctx* ctx, const lins_map_problem* in, lins_map_corr* corner, lins_map_corr* surf);
/* scan2MapOptimization for n independent problems, entirely on the device: the maps are bucketed into 1 m cells by
 * a counting-sort kernel (or reused, LINS_MAP_REUSE), then the up to 10 rounds of {correspondence + row + reduction
 * kernel, 6x6 Gauss-Newton step kernel with the degeneracy projection} run back to back; the precondition of LM:1636
 * (> 10 corner and > 100 surf map points) not met => transform returned unchanged with iters = 0 */
int lins_scan2map_batch(lins_ctx* ctx, int n, const lins_map_problem* in, lins_map_result* out);
/* HIP-event time (ms) of the device sequence of the last call (the rounds' kernels; lins_map_correspondences: its
 * one pass) and the number of query evaluations it did */
int lins_last_map_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* queries);

/* ---- the mapping node's local map on the device (LM:1201-1349, 1752-1763) ------------------------------------------
 * Key frames live on the device in per-slot rings, in the sensor frame, with the trigonometry of their pose formed on
 * the host once (std::cos / std::sin of float, as updateTransformPointCloudSinCos does, LM:612-624).  A build moves the
 * last min(window, K) frames of a slot into the map frame (transformPointCloud, LM:627-650, f32 as written),
 * concatenates them oldest first — corner map: corner_i; surf map: surf_i then outlier_i — and VoxelGrid-filters them
 * (corner 0.2 m, surf 0.4 m, LM:1316-1323); it filters the raw scan as downsampleCurrentScan does (LM:1326-1349).
 * A departure from the reference: "the last min(window, K) frames, each once".  The node's deque holds those frames only
 * while every scan that finds it full brings a new key frame; latestFrameID starts at 0 and the rebuild branch never sets
 * it, so the first scan that finds 50 entries without a new key frame (also after correctPoses() cleared the deques) pops
 * the oldest frame and pushes the newest a second time (LM:1225-1239).  Both behaviours are asserted by
 * tests/test_ref_mapnode.py and tests/test_gpu_ref_mapnode.py (DESIGN.md §5.3 "The mapping node's local map").
 * VoxelGrid is the project's contract: f32 box, stable order by PCL's linear voxel index, centroid
 * = sequential f32 sums in input order / (float)count, output in ascending voxel order, no minimum count.           */
typedef struct lins_key_pose {
  float x, y, z, roll, pitch, yaw; /* PointTypePose (LM:1721-1732: t[3], t[4], t[5], t[0], t[1], t[2] of transformAftMapped) */
} lins_key_pose;

typedef struct lins_keyframe { /* one key frame: cornerCloudKeyFrames / surf / outlier (sensor frame) + its pose */
  const lins_point* corner;
  const lins_point* surf;
  const lins_point* outlier;
  int32_t n_corner, n_surf, n_outlier, reserved;
  lins_key_pose pose;
} lins_keyframe;

typedef struct lins_local_scan { /* laserCloudCornerLast, laserCloudSurfLast, laserCloudOutlierLast of one build entry */
  const lins_point* corner;
  const lins_point* surf;
  const lins_point* outlier;
  int32_t n_corner, n_surf, n_outlier, reserved;
} lins_local_scan;

/* the six clouds of a build entry */
#define LINS_LOCAL_MAP_CORNER 0   /* laserCloudCornerFromMapDS  = VG0.2(corner_i ...)               */
#define LINS_LOCAL_MAP_SURF 1     /* laserCloudSurfFromMapDS    = VG0.4(surf_i, outlier_i ...)      */
#define LINS_LOCAL_SCAN_CORNER 2  /* laserCloudCornerLastDS     = VG0.2(corner)                     */
#define LINS_LOCAL_SCAN_SURF 3    /* laserCloudSurfLastDS       = VG0.4(surf)                       */
#define LINS_LOCAL_SCAN_OUTLIER 4 /* laserCloudOutlierLastDS    = VG0.4(outlier)                    */
#define LINS_LOCAL_SCAN_TOTAL 5   /* laserCloudSurfTotalLastDS  = VG0.4(surfDS ++ outlierDS)        */

typedef struct lins_local_map_sizes {
  int32_t n[6];          /* points of the six clouds (LINS_LOCAL_* order)                                          */
  int32_t box_min[2][3]; /* the 1 m cell box scan-to-map grids the corner / surf map into (floor of the coordinates; */
  int32_t box_dim[2][3]; /* an empty map: min 0, dim 1)                                                             */
  int32_t frames;        /* key frames in the window                                                               */
  int32_t status;        /* LINS_OK; LINS_E_CAPACITY: a VoxelGrid box of more than 2^31 cells; LINS_E_INPUT: a map
                            point beyond |coord| <= 1e6 — the entry's clouds are then empty                        */
} lins_local_map_sizes;

/* n_slots rings of `window` key frames (surroundingKeyframeSearchNum = 50), each frame up to max_points_per_frame
 * points over its three clouds.  Sized once; a second call drops every ring and sizes anew. */
int lins_local_map_init(lins_ctx* ctx, int n_slots, int window, int max_points_per_frame);
/* saveKeyFramesAndFactor's cloud copies (LM:1752-1763): one key frame onto the ring of `slot`; a full ring drops its
 * oldest frame (LM:1226-1240).  Clouds: finite, |coord| <= 1e6 (LINS_E_INPUT); pose finite, |x|,|y|,|z| <= 1e6. */
int lins_local_map_push(lins_ctx* ctx, int slot, const lins_keyframe* frame);
/* extractSurroundingKeyFrames + downsampleCurrentScan for n entries: entry k uses the ring of slots[k] and filters
 * scans[k]; everything runs on the context's stream with one synchronisation at the end; out[k] (may be NULL) gets
 * the sizes, the 1 m boxes and the entry's status.  An empty ring gives empty maps.  Scans: finite, |coord| <= 1e6. */
int lins_local_map_build(lins_ctx* ctx, int n, const int32_t* slots, const lins_local_scan* scans, lins_local_map_sizes* out);
/* lins_local_map_build with entry k's three scan clouds taken from stream streams[k] of the context's device-resident
 * streams (lins_streams_map.h) where they lie: the clouds lins_streams_map_cloud would return — corner last, surf last, outlier
 * last — are moved into the mapping node's axes, checked and boxed by one kernel instead of on the host; nothing is
 * downloaded or uploaded.  Everything behind that, and every result bit, is lins_local_map_build's;
 * lins_local_map_push_scans, lins_archive_push_scans, lins_local_map_download and LINS_MAP_LOCAL work on this build as on
 * any other.  A stream may appear once (LINS_E_ARG); a stream that has not stepped, or a failed streams context:
 * LINS_E_STATE.  The input contract is checked on the device: an entry with a scan point that is not finite or beyond
 * 1e6 gets status LINS_E_INPUT and empty clouds (as a window cloud outside the contract), the call returns LINS_OK.   */
int lins_local_map_build_streams(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* streams, lins_local_map_sizes* out);
/* extractSurroundingKeyFrames with the loop closure off (LM:1247-1315): the build with its map side read from a list of
 * frames of the key-frame archive (below; slot slots[k] of it) instead of the ring.  Entry k's corner map is
 * VG0.2(corner of ids[k][0], corner of ids[k][1], ...), its surf map VG0.4(surf_i, outlier_i, ...) in list order
 * (LM:1310-1314), each frame moved by its archive pose — the clouds lins_archive_assemble gives for the specs
 * {ids, CORNER, leaf 0.2} and {ids, SURF | OUTLIER, leaf 0.4}, bit for bit.  The four scan clouds, sizes, boxes and
 * per-entry status are lins_local_map_build's / _build_streams'; sizes.frames = n_ids[k]; n_ids[k] == 0 gives empty
 * maps, as an empty ring does.  The ring is neither read nor changed, and lins_local_map_download, LINS_MAP_LOCAL,
 * lins_local_map_push_scans and lins_archive_push_scans work on this build as on any other.  A map job of more tiles than
 * the archive's scan chunk has its scans split over workgroups as in an assembly (lins_archive_set_scan_chunk applies).
 * LINS_E_STATE without lins_local_map_init or lins_archive_init; LINS_E_ARG for a slot that is not one of both, or an id
 * that is no frame of its slot; a refused call changes nothing.  Which frames to list is the caller's rule —
 * lins_archive_select_radius and lins_host_surround_update (lins_host.h), or lins_streams_map_surround. */
int lins_local_map_build_surround(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* const* ids, const int32_t* n_ids,
                                  const lins_local_scan* scans, lins_local_map_sizes* out);
int lins_local_map_build_surround_streams(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* const* ids, const int32_t* n_ids,
                                          const int32_t* streams, lins_local_map_sizes* out);
/* The team map: lins_local_map_build_surround / _surround_streams with each list entry naming its own archive slot.
 * Entry k's list is the n_pairs[k] (slot, id) pairs at pairs[k] (2 * n_pairs[k] ints) — lins_keyposes_team_select_batch's
 * output, or any list; slots[k] stays the slot whose scan clouds and resident build the entry is.  The frames are moved
 * with their archive's current poses, so the slots listed must share a map frame (lins_team_rebase).  The same job table
 * and launches as the surround build: the bits are those of a surround build over one slot holding the same frames in
 * list order.  Refusals as the surround build's, plus LINS_E_ARG for a pair whose slot or id does not exist; a refused
 * call changes nothing. */
int lins_local_map_build_team(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* const* pairs, const int32_t* n_pairs,
                              const lins_local_scan* scans, lins_local_map_sizes* out);
int lins_local_map_build_team_streams(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* const* pairs, const int32_t* n_pairs,
                                      const int32_t* streams, lins_local_map_sizes* out);
/* HIP-event time (ms) of the staging kernel of the last lins_local_map_build_streams (part of the build's kernel_ms;
 * 0 after lins_local_map_build) */
int lins_last_local_map_stage_ms(lins_ctx* ctx, float* stage_ms);
/* the cornerDS, surfDS and outlierDS of the chosen entries of the last build become new key frames of their slots,
 * device to device, in the order given (the caller's key-frame rule, LM:1655-1669, decides which) */
int lins_local_map_push_scans(lins_ctx* ctx, int n, const int32_t* entries, const lins_key_pose* poses);
/* correctPoses (LM:1767-1795): the pose of the frame `age` frames before the newest (0: the newest) of `slot` */
int lins_local_map_set_pose(lins_ctx* ctx, int slot, int age, const lins_key_pose* pose);
/* cloud `which` (LINS_LOCAL_*) of entry `entry` of the last build; returns the point count (>= 0), LINS_E_CAPACITY
 * when it is larger than cap */
int lins_local_map_download(lins_ctx* ctx, int entry, int which, lins_point* out, int cap);
/* HIP-event time (ms) of the device sequence of the last build and the points it read (window frames + raw scans) */
int lins_last_local_map_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* points_in);

/* ---- the key-frame archive: global map and loop-closure submaps (LM:984-1031, 1043-1112, 1767-1795) ------------------
 * Every key frame of a slot stays on the device, in the sensor frame, in one bump-allocated point arena per context
 * (nothing is ever deleted); the host keeps per frame its offset, counts, pose, the pose's trigonometry as the local
 * map forms it, and a time.  Frame ids are 0, 1, 2 ... per slot in push order — the index cloudKeyPoses3D carries in
 * `intensity`.  The archive is independent of the local map's rings: a caller that wants both pushes to both.
 *
 * An assembly moves the chosen clouds of the chosen frames into the map frame (the two-argument transformPointCloud,
 * LM:654-686: the same f32 sequence as LM:627-650, and its cos / sin act on the same float members of PointTypePose in
 * the same translation unit as updateTransformPointCloudSinCos, so they are the same overloads — forming the six values
 * once per frame on the host is value-identical), concatenates them in the order given — within a frame always corner,
 * surf, outlier — and either VoxelGrid-filters the result (leaf > 0; DESIGN.md §5.3's contract, as the local map) or
 * hands it out as it is (leaf == 0), optionally without the points of (int)intensity < 0.  That predicate is C's cast as
 * x86 evaluates it for EVERY float: kept are exactly -1 < intensity < 2^31 (-0.5 is kept, -1.0 dropped; NaN, +-inf and
 * anything the cast cannot represent give INT_MIN there and are dropped), so intensity needs no input contract.
 *
 * The reference's three clouds are compositions (H = historyKeyframeSearchNum = 25, latest = count - 1):
 *   globalMapKeyFramesDS            ids = select_radius(centre, 500, 1.0)   clouds = corner | surf | outlier  leaf 0.4
 *   nearHistorySurfKeyFrameCloudDS  ids = max(0, closest - H) .. min(latest, closest + H)   corner | surf     leaf 0.4
 *   latestSurfKeyFrameCloud         ids = { latest }                        corner | surf   leaf 0, DROP_NEGATIVE      */
#define LINS_SUBMAP_CORNER 1
#define LINS_SUBMAP_SURF 2
#define LINS_SUBMAP_OUTLIER 4
#define LINS_SUBMAP_DROP_NEGATIVE 1 /* flags: drop (int)intensity < 0, order kept; only with leaf == 0 (else LINS_E_ARG) */

typedef struct lins_submap_spec {
  const int32_t* ids; /* frames of `slot`, concatenated in this order (an id may repeat) */
  int32_t n_ids;
  int32_t slot;
  int32_t clouds;     /* mask of LINS_SUBMAP_CORNER | _SURF | _OUTLIER, at least one */
  int32_t flags;      /* 0 or LINS_SUBMAP_DROP_NEGATIVE */
  float leaf;         /* 0: the bare concatenation; > 0: VoxelGrid of this leaf */
  int32_t reserved;
} lins_submap_spec;

typedef struct lins_submap_info {
  int32_t n;          /* points of the assembled cloud */
  int32_t frames;     /* n_ids */
  uint64_t points_in; /* points read from the archive */
  int32_t box_min[3]; /* the 1 m cell box of a filtered (leaf > 0) output, as lins_local_map_sizes has it; */
  int32_t box_dim[3]; /* an empty or unfiltered cloud: min 0, dim 1 */
  int32_t status;     /* LINS_OK; LINS_E_CAPACITY: a VoxelGrid box of more than 2^31 cells; LINS_E_INPUT: a
                         transformed point beyond |coord| <= 1e6 — the cloud is then empty */
  int32_t reserved;
} lins_submap_info;

/* Errors of every call below: LINS_E_STATE before lins_archive_init, LINS_E_ARG for a bad slot / id / mask / flag,
 * LINS_E_CAPACITY when the arena or a slot's frame list is full.  A refused call changes nothing.                */
/* n_slots frame lists of up to max_frames_per_slot frames over one arena of max_points_total points.  Sized once; a
 * second call drops every frame and sizes anew. */
int lins_archive_init(lins_ctx* ctx, int n_slots, int max_frames_per_slot, long long max_points_total);
/* one key frame behind the frames of `slot`; returns its id (>= 0) or an error.  Input contract of lins_local_map_push. */
int lins_archive_push(lins_ctx* ctx, int slot, const lins_keyframe* frame, double time);
/* cornerDS / surfDS / outlierDS of entries of the last lins_local_map_build become frames of their slots, device to
 * device, in the order given (as lins_local_map_push_scans); ids_out (may be NULL) gets the new ids */
int lins_archive_push_scans(lins_ctx* ctx, int n, const int32_t* entries, const lins_key_pose* poses, const double* times, int32_t* ids_out);
/* correctPoses over the whole history: frames first_id .. first_id + n - 1 of slot */
int lins_archive_set_poses(lins_ctx* ctx, int slot, int first_id, int n, const lins_key_pose* poses);
/* frames of slot (>= 0) */
int lins_archive_count(lins_ctx* ctx, int slot);
/* publishGlobalMap's choice of frames (LM:989-1007): radius search around centre, VoxelGrid(pose_leaf) of the hits as
 * points (x, y, z, (float)id), frame = (int) of each voxel's averaged intensity, in ascending voxel order (the
 * selection's contract: DESIGN.md §5.3, csrc/host/keyframe_select.h).  Returns the count; LINS_E_CAPACITY beyond cap. */
int lins_archive_select_radius(lins_ctx* ctx, int slot, const float centre[3], float radius, float pose_leaf, int32_t* ids, int cap);
/* detectLoopClosure's candidate (LM:1050-1067): the first hit of the radius search with |time - now| > min_gap_s;
 * *closest = its id or -1 */
int lins_archive_find_loop(lins_ctx* ctx, int slot, const float centre[3], float radius, double now, double min_gap_s, int32_t* closest);
/* n assemblies in one sequence of launches on the context's stream with one synchronisation; out[k] (may be NULL) */
int lins_archive_assemble(lins_ctx* ctx, int n, const lins_submap_spec* specs, lins_submap_info* out);
/* the cloud of entry `entry` of the last assembly; returns the point count, LINS_E_CAPACITY when larger than cap */
int lins_archive_download(lins_ctx* ctx, int entry, lins_point* out, int cap);
/* HIP-event time (ms) of the device sequence of the last assembly and the points it read */
int lins_last_archive_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* points_in);
/* test hook: the scans over a job's (256 digits x tiles) histogram and over its per-tile counts run in one workgroup
 * for a job of at most chunk_tiles tiles (of 512 points) and are split into chunks of chunk_tiles tiles over many
 * workgroups above it.  0: the default; INT_MAX: never split.  Results are the same bits for every value. */
int lins_archive_set_scan_chunk(lins_ctx* ctx, int chunk_tiles);

/* ---- key-pose selection on the device: lins_archive_select_radius / _find_loop / the surround list rule, batched ---------
 * The archive keeps a device mirror of every slot's key poses (x, y, z) and times; lins_archive_push, _push_scans and
 * _set_poses only note on the host from which id a slot's mirror is stale, and each call below brings the stale ranges of
 * the slots it names up in its one upload.  A call is one upload, one chain of launches on the context's stream (one
 * workgroup per entry), one download and one synchronisation.  The results are those of the single calls — the contract
 * of csrc/host/keyframe_select.h — bit for bit, for every entry, whatever the batch; a slot may appear in several entries.
 * An entry with more than 8 192 hits (or, in the surround call, a selected id that is no frame of the slot) is served by
 * that host text inside the same call: result.host = 1, counted in lins_last_keyposes_stats, not an error.
 * Errors: LINS_E_STATE before lins_archive_init; for the whole call, before anything is queued, LINS_E_ARG for what the
 * single calls refuse so (a bad slot, a centre or radius that is not finite, radius < 0, pose_leaf) and for a bad stride
 * or list, LINS_E_INPUT for a now that is not finite or a min_gap_s that is NaN; n = 0 is LINS_OK. */
typedef struct lins_keyposes_query {
  int32_t slot;
  float centre[3];
  float radius;    /* finite, >= 0 */
  float pose_leaf; /* > 0, 1 / pose_leaf finite (not read by lins_keyposes_find_loop_batch) */
} lins_keyposes_query;

typedef struct lins_keyposes_loop_query {
  lins_keyposes_query q;
  double now;       /* timeLaserOdometry */
  double min_gap_s; /* not NaN */
} lins_keyposes_loop_query;

typedef struct lins_keyposes_result {
  int32_t n;      /* frames selected (0 with a status) */
  int32_t hits;   /* poses within the radius */
  int32_t status; /* LINS_OK; LINS_E_CAPACITY: the hits' pose_leaf box has more than 2^31 cells, or the entry's output is
                     longer than stride — nothing is written for the entry */
  int32_t host;   /* 1: the host text served the entry */
} lins_keyposes_result;

/* lins_archive_select_radius for n entries: entry k's ids go to ids + k * stride (stride >= 0) */
int lins_keyposes_select_batch(lins_ctx* ctx, int n, const lins_keyposes_query* queries, int32_t* ids, int stride, lins_keyposes_result* results);
/* lins_archive_find_loop for n entries: closest[k] = the id or -1 */
int lins_keyposes_find_loop_batch(lins_ctx* ctx, int n, const lins_keyposes_loop_query* queries, int32_t* closest);
/* the selection and surroundingExistingKeyPosesID's rule (lins_host_surround_update) in one call: entry k's list is the
 * n_list[k] <= stride ids at lists + k * stride, every one a frame of its slot (else LINS_E_ARG); afterwards it holds the
 * updated list and n_list[k] its length.  An entry with a status keeps its list and length. */
int lins_keyposes_surround_batch(lins_ctx* ctx, int n, const lins_keyposes_query* queries, int32_t* lists, int stride, int32_t* n_list,
                                 lins_keyposes_result* results);
/* who selects for lins_streams_map_step in surround mode and for lins_loop_step's detect stage: the host loops (the
 * default after lins_create, and the definition) or the batched calls above.  The results are the same bits. */
#define LINS_KEYPOSES_HOST 0
#define LINS_KEYPOSES_DEVICE 1
int lins_keyposes_set_mode(lins_ctx* ctx, int mode);
int lins_keyposes_mode(lins_ctx* ctx); /* LINS_KEYPOSES_* (>= 0) */
/* of the last batched call: HIP-event time (ms) of its device sequence, the entries the host served, the hits over all
 * entries (0 after lins_keyposes_find_loop_batch, which counts none) */
int lins_last_keyposes_stats(lins_ctx* ctx, float* device_ms, int32_t* host_entries, uint64_t* hits);

/* ---- the team selection: the key frames of SEVERAL slots around a centre, for a merged local map ---------------------------
 * Slots whose maps share a frame (after lins_team_rebase, lins_team.h) are a team.  The node's rule cannot be carried
 * over one: it keeps the truncated mean id of each pose voxel, and a mean of ids of two robots names nothing.  The team
 * rule is the project's own (csrc/host/team_select.h, the one text both libraries compile; DESIGN.md §5.3 "Team map"):
 *   candidates  every frame of every target slot (a slot without frames is allowed; a slot named twice is LINS_E_ARG)
 *   hit         d = (dx dx + dy dy) + dz dz <= radius * radius in f32, uncontracted
 *   cell        floor(coord * (1 / pose_leaf)) per axis; the box of the hits' cells follows VoxelGrid's 2^31-cell rule
 *               (beyond it: per-entry LINS_E_CAPACITY, nothing selected)
 *   thinning    in every occupied cell exactly one hit survives, the one of smallest (d, slot, id)
 *   output      the survivors as (slot, id) pairs in ascending (slot, id); more than stride: per-entry LINS_E_CAPACITY
 * A total order decides, so the answer depends neither on the order of the target list nor on the batch, and there is no
 * list that persists between calls.  Conventions as the calls above (one upload with the stale mirror ranges of every
 * slot named, one chain of launches, one download, one synchronisation; every refusal before anything is queued; n = 0
 * is LINS_OK).  One workgroup serves one entry with a table of the occupied cells in LDS: the number of hits is not
 * bounded, the number of OCCUPIED CELLS is — an entry with more than LINS_KEYPOSES_TEAM_CELLS of them is served by the
 * host text inside the call (result.host = 1, counted in lins_last_keyposes_team_stats, the same bits). */
#define LINS_KEYPOSES_TEAM_CELLS 4096
typedef struct lins_keyposes_team_query {
  float centre[3];
  float radius;         /* finite, >= 0 */
  float pose_leaf;      /* > 0, 1 / pose_leaf finite */
  int32_t n_targets;    /* >= 0 */
  int32_t first_target; /* the entry's targets are targets[first_target .. first_target + n_targets) of the call's table */
  int32_t reserved;
} lins_keyposes_team_query;
/* targets: the call's table of n_table slot numbers the queries point into (entries may share a range).  Entry k's
 * survivors go to pairs + 2 * k * stride as (slot, id), results[k].n of them; results as lins_keyposes_select_batch. */
int lins_keyposes_team_select_batch(lins_ctx* ctx, int n, const lins_keyposes_team_query* queries, const int32_t* targets, int n_table,
                                    int32_t* pairs, int stride, lins_keyposes_result* results);
/* of the last team selection: HIP-event time (ms), the entries the host served, the hits over all entries */
int lins_last_keyposes_team_stats(lins_ctx* ctx, float* device_ms, int32_t* host_entries, uint64_t* hits);

/* ---- loop-closure alignment: ICP over the archive's submaps (performLoopClosure, LM:1114-1186) ----------------------
 * pcl::IterativeClosestPoint as the mapping node sets it up (LM:1128-1132), restated with a fixed operation sequence:
 * the project's contract ("Loop-closure ICP"), one scalar definition in csrc/loop_icp_math.h compiled
 * into both libraries.  Source S (ns points), target G (ng points, index = position in the cloud as
 * lins_archive_download returns it).  T_0 = identity (row-major 4 x 4, f64), mse_prev = DBL_MAX.  Round k:
 *   1 move       M = T_k rounded entry by entry to f32; x' = ((m00 x + m01 y) + m02 z) + m03 (f32, uncontracted; y', z'
 *                alike), from the ORIGINAL source point every round
 *   2 correspond the target of smallest (d, index), d = (dx dx + dy dy) + dz dz in f32; it counts iff
 *                d <= max_corr_dist * max_corr_dist (f32).  Exact: the exhaustive search's answer, ties by index
 *   3 too few    fewer than min_correspondences: stop, converged = 0, LINS_ICP_NO_CORRESPONDENCES, T kept
 *   4 fit        Kabsch in f64 from the sums n, S x', S g, S x' g^T (tiles of 32 source points: the tree
 *                ((q0+q4)+(q2+q6))+((q1+q5)+(q3+q7)) over each 8 consecutive points, the four eights in order, the tiles
 *                in order); 3 x 3 SVD by one-sided cyclic Jacobi, fixed sweep count; R = V diag(1, 1, det(V U^T)) U^T, a
 *                proper rotation also where the unconstrained optimum is a reflection, defined for a rank-2 H (planar
 *                points); an H of rank < 2 — sigma2 <= 2^14 x 2^-53 sigma1: collinear or coincident points, whose
 *                second singular value is the rounding noise of the raw moments — gives R = I, t = mu_g - mu_s
 *   5 compose    T_{k+1} = Delta T_k in f64
 *   6 stop       (a) k + 1 >= max_iterations  (b) 0.5 (trace R_Delta - 1) >= rotation_threshold and |t_Delta|^2 <=
 *                transformation_epsilon  (c) |mse - mse_prev| < fitness_epsilon  (d) |mse - mse_prev| / mse_prev < rel_mse;
 *                the first that holds stops (converged = 1); then mse_prev = mse.  mse: f64 mean of the counted d
 * After the loop one more pass of 1-2 at the final T without the distance cap: fitness = f64 mean of d over the source
 * points that found a target (n_fitness of them; DBL_MAX when none).  The caller applies converged && fitness <= 0.3
 * (LM:1140-1141).  */
#define LINS_ICP_NONE 0               /* still running (only seen with lins_debug_loop_icp_rounds) */
#define LINS_ICP_ITERATIONS 1
#define LINS_ICP_TRANSFORM 2
#define LINS_ICP_ABS_MSE 3
#define LINS_ICP_REL_MSE 4
#define LINS_ICP_NO_CORRESPONDENCES 5

typedef struct lins_loop_icp_params {
  double transformation_epsilon; /* 1e-6 (LM:1130) */
  double fitness_epsilon;        /* 1e-6 (LM:1131) */
  double rel_mse;                /* 1e-5: DefaultConvergenceCriteria's relative bound */
  double rotation_threshold;     /* 0.99999 */
  float max_corr_dist;           /* 100 (LM:1128) */
  int32_t max_iterations;        /* 100 (LM:1129) */
  int32_t min_correspondences;   /* 3 */
  int32_t reserved;
} lins_loop_icp_params;
void lins_loop_icp_default_params(lins_loop_icp_params* p);

typedef struct lins_loop_icp_problem { /* clouds: entries of the LAST lins_archive_assemble, read where they lie ... */
  int32_t source_entry, target_entry;  /* ... or -1: the host clouds below are uploaded */
  const lins_point* source;
  const lins_point* target;
  int32_t n_source, n_target;
} lins_loop_icp_problem;

typedef struct lins_loop_icp_result {
  double transform[16]; /* T, row-major */
  double fitness;       /* the fitness score (DBL_MAX: no source point found a target) */
  double mse;           /* the last round's mse */
  int32_t iterations, converged, reason, n_corr, n_fitness;
  uint32_t far_searches; /* queries, over every round and the fitness pass, that were finished by the whole-target scan */
  int32_t status;        /* LINS_OK; LINS_E_CAPACITY: a target box of more than 2^26 one-metre cells (nothing was run) */
  int32_t reserved;
} lins_loop_icp_result;

/* Input contract: host clouds finite, |coord| <= 1e6 (LINS_E_INPUT: nothing is run, the context stays usable).  Entry
 * problems: LINS_E_STATE without a prior assembly, LINS_E_ARG for a bad entry; an entry whose assembly failed (its
 * status) is an empty cloud.  An empty source or target gives LINS_ICP_NO_CORRESPONDENCES at iteration 0.  A problem's
 * result bits do not depend on the batch it is in.
 * Device sequence: every target is gridded once into 1 m cells; per round one search + sums kernel and one step kernel
 * (one wave per problem: sums in tile order, fit, compose, stop rule, the next round's M), queued back to back in
 * groups with one word "problems still running" read between the groups; then the fitness pass. */
int lins_loop_icp_batch(lins_ctx* ctx, int n, const lins_loop_icp_problem* in, const lins_loop_icp_params* prm, lins_loop_icp_result* out);
/* one pass of steps 1-2 at a given T (cap as max_corr_dist; cap <= 0: none): index (-1: none) and d per source point */
int lins_loop_icp_correspondences(lins_ctx* ctx, const lins_loop_icp_problem* in, const double T[16], float cap, int32_t* idx, float* sqdist);
/* HIP-event time (ms) of the device sequence of the last of the two calls above (gridding excluded) and the query
 * evaluations it did */
int lins_last_loop_icp_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* searches);

/* ---- the pose graph: loop closures correct the key-frame history (LM:1167-1183, 1673-1749, 1767-1795) -----------------
 * The factor graph the mapping node hands to iSAM2, per slot, resident on the device, and a batched Levenberg-Marquardt
 * solve of it.  The contract is the project's own (DESIGN.md §5.3 "Pose graph"; one scalar definition in
 * csrc/pose_graph_math.h and one text of the solve in csrc/pose_graph.h, compiled into both libraries):
 *   poses     T = (R, t) in f64 in the axes GTSAM sees.  Six floats p (pitch, yaw, roll, y, z, x — transformTobeMapped's
 *             order) give R = Rz(p[1]) Ry(p[0]) Rx(p[2]), t = (p[5], p[3], p[4]), the floats promoted to double before
 *             sin / cos.  Back: x = atan2(R21, R22), y = asin(-R20), z = atan2(R10, R00), translation as is, rounded once
 *             to f32; |y| at pi / 2 is outside the contract.
 *   factors   prior T_0 = Z_p (the first push's aft6) and odometry factor i = 1 .. N - 1 on (T_{i-1}, T_i) with
 *             Z_i = pose(last)^-1 pose(aft), formed once in f64 at the push; both with the variances (1e-6, 1e-6, 1e-6,
 *             1e-8, 1e-8, 1e-6), rotation first (LM:383-385).  Loop l on (T_b, T_a) = (latest, closest) with
 *             Z_l = pose_from^-1 T_a, T_a the estimate when the loop is added, and the variance (double)(float)fitness on
 *             all six components (LM:1171-1175).
 *   residual  of a between-factor Z on (T_i, T_j): E = Z^-1 T_i^-1 T_j, r = (Log_SO3(R_E), t_E) — the chart form, no
 *             SE(3) V^-1 on the translation; the retraction is (R Exp(omega), t + R v).  Cost C = 1/2 sum r^T Sigma^-1 r.
 *   solve     a graph without loops is returned with the bits it holds, 0 iterations: iSAM2 as the identity.  With loops:
 *             Levenberg-Marquardt on C over the increments T_{k-1}^-1 T_k (T_0 = Z_p exactly: the prior is satisfied, not
 *             weighed), one trial an iteration — step from the damped normal equations through the 6 L x 6 L Woodbury
 *             core, trial cost C'.  The first that holds ends the trial: |C - C'| <= rel_cost_decrease C — the cost
 *             does not tell the trial from the estimate; this last step is taken and the solve stops (LINS_PG_REL_COST);
 *             C' < C — the step is accepted, lambda is multiplied by lambda_down, and the solve stops if the step's
 *             largest component is <= max_increment (LINS_PG_INCREMENT); else the step is rejected and lambda multiplied
 *             by lambda_up.  iterations >= max_iterations stops it too (LINS_PG_ITERATIONS).
 *   poses     T_k = T_0 D_1 ... D_k is formed in blocks of 32 consecutive increments, left to right inside a block, the
 *             block totals left to right, T_k = (prefix of blocks) (prefix inside the block).
 * Departures from the reference: a converged batch optimum instead of iSAM2's incremental estimate (these parameters
 * replace relinearizeThreshold = 0.01, LM:249); GTSAM's chart flag is fixed as above; the prior is satisfied exactly; a
 * pushed frame's increment starts at its measurement Z_i (the reference inserts pose(aft), the same pose when `last` is
 * the previous frame's estimate).                                                                                     */
#define LINS_PG_NONE 0       /* not run (no loops), or still running */
#define LINS_PG_ITERATIONS 1
#define LINS_PG_INCREMENT 2
#define LINS_PG_REL_COST 3

typedef struct lins_pose_graph_params {
  int32_t max_iterations;    /* 50 */
  int32_t reserved;
  double rel_cost_decrease;  /* 1e-12 */
  double max_increment;      /* 1e-11 (rad or m) */
  double lambda_initial;     /* 1e-5 */
  double lambda_up;          /* 10 */
  double lambda_down;        /* 0.1 */
} lins_pose_graph_params;
void lins_pose_graph_default_params(lins_pose_graph_params* p);

typedef struct lins_pose_graph_result {
  double cost_before, cost_after; /* C at the first and at the last accepted estimate (0 for a graph without loops) */
  double max_increment;           /* the largest step component of the last trial */
  int32_t iterations, reason;     /* trials run; LINS_PG_* */
  int32_t status, reserved;       /* LINS_OK */
} lins_pose_graph_result;

/* Errors of every call below: LINS_E_STATE before lins_pose_graph_init, LINS_E_ARG for a bad slot / id or latest_id ==
 * closest_id, LINS_E_CAPACITY for a frame or loop beyond the sizes given at init, LINS_E_INPUT for non-finite input or a
 * loop variance that is not finite and > 0.  A refused call changes nothing.                                            */
/* n_slots graphs of up to max_frames_per_slot frames and max_loops_per_slot <= 64 loops (else LINS_E_ARG).  A second call
 * drops every graph and sizes anew.  Device memory: 1 248 bytes a frame and slot, 288 L^2 + 640 L bytes a slot for L
 * loops.  The loops' core is dense — a trial runs 3 L (L + 1) / 2 + 24 L barrier-separated phases on it — so the solve
 * suits the tens of loops a slot the reference closes, not hundreds. */
int lins_pose_graph_init(lins_ctx* ctx, int n_slots, int max_frames_per_slot, int max_loops_per_slot);
/* saveKeyFramesAndFactor's factor (LM:1673-1705): one frame behind the frames of `slot`; the first frame takes aft6 as
 * the prior (the caller passes transformTobeMapped, LM:1676; last6 is not read), every other the odometry factor
 * pose(last6)^-1 pose(aft6).  Returns the frame id — the archive's, when the caller pushes to both. */
int lins_pose_graph_push(lins_ctx* ctx, int slot, const float last6[6], const float aft6[6]);
/* performLoopClosure's factor (LM:1167-1181): pose_from as lins_host_loop_pose_from returns it, fitness the ICP's */
int lins_pose_graph_add_loop(lins_ctx* ctx, int slot, int latest_id, int closest_id, const lins_key_pose* pose_from, double fitness);
/* the solve for n slots (each at most once, else LINS_E_ARG) in one sequence of launches on the context's stream: one
 * workgroup per slot problem, the trials queued in groups with one word "problems still running" read between the
 * groups.  A problem's result bits do not depend on the batch it is in or on what the context ran before.  Parameters
 * outside max_iterations >= 1, finite bounds, lambda_initial > 0, lambda_up > 1, 0 < lambda_down <= 1: LINS_E_ARG. */
int lins_pose_graph_solve(lins_ctx* ctx, int n, const int32_t* slots, const lins_pose_graph_params* prm, lins_pose_graph_result* out);
/* the estimate of frames first_id .. first_id + n - 1 as PointTypePose, the fields as LM:1721-1733 assigns them */
int lins_pose_graph_poses(lins_ctx* ctx, int slot, int first_id, int n, lins_key_pose* out);
/* correctPoses (LM:1767-1795) and LM:1737-1749 in one call: every pose of `slot` goes to lins_archive_set_poses when the
 * archive is initialised (LINS_E_ARG when it holds fewer frames of the slot), the poses of the newest frames go to the
 * local map's ring by age when the local map is initialised — the ring's frames are taken to be the graph's newest;
 * LINS_E_ARG when it holds fewer than min(window, N) — and for stream >= 0 aft = last = tobe = the newest pose through
 * lins_streams_map_set_pose. */
int lins_pose_graph_apply(lins_ctx* ctx, int slot, int stream);
/* What n calls lins_pose_graph_apply(slots[k], streams[k]) do, with every refusal asked first — a refused call changes
 * nothing for any slot — and the streams' records written by ONE kernel (map_pose_correct_kernel: aft = last = tobe = the
 * newest pose; bef, prev and n_frames stay) behind one upload, with one synchronisation.  streams[k] = -1: no stream.  A
 * slot or a stream (>= 0) named twice: LINS_E_ARG. */
int lins_pose_graph_apply_batch(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* streams);
/* frames / loops of slot (>= 0) */
int lins_pose_graph_count(lins_ctx* ctx, int slot, int32_t* n_loops);
/* HIP-event time (ms) of the device sequence of the last solve and the trials it ran over all problems */
int lins_last_pose_graph_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* iterations);
/* test aids: the estimate in f64 (n x 12: R row-major, t) and loop l's measurement */
int lins_debug_pose_graph_poses_f64(lins_ctx* ctx, int slot, int first_id, int n, double* out);
int lins_debug_pose_graph_loop_z(lins_ctx* ctx, int slot, int loop, double z[12]);

/* ---- the loop thread's step: performLoopClosure + correctPoses for n slots in one call (LM:1033-1186, 1767-1795) --------
 * One call does, for every entry, what the chain lins_archive_find_loop -> lins_archive_assemble -> lins_loop_icp_batch ->
 * lins_pose_graph_poses + lins_host_loop_pose_from -> lins_pose_graph_add_loop -> lins_pose_graph_solve ->
 * lins_pose_graph_apply does for its slot, with the assembly, the alignment, the solve and the write-back each ONE batched
 * call over the entries that reach it.  An entry's result bits, and the state it leaves in the graph, the archive, the
 * ring and the map pose, are those of that chain: they do not depend on the batch, on its order, or on what the context
 * ran before.  What is decided between the stages is csrc/host/loop_step.h (lins_host_loop_* in lins_host.h); its two
 * departures from the reference — a frame is no loop with itself; a pair equal to the slot's most recent loop factor is a
 * repeat — are stated in DESIGN.md §5.3 "Loop thread's step". */
typedef struct lins_loop_step_params { /* lins_loop_step_default_params: the reference's values */
  float search_radius;  /* 5  (historyKeyframeSearchRadius, parameters.h:98) */
  float max_fitness;    /* 0.3 (historyKeyframeFitnessScore) */
  float history_leaf;   /* 0.4: VoxelGrid leaf of the history window; >= 0 */
  int32_t search_num;   /* 25 (historyKeyframeSearchNum); >= 0 */
  double min_gap_s;     /* 30 */
  lins_loop_icp_params icp;
  lins_pose_graph_params graph;
} lins_loop_step_params;
void lins_loop_step_default_params(lins_loop_step_params* p);

#define LINS_LOOP_CENTRE_STREAM 1 /* lins_loop_step_entry.flags: centre = currentRobotPosPoint of `stream` */

typedef struct lins_loop_step_entry {
  int32_t slot;
  int32_t stream;   /* -1, or the stream whose map pose the correction is written to */
  int32_t flags;    /* 0 or LINS_LOOP_CENTRE_STREAM: `centre` is not read, the search is centred on transform[3..5] of the
                       stream's last lins_streams_map_step entry with status LINS_OK (LM:1655-1658) */
  int32_t reserved;
  float centre[3];  /* currentRobotPosPoint */
  float pad;
  double now;       /* timeLaserOdometry */
} lins_loop_step_entry;

#define LINS_LOOP_NONE 0     /* no frames, no candidate, or the candidate is the latest frame itself */
#define LINS_LOOP_REPEAT 1   /* the candidate pair is the slot's most recent loop factor: nothing aligned or added */
#define LINS_LOOP_REJECTED 2 /* aligned; not converged, fitness above max_fitness, or an unusable variance */
#define LINS_LOOP_CLOSED 3   /* factor added, graph solved, history corrected */

typedef struct lins_loop_step_result { /* fields of stages that did not run are zero, the ids -1 */
  int32_t outcome;            /* LINS_LOOP_* */
  int32_t status;             /* LINS_OK; LINS_E_CAPACITY: the slot's graph holds max_loops loops (nothing was run), or the
                                 status of the entry's assembly / alignment / factor, behind which nothing ran for it */
  int32_t latest_id;          /* frames of the slot - 1 (-1: none) */
  int32_t closest_id;         /* lins_archive_find_loop's answer (-1: none) */
  lins_submap_info latest;    /* latestSurfKeyFrameCloud: corner | surf of `latest_id`, leaf 0, DROP_NEGATIVE */
  lins_submap_info history;   /* nearHistorySurfKeyFrameCloudDS: corner | surf of the window, history_leaf */
  lins_loop_icp_result icp;
  lins_key_pose pose_from;    /* lins_host_loop_pose_from of icp.transform and the graph's pose of `latest_id` */
  lins_pose_graph_result graph;
} lins_loop_step_result;

/* The stages, in order: detect (host: lins_archive_find_loop's selection, the candidate rule, and the loop capacity of
 * every slot with a candidate — a full slot reports LINS_E_CAPACITY with outcome NONE, the others proceed); assemble (one
 * lins_archive_assemble of two specs per candidate); align (one lins_loop_icp_batch over the entries whose assemblies have
 * no status); add the factor for every accepted entry (the graph's held pose of `latest`, pose_from, the variance rule);
 * solve (one lins_pose_graph_solve over the slots that gained a loop); correct the history (one
 * lins_pose_graph_apply_batch of those slots and their streams).
 * For the whole call, before anything is queued, and the call changes nothing: LINS_E_STATE before lins_archive_init or
 * lins_pose_graph_init, or for LINS_LOOP_CENTRE_STREAM on a stream that has not completed a step; LINS_E_ARG for a bad
 * slot, stream or flag, a slot or stream named twice, a named slot whose archive and graph hold different frame counts,
 * parameters outside the ranges of the calls they are handed to, or a write-back lins_pose_graph_apply would refuse;
 * LINS_E_INPUT for a non-finite centre or now.  The archive's last assembly and the ICP's buffers are this call's
 * afterwards, as after the explicit calls.
 * The same step with its candidates found by APPEARANCE — the K best separated places of the latest frame, every one
 * verified by ICP — is lins_loop_step_place of lins_place.h (its result carries a lins_place_result per candidate). */
int lins_loop_step(lins_ctx* ctx, int n, const lins_loop_step_entry* entries, const lins_loop_step_params* prm, lins_loop_step_result* out);
/* closed_cloud (LM:1143-1154) of entry `entry` of the last lins_loop_step, which must have been aligned (else LINS_E_ARG)
 * with no lins_archive_assemble since (LINS_E_STATE): the ICP contract's step 1 at the final T — M = T rounded to f32,
 * x' = ((m00 x + m01 y) + m02 z) + m03, uncontracted — over the source as assembled, intensity kept.  Returns the count;
 * LINS_E_CAPACITY beyond cap. */
int lins_loop_closed_cloud(lins_ctx* ctx, int entry, lins_point* out, int cap);
/* HIP-event times (ms) of the three device sequences of the last step (0 for one that did not run) and how many entries
 * had a candidate, were aligned, and closed a loop */
int lins_last_loop_step_stats(lins_ctx* ctx, float* assemble_ms, float* icp_ms, float* solve_ms, int32_t* candidates, int32_t* aligned,
                              int32_t* closed);

#ifdef __cplusplus
}
#endif
#endif /* LINS_MAP_H_ */
