/*
 * lins_lifecycle.h — ending one stream while the others keep running (entry points of liblins_ieskf.so;
 * csrc/lins_lifecycle_capi.hip and the release functions of the modules' own files, kernels ar_reclaim_* of
 * csrc/archive_kernels.hip; the compaction plan csrc/host/arena_reclaim.h is exported by liblins_host.so as
 * lins_host_arena_reclaim_plan).
 *
 * The init calls size every module once and a second call drops every stream.  A release puts the slots named back to
 * what their init left — field for field, so that what runs in the slot next gives the bits a fresh context gives —
 * and leaves the state and the results of every other slot untouched.  The key-frame archive's arena is bump-allocated:
 * a release compacts it on the device (stable: frame ids of the kept slots and each frame's corner | surf | outlier
 * layout survive), so that the points of the released slots can be pushed again.
 *
 * Conventions of every call here: LINS_E_STATE before the module's init; LINS_E_ARG for a slot / stream out of range or
 * named twice; n = 0 is LINS_OK.  Everything that can refuse is asked first: a refused call changes nothing.  Each call
 * synchronises the context's stream (behind the second launch queue, where one exists) before it touches state.
 * DESIGN.md section 5.3 "Stream lifecycle".
 */
#ifndef LINS_LIFECYCLE_H_
#define LINS_LIFECYCLE_H_

#include "lins_streams_slam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* arena accounting: points in use / points of capacity (LINS_E_STATE before lins_archive_init) */
int lins_archive_usage(lins_ctx* ctx, long long* used, long long* capacity);

/* drop every frame of the n slots named (each at most once), compact the arena; *released (may be NULL): points freed.
 * Afterwards the slots' frame lists are empty (ids restart at 0), every kept frame keeps its id and its points, the
 * key-pose mirror of the released slots is stale from id 0, and the clouds of the last assembly are as they were.   */
int lins_archive_release_slots(lins_ctx* ctx, int n, const int32_t* slots, long long* released);

/* test hook, as lins_archive_set_scan_chunk: points moved per compaction pass; 0 = default; results are the same bits
 * for every value >= 1 (LINS_E_ARG below 0)                                                                          */
int lins_archive_set_reclaim_chunk(lins_ctx* ctx, long long chunk_points);

int lins_pose_graph_release_slot(lins_ctx* ctx, int slot); /* frames, loops, estimate: as after lins_pose_graph_init */
int lins_local_map_release_slot(lins_ctx* ctx, int slot);  /* the slot's ring: empty */

/* the filter side of the streams named: resident scan and outlier counts, the device filter (no filter loaded), in
 * machine mode status LINS_STREAM_INIT with no IMU row seen and an empty pre-integration record, the odometry record
 * not valid — what lins_streams_init (+ lins_streams_machine_init) leave.  LINS_E_STATE before lins_streams_init or on
 * a failed streams context.                                                                                          */
int lins_streams_release(lins_ctx* ctx, int n, const int32_t* streams);

/* the mapping side: the stream's map pose as lins_streams_map_init leaves it, last_time = -1, no centre, an empty
 * surround list.  The modes of the context (loop, surround, interval) are not per stream and stay.                  */
int lins_streams_map_release(lins_ctx* ctx, int n, const int32_t* streams);

/* all of the above for stream == slot, in every module that is initialised, one call: LINS_E_STATE before
 * lins_streams_init, modules that are not initialised are skipped, LINS_E_ARG when a stream is out of range in any
 * initialised module                                                                                                 */
int lins_streams_retire(lins_ctx* ctx, int n, const int32_t* streams);

/* HIP-event time (ms) of the last compaction, points moved, passes run (staged: through the staging buffer; direct:
 * one arena-to-arena move) — zeros when the last release moved nothing                                               */
int lins_last_reclaim_stats(lins_ctx* ctx, float* ms, uint64_t* points_moved, int32_t* staged_passes, int32_t* direct_passes);

/* ---- the compaction plan (liblins_host.so; the same inline text the device path runs, csrc/host/arena_reclaim.h) --
 * blocks: the arena's blocks in ascending offset order, not overlapping.  The plan moves every kept block that lies
 * behind the first dropped one down to close the gaps, in passes of at most chunk points; a block may be split over
 * passes.  segs[i].pass counts from 0; segs[i].direct (the same for every segment of a pass) says that the pass's
 * destination range ends at or before its first source, so that one forward copy serves it; the other passes copy
 * out to a staging buffer of chunk points first, then in.  Invariant: after pass p has written [D_p, D_p + m_p),
 * every surviving point not yet moved has its source at or beyond D_p + m_p.
 * Returns the number of segments (only the first cap are written; segs may be NULL with cap = 0), *n_passes (may be
 * NULL) the number of passes; LINS_E_ARG for chunk < 1, a negative count, or blocks out of order.                   */
typedef struct lins_arena_block {
  long long off, n; /* points */
  int32_t keep, reserved;
} lins_arena_block;

typedef struct lins_arena_segment {
  long long src, dst, n; /* points; dst <= src */
  int32_t pass, direct;
} lins_arena_segment;

long long lins_host_arena_reclaim_plan(int n_blocks, const lins_arena_block* blocks, long long chunk, lins_arena_segment* segs,
                                       long long cap, int32_t* n_passes);

#ifdef __cplusplus
}
#endif
#endif
