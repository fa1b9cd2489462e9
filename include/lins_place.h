/*
 * lins_place.h — place recognition over the key-frame archive: which stored frame LOOKS like this one (entry points of
 * liblins_ieskf.so; csrc/lins_place_capi.hip, kernels csrc/place_kernels.hip; the definition is liblins_host.so's
 * lins_host_place_* of lins_host.h, the scalar text csrc/host/place_math.h in both libraries).
 *
 * lins_archive_find_loop finds a loop from the poses: the first stored key pose within a radius of where the robot
 * believes it is.  This finds it from the scans — Scan Context (Kim & Kim, IROS 2018): a polar height signature of
 * LINS_PLACE_RINGS x LINS_PLACE_SECTORS cells per key frame, compared under every yaw shift, exhaustively and exactly:
 * a search returns the minimum of (distance, id, shift) over every admissible candidate, bit for bit what
 * lins_host_place_search returns.  DESIGN.md section 5.3 "Place recognition" has the contract and its departures from
 * the paper.
 *
 * The descriptors are a derived mirror inside the archive, 9 616 bytes a frame (the f32 descriptor, and its normalised
 * columns with their valid bits and the frame's time), allocated for n_slots x max_frames_per_slot frames by
 * lins_place_init.  A frame is described on first use, or by lins_place_sync; a descriptor depends on the frame's points
 * only, so lins_archive_set_poses and the arena's compaction leave it, and a released or restored slot is described anew.
 *
 * Conventions: LINS_E_STATE before lins_archive_init / lins_place_init (lins_archive_init drops the store: call
 * lins_place_init again); LINS_E_ARG for a slot, id, mask or axis out of range; LINS_E_INPUT for a NaN gap or a time
 * that is not finite.  Every refusal is asked before anything is queued: a refused call changes nothing.
 */
#ifndef LINS_PLACE_H_
#define LINS_PLACE_H_

#include "lins_host.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lins_place_query {
  int32_t query_slot, query_id; /* the frame that asks */
  int32_t target_slot;          /* the slot whose frames are searched */
  int32_t reserved;
  double now;       /* a candidate c is admissible iff fabs(time_c - now) > min_gap_s (lins_archive_find_loop's gate) */
  double min_gap_s; /* < 0: every other frame; the query frame itself is never admissible */
} lins_place_query;

typedef struct lins_place_result {
  int32_t id;    /* -1: no admissible candidate (then shift 0, distance 1) */
  int32_t shift; /* what the query sees at azimuth phi the candidate sees at phi + shift 2 pi / LINS_PLACE_SECTORS */
  float distance;
  int32_t candidates; /* admissible candidates */
  int32_t status;
  int32_t reserved;
} lins_place_result;

/* sizes the store for the archive as it is initialised; a second call drops every descriptor.  LINS_E_CAPACITY for an
 * archive of more than 2^26 frames a slot (the ids a packed search key holds). */
int lins_place_init(lins_ctx* ctx, const lins_place_params* params);

/* describes the stale frames of the n slots named now (a slot may be named twice) */
int lins_place_sync(lins_ctx* ctx, int n, const int32_t* slots);

/* n searches: one upload, one build launch for the stale frames of every slot named, the search launches, one download,
 * one synchronisation.  An entry's bits depend neither on its batch, nor on how its candidates are cut into chunks, nor
 * on what the context ran before.  n = 0 is LINS_OK. */
int lins_place_search_batch(lins_ctx* ctx, int n, const lins_place_query* queries, lins_place_result* results);

/* the descriptor of one frame, D[ring][sector] */
int lins_place_descriptor(lins_ctx* ctx, int slot, int id, float out[LINS_PLACE_CELLS]);

/* test aid: one entry's whole row — per frame c of the target slot the smallest d over the shifts and the smallest shift
 * that gives it, d[c] = -1 and shift[c] = -1 for an inadmissible c.  Returns the number of frames; LINS_E_CAPACITY
 * beyond cap. */
int lins_place_distances(lins_ctx* ctx, const lins_place_query* query, float* d, int32_t* shift, int cap);

/* test hook, as lins_archive_set_scan_chunk: candidates per workgroup of the search; 0 = default; results are the same
 * bits for every value >= 1 */
int lins_place_set_chunk(lins_ctx* ctx, int chunk);

/* the last lins_place_sync / _search_batch / _distances: HIP-event time of the build and of the search (ms), frames
 * described, (query, candidate) pairs compared — inadmissible ones included, they are computed and masked */
int lins_last_place_stats(lins_ctx* ctx, float* build_ms, float* search_ms, uint64_t* pairs, int32_t* frames_built);

/* lins_loop_icp_batch with T_0 = T0[16 k .. 16 k + 16) (row-major f64) instead of the identity for problem k:
 * lins_host_place_guess gives the start.  LINS_E_INPUT for a T0 that is not finite. */
int lins_loop_icp_batch_from(lins_ctx* ctx, int n, const lins_loop_icp_problem* in, const double* T0, const lins_loop_icp_params* prm,
                             lins_loop_icp_result* out);

#ifdef __cplusplus
}
#endif
#endif
