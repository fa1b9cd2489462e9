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

/* n searches for the k best SEPARATED candidates each (k in [1, LINS_PLACE_MAX_K] of lins_host.h, min_sep >= 0, else
 * LINS_E_ARG; everything else as lins_place_search_batch): bit for bit lins_host_place_topk.  A candidate's row key is the
 * minimum of (distance, id, shift) over its shifts; rank 0 is the minimum row key — what lins_place_search_batch
 * returns, for every min_sep —, rank j the minimum among the candidates c with |c - id_i| > min_sep for every earlier
 * rank i.  results holds n * k records, entry e's ranks at results[e * k ..]; counts[e] is the number of ranks filled,
 * the records behind them are id -1, shift 0, distance 1; `candidates` is the entry's count in each of its records.
 * Device sequence: the search with its row buffer on (one key per candidate, sized for the batch), then one select
 * workgroup per entry; only the n * (1 + k) keys come back.  An entry's bits depend neither on its batch, nor on the
 * chunk, nor on what the context ran before. */
int lins_place_topk_batch(lins_ctx* ctx, int n, const lins_place_query* queries, int k, int min_sep, lins_place_result* results, int32_t* counts);

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

/* HIP-event time (ms) of the select launch of the last lins_place_topk_batch (0 after any other place call) */
int lins_last_place_select_ms(lins_ctx* ctx, float* select_ms);

/* lins_loop_icp_batch with T_0 = T0[16 k .. 16 k + 16) (row-major f64) instead of the identity for problem k:
 * lins_host_place_guess gives the start.  LINS_E_INPUT for a T0 that is not finite. */
int lins_loop_icp_batch_from(lins_ctx* ctx, int n, const lins_loop_icp_problem* in, const double* T0, const lins_loop_icp_params* prm,
                             lins_loop_icp_result* out);

/* ---- the loop thread's step with loops detected by APPEARANCE (lins_map.h lins_loop_step detects them from the poses) ----
 * The descriptor shortlists, the geometry decides: per entry the k best separated places of the slot's latest frame
 * (lins_place_topk_batch), every one verified by the ICP from its own guess in ONE batch, the best accepted fit closed by
 * lins_loop_step's own tail.  Stages, each one batched call over the entries that reach it:
 *   detect    lins_place_topk_batch: query = the slot's latest frame, target = the same slot, now = entry.now, min_gap_s
 *             = prm->min_gap_s.  Ranks with distance > max_distance are dropped; lins_host_loop_candidate per rank — a rank
 *             it calls a repeat is dropped; an entry whose ranks were all dropped as repeats is LINS_LOOP_REPEAT, one left
 *             without a rank LINS_LOOP_NONE.  The loop-capacity check is lins_loop_step's.
 *   assemble  one lins_archive_assemble: per entry the source (the latest frame, corner | surf, leaf 0, DROP_NEGATIVE) and
 *             one target per surviving rank, lins_host_loop_window(latest, id, search_num) at history_leaf
 *   align     one lins_loop_icp_batch_from over every (entry, rank): T0 = lins_host_place_guess(stored key pose of the
 *             latest frame, of the candidate, shift, the up_axis of lins_place_init)
 *   choose    lins_host_loop_choose per entry; -1: LINS_LOOP_REJECTED
 *   close     the chosen rank goes lins_loop_step's way by the same code: pose_from, the variance rule, the factor, one
 *             solve, one lins_pose_graph_apply_batch
 * An entry's result bits and the state it leaves are those of the explicit chain for its slot (DESIGN.md section 5.3 "Loop
 * thread's step by appearance"), independent of batch, order and history.  In LINS_LOOP_DETECT_POSE_THEN_PLACE an entry
 * whose pose search has a candidate is bit for bit lins_loop_step's entry (detect 0, cand[0].id = closest_id, its icp in
 * icp[0] when it was aligned).
 * Refusals: lins_loop_step's (in DETECT_PLACE the centre is not read, so its two do not apply), LINS_E_STATE before
 * lins_place_init, LINS_E_ARG for a mode outside the two, k outside [1, LINS_PLACE_MAX_K] or min_sep < -1;
 * LINS_E_CAPACITY when n (1 + k) submaps or n k alignments exceed what one assembly or one ICP batch takes.  All are
 * asked before anything is queued: a refused call changes nothing. */
#define LINS_LOOP_DETECT_PLACE 0           /* appearance only; entry.centre is not read */
#define LINS_LOOP_DETECT_POSE_THEN_PLACE 1 /* lins_loop_step's detect first; appearance only for entries it leaves without a candidate */

typedef struct lins_loop_place_params {
  int32_t mode;       /* LINS_LOOP_DETECT_* (default PLACE) */
  int32_t k;          /* 4: candidates verified per entry */
  int32_t min_sep;    /* -1: prm->search_num — two candidates closer than the window's half-width assemble nearly the same target */
  int32_t reserved;
  float max_distance; /* 1: distances lie in [0, 1], so the default gates nothing and the ICP is the gate */
  float pad;
} lins_loop_place_params;
void lins_loop_place_default_params(lins_loop_place_params* p);

typedef struct lins_loop_place_result {
  lins_loop_step_result step; /* as lins_loop_step's, for the chosen candidate (closest_id = its id, history = its window, icp = its
                                 alignment); without one: latest as assembled, closest_id -1, history and icp zero */
  int32_t detect;             /* 0: the candidate came from the pose search, 1: from appearance */
  int32_t n_candidates;       /* ranks that went to the alignment */
  int32_t chosen;             /* the chosen rank, or -1 */
  int32_t reserved;
  lins_place_result cand[LINS_PLACE_MAX_K]; /* the surviving ranks, in rank order; behind them id -1, shift 0, distance 1 */
  lins_loop_icp_result icp[LINS_PLACE_MAX_K];
} lins_loop_place_result;

int lins_loop_step_place(lins_ctx* ctx, int n, const lins_loop_step_entry* entries, const lins_loop_step_params* prm,
                         const lins_loop_place_params* place, lins_loop_place_result* out);

#ifdef __cplusplus
}
#endif
#endif
