/*
 * lins_team.h — rendezvous: which frame of ANOTHER robot looks like this one (entry points of liblins_ieskf.so;
 * csrc/lins_team_capi.hip, kernels csrc/team_kernels.hip; the definition is liblins_host.so's
 * lins_host_place_team_topk of lins_host.h, the scalar text the lower part of csrc/host/place_math.h in both libraries).
 *
 * lins_place_search_batch compares a query with every frame of ONE target slot under every yaw shift.  Over a team of
 * slots that is not affordable, so a team search shortlists first: every frame carries a ring key — per ring the number
 * of occupied sectors, Scan Context's rotation-invariant ring key kept as integers — and the candidates of every target
 * slot are ranked by the integer key distance; only the `shortlist` best of them reach the full comparison.  DESIGN.md
 * section 5.3 "Rendezvous" has the contract and its departures from the paper.
 *
 * The ring keys are a second derived mirror inside the place store, 32 bytes a frame (20 occupancy counts, the sum of
 * their squares, the frame's time), allocated for n_slots x max_frames_per_slot frames by the FIRST team call: a caller
 * who never searches a team pays nothing.  A slot's keys are dropped exactly where its descriptors are — lins_place_init,
 * lins_archive_release_slots, a restore — and built again on first use, from the descriptors.
 *
 * Conventions: lins_place.h's.  LINS_E_CAPACITY for an archive of more than LINS_PLACE_MAX_TEAM_SLOTS slots.
 */
#ifndef LINS_TEAM_H_
#define LINS_TEAM_H_

#include "lins_place.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lins_place_team_query {
  int32_t query_slot, query_id; /* the frame that asks */
  double now;       /* inside query_slot a candidate c is admissible iff c != query_id and fabs(time_c - now) > min_gap_s; */
  double min_gap_s; /* a frame of any other slot is always admissible: another robot's frame of the same second is what a rendezvous looks like */
} lins_place_team_query;

/* n queries against the frames of the n_targets slots of target_slots (one list for the call; it may hold a query's own
 * slot; no slot twice: LINS_E_ARG; n_targets = 0 or a slot without frames is allowed), bit for bit
 * lins_host_place_team_topk per query.  results holds n * prm->k records, entry e's ranks at results[e * k ..]; counts[e] is
 * the number of ranks filled, the records behind them are slot -1, id -1, shift 0, distance 1, dk -1; `candidates` is the
 * entry's count of admissible candidates in each of its records.
 * Device sequence: the stale frames of every slot named are described (lins_place_sync's launch), then ONE upload, the
 * key launch for the frames without a key, the shortlist launch (one workgroup per (query, chunk of the concatenated
 * candidates)) and its merge (one workgroup per query), the pair launch (the search's column walk over the n * shortlist
 * (query, candidate) pairs), one download of the n * shortlist shortlist and row keys, one synchronisation; the ranks are
 * chosen on the host.  An entry's bits depend neither on its batch, nor on the order of the target list, nor on the chunk,
 * nor on what the context ran before.  n = 0 is LINS_OK. */
int lins_place_team_topk_batch(lins_ctx* ctx, int n, const lins_place_team_query* queries, int n_targets, const int32_t* target_slots,
                               const lins_place_team_params* prm, lins_place_team_result* results, int32_t* counts);

/* the ring key of one frame as the device holds it (built on demand) */
int lins_place_team_key(lins_ctx* ctx, int slot, int id, uint8_t occ[LINS_PLACE_RINGS], uint32_t* sumsq, double* time);

/* test hook, as lins_place_set_chunk: candidates per workgroup of the shortlist launch; 0 = default, values beyond the
 * default (what the workgroup's LDS holds) are cut to it; results are the same bits for every value >= 1 */
int lins_place_team_set_chunk(lins_ctx* ctx, int chunk);

/* the last lins_place_team_topk_batch: HIP-event time (ms) of the key launch, of the shortlist launches (with the
 * merge) and of the pair launch; frames that got a key; (query, candidate) pairs the shortlist scanned — inadmissible ones
 * included, they are computed and masked */
int lins_last_place_team_stats(lins_ctx* ctx, float* key_ms, float* shortlist_ms, float* pair_ms, int32_t* frames_keyed, uint64_t* scanned);

/* ---- verification: did the robot of `slot` just see a place another robot has mapped, and how do the two map frames relate ----
 * The key shortlists, the descriptor ranks, the geometry decides.  Stages, each ONE batched call over the entries that
 * reach it:
 *   detect    lins_place_team_topk_batch: query = the slot's latest frame, now = entry.now, min_gap_s = prm->min_gap_s, the
 *             call's target list; team->min_sep = -1 means prm->search_num.  Ranks with distance > max_distance are dropped.
 *   assemble  one lins_archive_assemble: per entry the source (its latest frame, corner | surf, leaf 0, DROP_NEGATIVE) and
 *             one target per surviving rank, lins_host_loop_window(latest frame of the CANDIDATE's slot, id, search_num) at
 *             history_leaf, assembled from the candidate's slot
 *   align     one lins_loop_icp_batch_from over every (entry, rank): T0 = lins_host_place_team_guess(stored key pose of the
 *             query frame, of the candidate frame, shift, the up_axis of lins_place_init) — with the two poses taken from two
 *             slots it takes the query's map frame into the target's
 *   choose    lins_host_loop_choose per entry; -1: LINS_RENDEZVOUS_REJECTED
 * The call reads and changes no pose graph, no ring and no map pose.  An entry's bits are those of the explicit chain of the
 * four calls for its slot, in any batch and order.  Of prm the call reads max_fitness, history_leaf, search_num, min_gap_s
 * and icp.
 * Refusals: LINS_E_STATE before lins_archive_init / lins_place_init; LINS_E_ARG for a slot out of range or named twice among
 * the entries or among the targets, for parameters out of lins_loop_step's or lins_place_team_topk_batch's ranges
 * (min_sep < -1) or a NaN max_distance; LINS_E_INPUT for a now that is not finite; LINS_E_CAPACITY when n (1 + k) submaps
 * exceed what one assembly takes — asked of the most the ranks could ask for, every window as large as the largest target
 * slot's whole history (a submap of more than INT_MAX / 2 points, more than INT_MAX / 256 tiles of 512 points in the call).  All are asked before anything is queued: a refused call changes nothing. */
#define LINS_RENDEZVOUS_NONE 0     /* no frame, or no rank within max_distance */
#define LINS_RENDEZVOUS_REJECTED 1 /* ranks were aligned and none was accepted */
#define LINS_RENDEZVOUS_FOUND 2

typedef struct lins_rendezvous_entry {
  int32_t slot; /* the robot that asks: its latest frame is the query */
  int32_t reserved;
  double now;
} lins_rendezvous_entry;

typedef struct lins_rendezvous_params {
  lins_place_team_params team; /* shortlist 32, k 4, min_sep -1: prm->search_num */
  float max_distance;          /* 1: distances lie in [0, 1], so the default gates nothing and the ICP is the gate */
  float pad;
} lins_rendezvous_params;
void lins_rendezvous_default_params(lins_rendezvous_params* p);

typedef struct lins_rendezvous_result {
  int32_t outcome;                /* LINS_RENDEZVOUS_* */
  int32_t status;                 /* LINS_OK, or the first status of the entry's assemblies / alignments (then nothing is chosen) */
  int32_t latest_id;              /* the query frame; -1: the slot has no frame */
  int32_t n_candidates;           /* ranks that went to the alignment */
  int32_t chosen;                 /* the chosen rank, or -1 */
  int32_t target_slot, target_id; /* the chosen candidate, or -1, -1 */
  int32_t reserved;
  lins_submap_info latest;        /* the source as assembled */
  lins_place_team_result cand[LINS_PLACE_MAX_K]; /* the surviving ranks, in rank order; behind them slot -1, id -1, shift 0, distance 1, dk -1 */
  lins_submap_info target[LINS_PLACE_MAX_K];     /* their windows as assembled */
  lins_loop_icp_result icp[LINS_PLACE_MAX_K];
  double X[16]; /* FOUND: the chosen alignment, row-major f64 — it takes coordinates of the query slot's map frame to the
                   target slot's; otherwise zero */
} lins_rendezvous_result;

int lins_rendezvous_step(lins_ctx* ctx, int n, const lins_rendezvous_entry* entries, int n_targets, const int32_t* target_slots,
                         const lins_loop_step_params* prm, const lins_rendezvous_params* team, lins_rendezvous_result* out);

/* ---- merge: move a robot's whole history into the frame of the robot it met ----
 * The pose graph's unknowns are increments and its prior is satisfied exactly, so a change of map frame is a change of the
 * prior alone.  lins_pose_graph_rebase_batch, for each of the n slots (X + 16 k belongs to slots[k]):
 *   Z[0] <- X Z[0] in f64, by ONE product (csrc/pose_graph_math.h compose); no increment and no loop measurement is touched,
 *   so every factor's residual and the cost keep their values up to the rounding of the poses;
 *   the absolute poses of EVERY frame, frame 0 included, are formed again by the solve's phase_poses in its prefix order,
 *   through the solve's begin launch (one workgroup per slot) — for a graph without loops as well — and become the estimate
 *   (f64, and the six floats rounded once); the changed prior is uploaded.
 * X is 4 x 4 row-major f64 in the archive's axes: those of lins_key_pose's x, y, z, of the clouds, and of
 * lins_rendezvous_result.X, which can be passed as it is.  The graph's own axes are a permutation of them; the entries of X
 * are moved, not recomputed.
 * A graph that was never solved holds the poses as they were PUSHED; after a rebase it holds them COMPOSED from its
 * measurements.  So a rebase by the identity may move the bits of such a graph (by the rounding of the composition), and it
 * leaves the bits of a rebased or solved graph's f64 poses only as far as the composition repeats them.
 * lins_host_pose_graph_rebase (lins_host.h) is the same text on the CPU; device and host differ where libm does.
 * Refusals, all asked before anything is queued: LINS_E_STATE before lins_pose_graph_init; LINS_E_ARG for a slot out of
 * range, named twice, or without frames; LINS_E_INPUT for an X with an entry that is not finite, with a last row other than
 * 0 0 0 1, with |R^T R - I| > 1e-9 in some entry, or with det R <= 0.  n = 0 is LINS_OK. */
int lins_pose_graph_rebase_batch(lins_ctx* ctx, int n, const int32_t* slots, const double* X);

/* lins_pose_graph_rebase_batch followed by lins_pose_graph_apply_batch(ctx, n, slots, streams): the archive's key poses, the
 * local map's ring and the map poses of the streams named (streams[k] = -1: none) follow the graph through the code that
 * follows a solve.  Refusals: the union of the two calls', asked first on the graph as it stands.  The rebased poses
 * themselves must be ones the archive and the ring take (|x|, |y|, |z| <= 1e6): that is asked of the poses the begin launch
 * formed, before they are stored — LINS_E_INPUT then, and the graphs, the archive, the rings and the streams are as they were. */
int lins_team_rebase(lins_ctx* ctx, int n, const int32_t* slots, const int32_t* streams, const double* X);

/* ---- rendezvous over a window: merge only where several frames agree on X ----
 * lins_rendezvous_step decides from ONE frame, and nothing undoes a lins_team_rebase.  Here the last `window` frames of a
 * robot ask, and a merge is reported only where min_support of them agree on the same transform (DESIGN.md section 5.3
 * "Rendezvous over a window").
 *
 * The consensus rule is lins_host.h's lins_host_rendezvous_consensus (the scalar text csrc/host/rendezvous_consensus.h in
 * both libraries; the kernel, csrc/rendezvous_consensus_kernels.hip, calls that text).  lins_rendezvous_consensus_batch
 * answers n tables in one launch, one workgroup per table, bit for bit the host call per table.
 * Layout: `hypotheses` is ONE array of lins_consensus_hyp (176 bytes: X[16], p[3], fitness as 20 doubles, then query, rank,
 * target_slot, admissible) holding the tables back to back; `offsets` holds n + 1 entries, offsets[0] = 0, ascending;
 * table e is hypotheses[offsets[e] .. offsets[e + 1]), at most LINS_RENDEZVOUS_MAX_HYP of them (an empty table is allowed:
 * winner -1); results holds n records.  Of prm the call reads max_translation and min_cos_rotation.
 * Device sequence: ONE upload (the hypotheses | the offsets), one launch, one download, one synchronisation.  An entry's
 * bits depend neither on its batch, nor on the order of its hypotheses (up to the index mapping), nor on what the context
 * ran before.  n = 0 is LINS_OK.  The call needs a context only: no archive, no place store.
 * Refusals, all before anything is queued: LINS_E_ARG for a null pointer, offsets that do not start at 0, descend or give
 * a table more than LINS_RENDEZVOUS_MAX_HYP hypotheses, and whatever lins_host_rendezvous_consensus refuses with
 * LINS_E_ARG in some table; LINS_E_INPUT where it refuses with LINS_E_INPUT (an admissible hypothesis with an entry of X
 * or p that is not finite, or a fitness that is not finite or < 0). */
int lins_rendezvous_consensus_batch(lins_ctx* ctx, int n, const lins_consensus_hyp* hypotheses, const int32_t* offsets,
                                    const lins_consensus_params* prm, lins_consensus_result* results);
/* HIP-event time (ms) of the last consensus launch */
int lins_last_rendezvous_consensus_stats(lins_ctx* ctx, float* kernel_ms);

/* lins_rendezvous_window_step.  Stages, each ONE batched call over the entries that reach it, the whole a composition of
 * the public calls:
 *   queries   per entry the frames latest - j * stride, j = 0 .. window - 1, that exist (query 0 is the latest frame);
 *             every query uses entry.now
 *   detect    one lins_place_team_topk_batch over all queries of all entries, as lins_rendezvous_step.  Ranks with
 *             distance > max_distance are dropped, and so are the ranks INSIDE THE ASKING SLOT: a robot's own older frames
 *             would agree with each other on X = I and win.  They are never aligned.
 *   assemble  one lins_archive_assemble: per (entry, query) the source, per surviving rank the target window, the specs
 *             exactly lins_rendezvous_step's
 *   align     one lins_loop_icp_batch_from over every (entry, query, rank), T0 = lins_host_place_team_guess from that
 *             query frame's own stored pose
 *   consensus admissible = the alignment ran (status 0) and lins_host_loop_accept(converged, fitness, max_fitness) and
 *             its fitness and transform are finite (a NaN fitness passes lins_host_loop_accept; it is no witness here);
 *             p = the query frame's stored position; one lins_rendezvous_consensus_batch over the entries with a hypothesis
 *   outcome   NONE: no frame, or no rank survived.  REJECTED: ranks were aligned and none is admissible.  UNCONFIRMED: the
 *             winner's support is below min_support.  FOUND: X, target_slot, target_id are the winner's; X is its ICP
 *             transform unchanged and can go to lins_team_rebase as it is.
 * With window 1 and min_support 1 the outcome, the target and X are lins_rendezvous_step's wherever that step's ranks
 * hold none of the asking slot.
 * hyp: room for n * window * k records (k = team->team.k); entry e's records are hyp[e * window * k ..], n_hypotheses of
 * them in (query, rank) order — the order of the entry's consensus table, so `winner` and `members` index them; the records
 * behind them are zero.  The call reads and changes no pose graph, no ring and no map pose.  An entry's bits are those of
 * the explicit chain of the five calls for its slot, in any batch and order.
 * Refusals: lins_rendezvous_step's, LINS_E_ARG for consensus parameters out of range (window outside [1,
 * LINS_RENDEZVOUS_MAX_WINDOW], stride < 1, min_support outside [1, window], max_translation not finite or < 0, a NaN
 * min_cos_rotation) or a null hyp with n > 0; LINS_E_CAPACITY as lins_rendezvous_step, asked of the most the window can
 * ask for: n * window * (1 + k) submaps, every entry's queries that exist with k windows each as large as the largest
 * target slot's whole history.  All are asked before anything is queued: a refused call changes nothing. */
#define LINS_RENDEZVOUS_UNCONFIRMED 3 /* alignments were accepted, but fewer than min_support frames agree */

typedef struct lins_rendezvous_hypothesis {
  int32_t query, rank;        /* query: j of the frame latest - j * stride; rank: among that query's surviving ranks */
  int32_t admissible, member; /* member: 1 iff it is the winner or consistent with it */
  lins_place_team_result cand;
  lins_submap_info target;    /* its window as assembled */
  lins_loop_icp_result icp;
} lins_rendezvous_hypothesis;

typedef struct lins_rendezvous_window_result {
  int32_t outcome;                /* LINS_RENDEZVOUS_* */
  int32_t status;                 /* LINS_OK, or the first status of the entry's assemblies / alignments (then nothing is chosen) */
  int32_t n_queries;              /* frames that asked */
  int32_t n_hypotheses;           /* ranks that went to the alignment, over all queries */
  int32_t winner;                 /* index among the entry's hypotheses, or -1 */
  int32_t support, n_admissible;
  int32_t target_slot, target_id; /* FOUND: the winner's candidate; otherwise -1, -1 */
  int32_t reserved;
  uint32_t members[4];            /* as lins_consensus_result */
  int32_t query_id[LINS_RENDEZVOUS_MAX_WINDOW];     /* the frames that asked, query 0 first; -1 behind them */
  int32_t n_ranks[LINS_RENDEZVOUS_MAX_WINDOW];      /* per query: ranks that went to the alignment */
  lins_submap_info source[LINS_RENDEZVOUS_MAX_WINDOW]; /* per query: the source as assembled (zero when none of its ranks survived) */
  double X[16];                   /* FOUND: the winner's alignment; otherwise zero */
} lins_rendezvous_window_result;

int lins_rendezvous_window_step(lins_ctx* ctx, int n, const lins_rendezvous_entry* entries, int n_targets, const int32_t* target_slots,
                                const lins_loop_step_params* prm, const lins_rendezvous_params* team, const lins_consensus_params* consensus,
                                lins_rendezvous_window_result* out, lins_rendezvous_hypothesis* hyp);
/* the last lins_rendezvous_window_step: host-clock time (ms) of its stages — detect, assemble, align, consensus — and of
 * the whole call (each stage ends in a synchronisation) */
int lins_last_rendezvous_window_stats(lins_ctx* ctx, float* detect_ms, float* assemble_ms, float* align_ms, float* consensus_ms, float* total_ms);

/* ---- team graph: the pose graphs of the robots that met, solved jointly ----
 * (csrc/lins_team_graph_capi.hip, kernels csrc/team_graph_kernels.hip; the text of the solve is csrc/pose_graph_team.h in
 * both libraries, on the scalar pieces of csrc/pose_graph.h; lins_host.h has the CPU twin lins_host_team_graph_solve;
 * DESIGN.md section 5.3 "Team graph".)
 *
 * A GROUP is an ordered list of slots that share a map frame.  Its graph: every member's own graph as it stands (Z, the
 * increments D, its loops) and the TEAM FACTORS handed into the call.  The call is stateless: the context keeps no factor.
 *   Member 0, the anchor, keeps its prior exactly, as in lins_pose_graph_solve.
 *   Every other member's root T_0 is an unknown with ONE factor of odometry form, E = Z^-1 T_0, Z the member's current
 *   Z[0], under the six variances root_variance (rotation first); it retracts like an increment — an increment relative to
 *   the identity — and starts at Z.
 *   A team factor on ((slot_b, id_b), (slot_a, id_a)) is a loop factor in the existing form: E = Z^-1 T_b^-1 T_a, one
 *   variance for all six components, the loop's residual and retraction.  Its two slots are two DIFFERENT members.
 * Linearisation.  M = J_E Ad(T_a^-1), as a loop's but without the sign folded in.  The factor's row over unknown k is
 * sigma(k) M Ad(T_k): sigma = +1 for the unknowns of chain a with index <= id_a, -1 for those of chain b with index <= id_b,
 * the root included where it is an unknown.  A member's own loops keep their form: span (lo, hi], the sign folded into M.
 * The Woodbury core keeps its shape, S_{l,l'} = W^-1 delta + M_l (sum_k sigma_l(k) sigma_l'(k) P_k) M_l'^T, the sum over the
 * intersection of the two supports — at most one interval per chain, so at most two signed intervals.  ORDER of that sum:
 * the intervals in group order; each as 7 chunk sums over consecutive unknowns (the single solve's chunks), the chunks
 * added left to right; each total under its sign; then the totals left to right.  The right-hand side sums over a loop's
 * own intervals in the same order.
 * Poses: each member's by the single solve's prefix product, in blocks of 32 INSIDE the member; no block runs across two
 * members.  The cost order (lane t adds the unknowns t + 1, t + 257 ... of the concatenated chains, lane 0 the lanes, then the
 * loops), the accept rule and its `flat` rule, the lambda schedule and the stop reasons are lins_pose_graph_solve's, with
 * one lins_pose_graph_params.  Loop order inside a group: the members' loops first, in member order and each member's
 * own order, then the team factors in the caller's order.
 * A group's result bits are a function of the group AS LISTED — member order and factor order — and depend neither on the
 * batch, nor on the order of the groups, nor on what the context ran before.  Invariance under a permutation inside a
 * group is not promised.
 * GROUP OF ONE: a group of one member and no factor gives the bits of lins_pose_graph_solve of that slot — the result
 * record, the f64 poses, the six floats.  A group without any loop or factor returns the bits it holds with 0 iterations.
 *
 * What a solve leaves, in the host's graph and the device's rows of every member: the solved increments and poses (as a
 * single solve stores them), and for a non-anchor member Z[0] <- its solved root (as a rebase stores a prior; the held
 * floats are rounded once).  A later lins_pose_graph_solve, a snapshot or a lins_pose_graph_apply_batch of the members sees
 * a self-consistent graph; the archive, the rings and the streams follow through lins_pose_graph_apply_batch.
 * A group whose solved poses are not finite or lie beyond the archive's bound (|x|, |y|, |z| <= 1e6) — asked of the
 * device's solved poses before anything is stored — has solve.status LINS_E_INPUT, and none of its members changes.
 * DEPARTURE: a member's own lins_pose_graph_solve, and so lins_loop_step, knows nothing of team factors.  A caller with team
 * factors calls lins_team_graph_solve after the loop step.
 *
 * Limits: at most LINS_TEAM_GRAPH_MAX_MEMBERS members a group; the loops of a group — its members' own and its factors —
 * at most min(64, members x max_loops of lins_pose_graph_init): LINS_E_CAPACITY beyond either.
 * Refusals, all asked before anything is queued; a refused call changes nothing.  LINS_E_STATE before lins_pose_graph_init.
 * LINS_E_ARG: null pointers, offsets that do not start at 0 or descend, an empty group, a slot out of range, without
 * frames or named twice in the call, a factor naming a slot outside its group or the same member twice, a factor id out
 * of range, parameters lins_pose_graph_solve refuses.  LINS_E_INPUT: a Z that is not finite or whose rotation is no
 * rotation by lins_pose_graph_rebase_batch's bound, a var or a root_variance entry (of a non-anchor member) that is not
 * finite and > 0.  n_groups = 0 is LINS_OK.
 * Workspace: the concatenated Z / D / Dt / I / T / Tt / B / c / P / q rows of every group of the call, S, y, the loop
 * records and the states; grow-only, allocated by the FIRST team solve — a caller who never calls it pays nothing.
 * 1 248 bytes a frame (and 96 per 32 frames + 192 a member for the block prefixes), 672 bytes a loop and 288 L bytes of S
 * per loop in a group of L loops.
 * Device sequence: the members' new frames are uploaded as a solve uploads them; ONE upload of the tables (groups, members,
 * loop records, supports, states); the gather launch (one workgroup per member: its Z and D rows into the group's rows);
 * the begin launch and the trial launches, one workgroup of 256 lanes per GROUP, queued in fours with one "still running"
 * word read between them, as the single solve; ONE download of the states and the poses; the check; the scatter launch (the
 * solved D and T rows, and the non-anchor Z[0], into the members' own rows); one synchronisation each. */
#define LINS_TEAM_GRAPH_MAX_MEMBERS 32
/* (the records lins_team_factor, lins_team_member and lins_team_graph_result are lins_host.h's: both libraries use them) */

/* Z =(X T_b)^-1 T_a from the two graphs' f64 estimates as they stand, var = (double)(float)fitness.
 * X: 4 x 4 row-major f64, archive axes, as lins_rendezvous_result.X / a hypothesis' icp.transform; NULL: the identity (the
 * two slots already share a frame).  Built with X BEFORE lins_team_rebase by X, the factor's residual after it is zero up
 * to rounding.  Pure host work.  LINS_E_ARG: a slot or an id out of range, slot_b == slot_a, a null out; LINS_E_INPUT: an X
 * lins_pose_graph_rebase_batch refuses, a fitness that is not finite and > 0 once rounded. */
int lins_team_factor_from_alignment(lins_ctx* ctx, int slot_b, int id_b, int slot_a, int id_a, const double* X, double fitness,
                                    lins_team_factor* out);

/* n_groups groups: members[member_offsets[g] .. member_offsets[g + 1]), factors[factor_offsets[g] .. factor_offsets[g + 1]);
 * out: n_groups records */
int lins_team_graph_solve(lins_ctx* ctx, int n_groups, const lins_team_member* members, const int32_t* member_offsets,
                          const lins_team_factor* factors, const int32_t* factor_offsets, const lins_pose_graph_params* prm,
                          lins_team_graph_result* out);
/* the last lins_team_graph_solve: HIP-event time (ms) from the gather launch to the last trial, and the trials run */
int lins_last_team_graph_stats(lins_ctx* ctx, float* kernel_ms, uint64_t* iterations);

/* ---- pairwise-consistent team factors: which factors of a group agree with each other two by two ----
 * (csrc/lins_team_pcm_capi.hip, kernel csrc/team_pcm_kernels.hip; the rule is lins_host.h's
 * lins_host_team_factors_consistent, the scalar text csrc/host/team_pcm.h in both libraries, which the kernel calls;
 * DESIGN.md section 5.3 "Pairwise-consistent team factors".)
 *
 * lins_team_graph_solve takes every factor it is handed, and one aliased factor bends every member's history.  This call
 * comes ahead of it: per group and per pair of members it keeps the largest set of factors whose implied frame transforms
 * agree two by two — the consensus rule's rotation bar, and both places the robot stood within the translation bar —
 * and drops a pair's set below min_support.  The transform a factor implies depends on the two chains' relative poses
 * only, so the answer does not depend on the members' roots and can be asked BEFORE any lins_team_rebase.
 * Layout: lins_team_graph_solve's — members[member_offsets[g] .. member_offsets[g + 1]), factors[factor_offsets[g] ..
 * factor_offsets[g + 1]), out: n_groups records — with the same membership checks; root_variance is not read.  At most
 * LINS_TEAM_PCM_MAX_FACTORS factors a group, whatever max_loops of lins_pose_graph_init is.  The poses are the members'
 * f64 estimates in the context's host graphs.  In a record, factor f of its group is bit f % 32 of kept[f / 32].
 * The call reads and changes no graph, archive, ring or stream.  A group's bits are those of
 * lins_host_team_factors_consistent of the group as listed (slots replaced by member indices), `exact` and `nodes_max`
 * included, and depend neither on the batch, nor on the order of the groups, nor on what the context ran before.
 * Device sequence: ONE upload (the records | the offsets), one launch (one workgroup of 64 lanes per group), one download,
 * one synchronisation; the staging is grow-only and allocated by the first call.  n_groups = 0 is LINS_OK.
 * Refusals, all asked before anything is queued; a refused call changes nothing and writes nothing.  LINS_E_STATE before
 * lins_pose_graph_init.  LINS_E_ARG: null pointers, parameters lins_host_team_factors_consistent refuses, offsets that do
 * not start at 0 or descend, an empty group, a slot out of range, without frames or named twice in the call, a factor naming
 * a slot outside its group or the same member twice, a factor id out of range.  LINS_E_INPUT: a Z or a var that
 * lins_team_graph_solve refuses, a pose entry that is not finite.  LINS_E_CAPACITY: more than LINS_TEAM_PCM_MAX_FACTORS
 * factors or LINS_TEAM_GRAPH_MAX_MEMBERS members in a group. */
int lins_team_factors_consistent_batch(lins_ctx* ctx, int n_groups, const lins_team_member* members, const int32_t* member_offsets,
                                       const lins_team_factor* factors, const int32_t* factor_offsets, const lins_team_pcm_params* prm,
                                       lins_team_pcm_result* out);
/* HIP-event time (ms) of the last lins_team_factors_consistent_batch launch */
int lins_last_team_pcm_stats(lins_ctx* ctx, float* kernel_ms);
/* test aid: the search stage alone on a given graph, through the device function the production kernel calls; arguments
 * and refusals are lins_host_team_pcm_clique's */
int lins_debug_team_pcm_clique(lins_ctx* ctx, int n, const uint64_t* adj, const int32_t* pair, const lins_team_pcm_params* prm,
                               lins_team_pcm_result* out);

#ifdef __cplusplus
}
#endif
#endif
