// lins_launch.h — every host-callable launcher and capacity query of the kernel files, declared ONCE with parameter
// names.  The kernel file that defines a launcher includes this header (a changed signature is a compile error there),
// and so does every C API file that calls one.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lins_ieskf.h"
#include "../../include/lins_map.h"
#include "../../include/lins_streams_map.h"
#include "lins_records.h"

namespace lins_pg {
struct Prob;  // pose_graph.h
struct TeamProb;  // pose_graph_team.h
struct TeamCopy;
}
namespace lins_pcm {
struct Rec;  // host/team_pcm.h
}
struct lins_snapshot_segment;  // include/lins_snapshot.h

namespace lins {

struct DevParams;   // ieskf_device.h
struct ScanDesc;
struct RelayArgs;
struct GridTables;  // ieskf_grid.h
struct LmCarry;     // lm_math.h
struct MapRoundParams;
struct LmSeg;       // local_map.h
struct LmScanSeg;
struct LmJob;
struct LmState;
struct ArChunk;    // keyframe_archive.h
struct ArSplit;
struct ArMove;
struct KpStale;
struct KpEntry;
struct KpOut;
struct TsTarget;
struct TsEntry;
struct PlStale;    // place.h
struct PlParams;
struct PlEntry;
struct TmStale;
struct TmTarget;
struct TmQuery;

// ---- ieskf_kernels.hip: the any-size update kernel (global-memory grid or exhaustive search), re-projection, copy probe
void launch_persistent(hipStream_t stream, int n, const DevParams& prm, const ScanDesc* descs, const float4* arena, const double* state_in, const double* cov_in, double* state_out, double* cov_out,
                       double* a6, OutRec* out, int4* idx_store, lins_pose_record* poses, int scan_id_base, float4* binned, long long* prof);
void launch_pass(hipStream_t stream, int n, const DevParams& prm, const ScanDesc* descs, const float4* arena, const double* lin_state, const double* filt_state, int iter, int4* idx_store,
                 lins_corr* dump, double* sums_out, int* counts_out, float4* binned);
void launch_joseph(hipStream_t stream, int n, const DevParams& prm, const double* cov_in, const double* a6, const OutRec* out, double* cov_out);  // launch_persistent's covariance kernel alone
void launch_transform_to_end(hipStream_t stream, int n_jobs, int max_n, const ReprojectJob* jobs, const float4* in, float4* out_xyz, float4* out_yzx);
void launch_reproject_in_place(hipStream_t stream, int n_jobs, int max_n, const StreamCloud* jobs, const double* states, float4* arena, double inv_period);
void launch_stream_copy(hipStream_t stream, const float4* in, float4* out, size_t n);

// ---- ieskf_grid.hip: the search index of scans [0, n) of `descs` — sorted copy into gsorted (same offsets as the targets
// in the arena: positions 0 .. n_all - 1 at off_surf_t), tables into tab[scan]
void launch_grid_index(hipStream_t stream, int n, const ScanDesc* descs, const float4* arena, float4* gsorted, GridTables* tab);
// updatePointCloud in one kernel: the clouds `descs` name as targets are re-projected in place with states[scan] (19
// doubles each: t at 0, q at 6) and indexed as re-projected (grid_index_kernel<true>)
void launch_reproject_and_index(hipStream_t stream, int n, const ScanDesc* descs, float4* arena, float4* gsorted, GridTables* tab, const double* states, double inv_period);

// ---- ieskf_lds.hip: the full-residency LDS kernel (lanes = 3: 1024 threads, lanes = 1: 384 threads)
int lds_np_cap();  // target points of a scan the kernel takes
void launch_lds(hipStream_t stream, int n, const DevParams& prm, int lanes, const ScanDesc* descs, const float4* arena, const float4* sorted, const GridTables* tabs, const double* state_in,
                const double* cov_in, double* state_out, double* a6, double* cov_out, OutRec* out, int4* idx_store, lins_pose_record* poses, int scan_id_base, long long* prof, int* carry);
void launch_lds_pass(hipStream_t stream, int n, const DevParams& prm, int lanes, const ScanDesc* descs, const float4* arena, const float4* sorted, const GridTables* tabs, const double* lin_state,
                     const double* filt_state, int iter, int4* idx_store, lins_corr* dump, double* sums_out, int* counts_out);
// test aid (lins_debug_cov_update): joseph_epilogue of the shape `lanes` selects on n (prior, 21 sums, diverged) cases, one workgroup each
void launch_debug_cov_lds(hipStream_t stream, int n, int lanes, double r2, const double* cov_in, const double* sums, const int* diverged, double* cov_out);

// ---- ieskf_lds_mr.hip: the multi-resident (batch) LDS kernel
int lds_mr_np_cap();
bool lds_mr_has_parts();                   // the build has the several-part updates
int lds_mr_queue_flags_offset();           // ints of ticket counters in front of the per-scan flags of RelayArgs::queue
int lds_mr_resident_workgroups(int n_cu);  // workgroups resident at once on the current device
void launch_lds_mr(hipStream_t stream, int n, const DevParams& prm, const ScanDesc* descs, const int* order, const float4* arena, const float4* sorted, const GridTables* tabs, const double* state_in,
                   const double* cov_in, double* state_out, double* a6, double* cov_out, OutRec* out, int4* idx_store, lins_pose_record* poses, int scan_id_base, long long* prof,
                   const RelayArgs* relay, unsigned* walk_cache, int run_gen, int* carry);
void launch_lds_mr_icp(hipStream_t stream, int n, const DevParams& prm, const ScanDesc* descs, const float4* arena, const float4* sorted, const GridTables* tabs, const double* state_in,
                       double* state_out, OutRec* out, int4* idx_store);
void launch_lds_mr_pass(hipStream_t stream, int n, const DevParams& prm, const ScanDesc* descs, const float4* arena, const float4* sorted, const GridTables* tabs, const double* lin_state,
                        const double* filt_state, int iter, int4* idx_store, lins_corr* dump, double* sums_out, int* counts_out);
void launch_debug_cov_lds_mr(hipStream_t stream, int n, double r2, const double* cov_in, const double* sums, const int* diverged, double* cov_out);  // as launch_debug_cov_lds

// ---- frontend_kernels.hip / segment_kernels.hip
int fe_pick_stride();  // ints of pick scratch per scan
void launch_frontend(hipStream_t stream, int n_scans, const FeScan* scans, const float4* cloud, const float* range, const unsigned* col, const unsigned char* ground, double scan_period, int* picks,
                     float4* out, int* out_counts);
void launch_segment(hipStream_t stream, int n_scans, const SgRaw* raws, const float4* raw, float sin_ax, float cos_ax, float sin_ay, float cos_ay, float theta, unsigned* cellidx, int* seg_rows,
                    FeScan* fe_scans, float4* out_cloud, float* out_range, unsigned* out_col, unsigned char* out_ground, int* out_outliers,
                    float4* out_outl);  // out_outl: null, or the outlier arena (LINS_OUTLIER_MAX points per slot; scan k's slot: raws[k].o_slot)

// ---- filter_kernels.hip: the streams' device-resident filter (filter_math.h).  imu: rows (dt, acc, gyr), stream k's
// n_imu[k] rows start at row imu_off[k]; aux: lins_filt::kAux doubles per stream.  finish mode[k]: 0 leave the filter,
// 1 posterior state + covariance, 2 posterior state with the filter's own (prior) covariance
void launch_filter_predict(hipStream_t stream, int n, const int* n_imu, const int* imu_off, const double* imu, double* state, double* cov, const double* noise, double* aux);
void launch_filter_finish(hipStream_t stream, int n, const int* mode, const double* post_state, const double* post_cov, double* state, double* cov, const double* aux, double* gstate);

// ---- boot_kernels.hip: the streams' two-scan bootstrap (boot_math.h).  rows: this call's IMU rows component-major,
// element (row it, component j, stream k) at (it * 7 + j) * n + k; pre: lins_boot::kPre doubles per stream; tmpl: the
// lins_boot::kTmpl doubles of the filter template; list / icp_slot: the compact list of second scans and its inverse;
// scan: 8 doubles per stream (imu_last_ acc, gyr, the scan's time); finish mode[k]: 0 nothing, 1 first scan, 2 second scan
void launch_boot_preintegrate(hipStream_t stream, int n, const int* n_rows, const double* rows, const double* tmpl, double* pre, double* aux);
void launch_boot_start(hipStream_t stream, int m, const int* list, const double* pre, double* state_in);
void launch_boot_finish(hipStream_t stream, int n, const int* mode, const int* icp_slot, const double* icp_state, const double* scan, const double* tmpl,
                        double* pre, double* state, double* cov, double* noise, double* aux, double* gstate, double* lin);

// ---- debug_kernels.hip (lins_debug_math; op codes there)
void launch_debug_math(hipStream_t stream, int op, int n, int n_in, int n_out, const double* in, double* out);
void launch_debug_cycles(hipStream_t stream, int op, int blocks, const double* in, double* out);
void launch_debug_wave_solve(hipStream_t stream, int n, int gj, const double* in, double* out);
void launch_debug_icp_gn(hipStream_t stream, int n, int wave_version, const double* in, double* out);
void launch_debug_reduce_rows(hipStream_t stream, int op, int n, const double* in, double* out);

// ---- map_kernels.hip: scan-to-map
int map_block();  // queries per block of map_corr_kernel
void launch_map_selfcheck(hipStream_t stream, float* out);
void launch_map_grid(hipStream_t stream, int n_jobs, const MapGridJob* jobs, const float4* raw, float4* pts, int* cells);
void launch_map_corr(hipStream_t stream, int n_problems, int blocks_per_problem, const MapDev* probs, const MapRoundParams* rounds, const float4* pts, const int* cells, const float4* queries,
                     lins_map_corr* recs, double* partials);
void launch_map_lm(hipStream_t stream, int n, int iter, int blocks_per_problem, MapDev* probs, MapRoundParams* rounds, const double* partials, lins_map_result* results, LmCarry* carry);
void launch_debug_lm_step(hipStream_t stream, int n, int wave_version, const double* in, double* out, LmCarry* scratch);

// ---- map_pose_kernels.hip: the mapping node's pose arithmetic around scan-to-map (map_pose_math.h).  One lane per entry;
// probs[k].pad: < 0 the build entry's status, 1 the precondition of LM:1636 held, 0 it did not (associate: probs may be
// null = 0, results may be null).  odom null: transformSum is the entry's uploaded sum; else it is read from the resident
// record of the entry's stream, odom[entries[k].stream].transform_sum (lins_streams_map_step_resident)
void launch_map_associate(hipStream_t stream, int n, const MapPoseEntry* entries, const MapDev* probs, MapPoseRec* poses, lins_map_result* results,
                          lins_map_step_result* out, const lins_stream_odom* odom = nullptr);
void launch_map_pose_finish(hipStream_t stream, int n, const MapPoseEntry* entries, const MapDev* probs, MapPoseRec* poses,
                            const lins_map_result* results, lins_map_step_result* out, const lins_stream_odom* odom = nullptr);
// aft = last = tobe = fixes[k].p of stream fixes[k].stream, k < n; bef, prev and n_frames stay (a stream at most once)
void launch_map_pose_correct(hipStream_t stream, int n, const MapPoseFix* fixes, MapPoseRec* poses);

// ---- odom_kernels.hip: the seam between the streams' filter and their mapping step (odom_math.h).  One lane per stream / entry
// recs[k] of globalState_ row k (19 doubles), k < n; has[k] == 0: the stream has no globalState_ yet (valid = 0)
void launch_odom_records(hipStream_t stream, int n, const double* gstate, const int* has, lins_stream_odom* recs);
// out[k] = the transform fusion node's pose of stream list[k] from poses[list[k]].bef / .aft and recs[list[k]].transform_sum
void launch_odom_fuse(hipStream_t stream, int n, const int* list, const MapPoseRec* poses, const lins_stream_odom* recs, lins_fused_pose* out);

// ---- local_map_kernels.hip: the mapping node's local map
void launch_lm_transform(hipStream_t s, int n_blocks, const LmSeg* segs, const int2* blocks, const float4* frames, float4* stage, LmState* states);
// the scan clouds of a build out of the streams' arenas: (x, y, z) <- (y, z, x) into the staging arena at the segment's
// dst, f32 box folded into its job's state, a point outside the input contract flags the job (blocks: (segment, tile))
void launch_lm_stage_scans(hipStream_t s, int n_blocks, const LmScanSeg* segs, const int2* blocks, float4* stage, LmState* states);
// one stage: jobs [j0, j0 + n_jobs), tiles [0, n_tiles) of `tiles`
void launch_lm_stage(hipStream_t s, int j0, int n_jobs, int n_tiles, const int2* tiles, const LmJob* jobs, LmState* states, float4* stage, unsigned* keys_a, unsigned* keys_b, int* vals_a, int* vals_b,
                     int* hist, int* tilecnt, int* starts, float4* out);
// ... with the scans of its first n_split jobs split over many workgroups (launch_ar_scan below; chunks / splits: the
// tables of keyframe_archive.h for those jobs, csum: one int per chunk).  n_split == 0: the launches of launch_lm_stage
void launch_lm_stage_split(hipStream_t s, int j0, int n_split, int n_jobs, int n_tiles, const int2* tiles, const LmJob* jobs, LmState* states, float4* stage, unsigned* keys_a, unsigned* keys_b,
                           int* vals_a, int* vals_b, int* hist, int* tilecnt, int* starts, float4* out, int chunk_tiles, int n_chunks, const ArChunk* chunks, const ArSplit* splits, int* csum);
// the same kernels one by one (job kernels: jobs [j0, j0 + n_jobs); tile kernels: tiles [0, n_tiles) of `tiles`)
void launch_lm_setup(hipStream_t s, int j0, int n_jobs, const LmJob* jobs, LmState* states);
void launch_lm_keys(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const float4* stage, unsigned* keys, int* vals);
void launch_lm_hist(hipStream_t s, int pass, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const unsigned* kin, int* hist);
void launch_lm_scan(hipStream_t s, int pass, int j0, int n_jobs, const LmJob* jobs, const LmState* states, int* hist);
void launch_lm_scatter(hipStream_t s, int pass, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const int* hist, const unsigned* kin,
                       const int* vin, unsigned* kout, int* vout);
void launch_lm_heads(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const unsigned* keys_a, const unsigned* keys_b,
                     int* tilecnt);
void launch_lm_heads_scan(hipStream_t s, int j0, int n_jobs, const LmJob* jobs, LmState* states, int* tilecnt);
void launch_lm_starts(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const unsigned* keys_a, const unsigned* keys_b,
                      const int* tilecnt, int* starts);
void launch_lm_sum(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, LmState* states, const int* vals_a, const int* vals_b, const int* starts,
                   float4* stage, float4* out);

// ---- archive_kernels.hip: the key-frame archive's assembly (keyframe_archive.h)
// gather-transform from the archive arena into the staging arena, f32 box folded once per workgroup
void launch_ar_gather(hipStream_t s, int n_blocks, const LmSeg* segs, const int2* blocks, const float4* arena, float4* stage, LmState* states);
// the scan of lm_scan_kernel / lm_heads_scan_kernel over many workgroups, for the jobs the chunk tables name: `rows` x
// tiles counts per job at data + tile0 * rows (256: a radix pass's histogram, pass < the job's passes; 1: the per-tile
// counts, pass = -1, the total goes to the job's nvox), in chunks of rows * chunk_tiles elements of the digit-major row
void launch_ar_scan(hipStream_t s, int rows, int pass, int chunk_tiles, int n_chunks, const ArChunk* chunks, int n_splits, const ArSplit* splits,
                    const LmJob* jobs, LmState* states, int* data, int* csum);
// leaf == 0 jobs [j0, j0 + n_jobs), their tiles [0, n_tiles) of `tiles`: status, per-tile keep counts; then (behind the
// scan of the counts) the stable scatter of the kept points to out.  jflags[job] & 1: keep only (int)intensity >= 0
void launch_ar_keep(hipStream_t s, int j0, int n_jobs, int n_tiles, const int2* tiles, const LmJob* jobs, LmState* states, const int* jflags,
                    const float4* stage, int* tilecnt);
void launch_ar_compact(hipStream_t s, int n_tiles, const int2* tiles, const LmJob* jobs, const LmState* states, const int* jflags, const float4* stage,
                       const int* tilecnt, float4* out);
// the arena's compaction, one pass of the plan (host/arena_reclaim.h): blocks: the pass's (segment, tile) entries.  A
// staged pass is gather (arena -> stage) then scatter (stage -> arena); a direct pass — destination range in front of
// its first source — is one move inside the arena
void launch_ar_reclaim_gather(hipStream_t s, int n_blocks, const ArMove* segs, const int2* blocks, const float4* arena, float4* stage);
void launch_ar_reclaim_scatter(hipStream_t s, int n_blocks, const ArMove* segs, const int2* blocks, const float4* stage, float4* arena);
void launch_ar_reclaim_move(hipStream_t s, int n_blocks, const ArMove* segs, const int2* blocks, float4* arena);

// ---- keypose_select_kernels.hip: which key frames a map or a loop closure takes (keyframe_archive.h Kp*, keypose_select_math.h)
// the stale records into the mirror, one lane each
void launch_kp_refresh(hipStream_t s, int n, const KpStale* stale, float4* poses, double* times);
// radius search + pose grid, one workgroup per entry: entry k's ids to ids + k * stride (stride: the entries' own)
void launch_kp_select(hipStream_t s, int n, const KpEntry* entries, const float4* poses, int* ids, KpOut* out);
// ... and the list rule behind it: entry k's list at list_in + k * stride, the list afterwards at list_out + k * stride
void launch_kp_surround(hipStream_t s, int n, const KpEntry* entries, const float4* poses, const int* list_in, int* list_out, int* scratch, KpOut* out);
// the loop candidate: closest[k] = the hit of smallest (d, id) with fabs(time - now) > gap, or -1
void launch_kp_find_loop(hipStream_t s, int n, const KpEntry* entries, const float4* poses, const double* times, int* closest);
// ---- team_select_kernels.hip: the key frames of a team of slots around a centre (keyframe_archive.h Ts*, host/team_select.h)
// one workgroup per entry: entry k's survivors as (slot, id) to pairs + k * stride, ascending
void launch_team_select(hipStream_t s, int n, const TsEntry* entries, const TsTarget* targets, const float4* poses, int2* pairs, KpOut* out);

// ---- place_kernels.hip: place recognition over the archive's frames (place.h, host/place_math.h)
// the descriptors of the stale frames, one workgroup each: D to D + dst * 1200, the normalised columns to recs + dst * kPlRecWords
void launch_place_build(hipStream_t s, int n, const PlStale* stale, const float4* arena, const PlParams& prm, float* D, float* recs);
// one workgroup per (entry, first candidate) of `chunks`, `chunk` candidates each: its best key to chunk_best; then one
// workgroup per entry: the minimum of its chunks' bests to out.  row (may be null): every candidate's best key, at the entry's `row`
void launch_place_search(hipStream_t s, int n_entries, int n_chunks, const PlEntry* entries, const int2* chunks, int chunk, const float* recs,
                         unsigned long long* chunk_best, unsigned long long* row, unsigned long long* out);
// behind a search that wrote `row`: one workgroup per entry, the keys of its k best candidates more than min_sep ids apart
// to out + entry * k (kNoKey behind the last rank filled)
void launch_place_select(hipStream_t s, int n_entries, const PlEntry* entries, const unsigned long long* row, int k, int min_sep,
                         unsigned long long* out);

// ---- team_kernels.hip: the team search over the frames of many slots (place.h, the lower part of host/place_math.h)
// the ring keys of the stale frames, one wave each: two 16-byte words to keys + 2 * rec, read from D + rec * 1200
void launch_team_keys(hipStream_t s, int n, const TmStale* stale, const float* D, uint4* keys);
// one workgroup per (query, chunk) over the `total` concatenated candidates of `targets`, `chunk` <= kTmChunk each: the M
// smallest shortlist keys of the chunk to lists + (query * n_chunks + chunk) * M; then one workgroup per query: the M
// smallest of its lists to shortlist + query * M (kNoKey behind the last one there is)
void launch_team_shortlist(hipStream_t s, int n_queries, const TmQuery* queries, int n_targets, const TmTarget* targets, long long total, int chunk,
                           int n_chunks, int M, const uint4* keys, unsigned long long* lists, unsigned long long* shortlist);
// one workgroup per (query, ten shortlist positions): the row key of position m to row + query * M + m (kNoKey where the
// shortlist ends)
void launch_team_pairs(hipStream_t s, int n_queries, const TmQuery* queries, int M, int max_frames, const unsigned long long* shortlist,
                       const float* recs, unsigned long long* row);

// ---- rendezvous_consensus_kernels.hip: which alignments of a window of query frames agree (host/rendezvous_consensus.h)
// one workgroup of kCsBlock lanes per entry: entry e's hypotheses are table[offsets[e] .. offsets[e + 1]), at most
// kCsBlock of them, checked by lins_consensus::table_check; its record goes to out + e
constexpr int kCsBlock = 128;
void launch_rendezvous_consensus(hipStream_t s, int n, const ::lins_consensus_hyp* table, const int* offsets, double max_translation,
                                 double min_cos_rotation, ::lins_consensus_result* out);

// ---- team_pcm_kernels.hip: which team factors of a group agree two by two (host/team_pcm.h) ----
// one workgroup of kPcmBlock lanes per group: group g's records are recs[offsets[g] .. offsets[g + 1]), at most kPcmBlock
// of them, checked by the caller; its record goes to out + g
constexpr int kPcmBlock = 64;
void launch_team_pcm(hipStream_t s, int n_groups, const lins_pcm::Rec* recs, const int* offsets, const ::lins_team_pcm_params& prm,
                     ::lins_team_pcm_result* out);
// the search and the winners alone, one workgroup: n <= kPcmBlock rows and pair keys that lins_pcm::graph_check took
void launch_team_pcm_clique(hipStream_t s, int n, const uint64_t* adj, const int* key, const ::lins_team_pcm_params& prm, ::lins_team_pcm_result* out);

// ---- pose_graph_kernels.hip: the pose graph's solve, one workgroup per problem (pose_graph.h) ----
// the poses and the cost of every problem as it stands (the first launch of a solve)
void launch_pose_graph_begin(hipStream_t s, int n_problems, const lins_pg::Prob* probs);
// one Levenberg-Marquardt trial of every problem still active; still_running (may be null) += the problems that go on
void launch_pose_graph_trial(hipStream_t s, int n_problems, const lins_pg::Prob* probs, const lins_pose_graph_params& prm, int* still_running);

// ---- team_graph_kernels.hip: the team graph's solve, one workgroup per group of robots (pose_graph_team.h) ----
void launch_team_graph_begin(hipStream_t s, int n_groups, const lins_pg::TeamProb* probs);
void launch_team_graph_trial(hipStream_t s, int n_groups, const lins_pg::TeamProb* probs, const lins_pose_graph_params& prm, int* still_running);
// one workgroup per member: its Z and D rows into its group's rows, or (scatter) the solved rows back where recs[].store
void launch_team_graph_copy(hipStream_t s, int n_members, const lins_pg::TeamCopy* recs, bool scatter);

// ---- snapshot_kernels.hip: the device-resident pieces of a call's streams into / out of one staging buffer (include/
// lins_snapshot.h).  tiles: the (segment, tile) entries of the segments of `unit` bytes (16 or 8); bases: the module
// buffers by buffer id, on the device.  The segments have passed lins_snap::segments_ok.
void launch_snap_pack(hipStream_t s, int unit, int n_tiles, const ::lins_snapshot_segment* segs, const int2* tiles, void* const* bases, char* stage);
void launch_snap_unpack(hipStream_t s, int unit, int n_tiles, const ::lins_snapshot_segment* segs, const int2* tiles, void* const* bases, const char* stage);

}  // namespace lins
