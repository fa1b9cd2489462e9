// keyframe_archive.h — the device records of the key-frame archive's assembly (archive_kernels.hip,
// lins_archive_capi.hip).  An assembly is one VoxelGrid job (leaf > 0) or one compaction job (leaf == 0) per spec, in
// the records of the local-map build (local_map.h LmJob / LmState / LmSeg and its (job, tile) table): the VoxelGrid
// arithmetic is that build's kernels.  What is the archive's own is the gather from its arena, the compaction, and the
// scan of a large job's counts over many workgroups:
//   a job of more than `chunk` tiles has its digit-major row of (rows x tiles) counts cut into chunks of rows * chunk
//   elements; chunk sums (one workgroup per chunk) -> exclusive scan of the job's chunk sums (one workgroup per job) ->
//   each chunk re-scanned from its offset (one workgroup per chunk).  Integer sums: the same bits whatever the split.
#pragma once
#include <vector>

#include "local_map.h"

namespace lins {

constexpr int kArScanChunk = 16;  // default chunk (tiles): a job of at most this many tiles is scanned in one workgroup

struct ArChunk {  // one chunk of one split job
  int job;
  int k;       // chunk index within the job
  int c0;      // the job's first chunk sum in the chunk-sum arena
  int pad;
};
static_assert(sizeof(ArChunk) == 16, "ArChunk layout");

struct ArSplit {  // one split job
  int job;
  int c0, nc;  // its chunk sums
  int pad;
};
static_assert(sizeof(ArSplit) == 16, "ArSplit layout");

// ---- the arena's compaction (lins_archive_release_slots; the plan: host/arena_reclaim.h).  One segment of one pass:
// n points from arena + src to arena + dst, a staged pass by way of stage + stg (the pass's points lie packed there)
struct ArMove {
  long long src, dst, n;
  long long stg;
};
static_assert(sizeof(ArMove) == 32, "ArMove layout");
constexpr long long kArReclaimChunk = 1ll << 20;  // default points per pass (16 MiB of staging; DESIGN.md "Stream lifecycle")

// (host side) the clouds of the last assembly where the loop-closure ICP reads them: cloud k starts at d_out + off[k]
// and holds info[k].n points; filtered[k]: it went through VoxelGrid, so info[k] carries its 1 m box.  LINS_E_STATE
// when there was no assembly.
struct ArchiveView {
  const float4* d_out;
  int n;
  const long long* off;
  const lins_submap_info* info;
  const char* filtered;
  unsigned long long serial;  // counts the assemblies of the context: whose clouds these are
};
int archive_view(lins_ctx* ctx, ArchiveView* v);  // lins_archive_capi.hip

// (host side) one stored key frame, and the store where the local map's surround build (lins_local_map_build_surround)
// reads it: frame id of slot s is (*frames)[s][id], its clouds lie at d_arena + off.  LINS_E_STATE before lins_archive_init.
struct ArFrame {
  long long off;  // of the frame's block in the arena: corner, surf, outlier one after the other
  int n[3];
  lins_key_pose pose;
  float t[9];  // ctRoll, stRoll, ctPitch, stPitch, ctYaw, stYaw, tInX, tInY, tInZ
  double time;
};
struct ArchiveStore {
  const float4* d_arena;
  int n_slots;
  int chunk;  // lins_archive_set_scan_chunk: a job of more tiles has its scans split
  const std::vector<std::vector<ArFrame>>* frames;
};
int archive_store(lins_ctx* ctx, ArchiveStore* v);

// (host side) the team selection's host text (host/team_select.h) over the archive's own key poses, for the callers that
// select without the device: pairs gets the survivors as (slot, id), flattened.  LINS_OK, LINS_E_CAPACITY (the cell box)
// or LINS_E_ARG (a slot that is none, or named twice); LINS_E_STATE before lins_archive_init.
int archive_team_select_host(lins_ctx* ctx, int n_targets, const int32_t* slots, const float centre[3], float radius, float pose_leaf,
                             std::vector<int32_t>& pairs);

// ---- the key-pose selection on the device (keypose_select_kernels.hip, lins_keyposes_*): the slots' key poses and times
// have a device mirror, frame id of slot s at s * max_frames + id.  One workgroup serves one entry.
struct KpStale {  // one frame whose mirror record is out of date
  double time;
  float x, y, z;
  int pad;
  long long dst;  // its place in the mirror
};
static_assert(sizeof(KpStale) == 32, "KpStale layout");

struct KpEntry {
  long long base;      // the slot's first record in the mirror
  long long mark_off;  // surround: the entry's 2 * nf ints of scratch (the list rule's marks, then the selection)
  double now, gap;     // find-loop
  float c[3], r2, inv; // centre, radius * radius and 1 / pose_leaf as the host forms them
  int nf;              // frames of the slot
  int stride;          // ids (select) / list ids (surround) the entry's output holds
  int n_list;          // surround: the list's length
};
static_assert(sizeof(KpEntry) == 64, "KpEntry layout");

struct KpOut {
  int n, hits, status;
  int host;    // 1: more hits than the kernel sorts, or a selected id that is no frame — the host text serves the entry
  int n_list;  // surround: the list's length afterwards
  int pad[3];
};
static_assert(sizeof(KpOut) == 32, "KpOut layout");

// ---- the team selection (team_select_kernels.hip, lins_keyposes_team_select_batch; the contract: host/team_select.h).
// An entry's candidates are the frames of its targets, concatenated in ascending slot order: the candidate at place g
// is frame g - first of the last target whose first is <= g (a slot without frames shares its successor's place and is
// passed over).  A place orders as (slot, id).
constexpr int kTsCells = LINS_KEYPOSES_TEAM_CELLS;  // occupied cells an entry's LDS table serves; above: the host text
constexpr int kTsSlots = 2 * kTsCells;              // the table's places (open addressing, linear probing)

struct TsTarget {
  long long base;  // the slot's first record in the mirror
  int first;       // the place of its frame 0 in the entry's concatenation
  int slot;
};
static_assert(sizeof(TsTarget) == 16, "TsTarget layout");

struct TsEntry {
  float c[3], r2, inv;  // centre, radius * radius and 1 / pose_leaf as the host forms them
  int n_targets;
  int t0;               // the entry's first record in the call's TsTarget table
  int total;            // candidates: the frames of all targets
  int stride;           // pairs the entry's output holds
  int host;             // 1: the host text serves the entry whatever it holds (more candidates than a place can number)
  int pad[6];
};
static_assert(sizeof(TsEntry) == 64, "TsEntry layout");

}  // namespace lins
