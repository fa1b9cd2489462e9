// place.h — the device records of place recognition (place_kernels.hip, lins_place_capi.hip; the scalar text is
// host/place_math.h) and the descriptor store the key-frame archive keeps beside its key-pose mirror
// (lins_archive_capi.hip owns it and drops a slot's mark wherever the mirror's stale_from drops).
//
// Per frame the store holds 9 616 bytes, frame id of slot s at record s * max_frames + id:
//   D     1 200 f32, [ring][sector]: what lins_place_descriptor returns
//   rec   1 204 words: U column-major (sector-major, the 20 rings of a column contiguous: a column is five 16-byte reads)
//         | the 60 columns' valid bits in two words | the frame's time (f64)
// D plus U, not D plus norms: the search reads only `rec`, 4.8 KB a candidate, and divides nothing.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/lins_place.h"
#include "keyframe_archive.h"
#include "lins_buf.h"

namespace lins {

constexpr int kPlRecWords = 1204;   // words of one `rec`
constexpr int kPlMaskWord = 1200;   // valid bits: sector s is bit s of the 64-bit word here
constexpr int kPlTimeWord = 1202;   // the frame's time
constexpr int kPlBuildBlock = 256;  // threads of the build kernel: the tile of points it takes per step
constexpr int kPlChunk = 20;        // default candidates per workgroup of the search
constexpr int kPlSelectBlock = 256; // threads of the top-K select: four waves stride an entry's row

struct PlStale {  // one frame whose descriptor is to be built
  long long src;  // its block in the archive's arena: corner, surf, outlier one after the other
  long long dst;  // its record
  double time;
  int n[3];
  int pad;
};
static_assert(sizeof(PlStale) == 40, "PlStale layout");

struct PlParams {
  float r_max, lift, inv_r;
  int up, clouds;
};

struct PlEntry {  // one search
  long long q_rec;  // the query's record
  long long base;   // the target slot's first record
  long long row;    // lins_place_distances: the entry's first key in `row`
  double now, gap;
  int nf;           // frames of the target slot
  int skip;         // the id that is the query itself, or -1
  int chunk0, n_chunks;  // its chunks' bests
};
static_assert(sizeof(PlEntry) == 56, "PlEntry layout");

// ---- team search (include/lins_team.h; team_kernels.hip, lins_team_capi.hip): the ring keys, 32 bytes a frame beside
// its descriptor — lins_place::RingKey, two 16-byte words: occ[0 .. 16) | occ[16 .. 20), sumsq, the frame's time
constexpr int kTmBlock = 256;     // threads of the key, shortlist and merge kernels
constexpr int kTmChunk = 2048;    // candidates per workgroup of the shortlist, at most: their keys lie in LDS (16 KB)

struct TmStale {  // one frame whose key is to be built
  long long rec;  // its record
  double time;
};
static_assert(sizeof(TmStale) == 16, "TmStale layout");

struct TmTarget {  // one target slot of a call
  long long base;   // its first record
  long long first;  // the place of its frame 0 among the call's concatenated candidates
  int slot, nf;
};
static_assert(sizeof(TmTarget) == 24, "TmTarget layout");

struct TmQuery {
  long long q_rec;  // the query's record
  double now, gap;
  int slot, id;
};
static_assert(sizeof(TmQuery) == 32, "TmQuery layout");

// the staging of lins_rendezvous_consensus_batch and the last calls' times: no frame's state, nothing a snapshot carries
struct ConsensusStore {
  DevBuf<char> d_up, d_down;  // (bytes) the hypotheses | the offsets; the results
  PinBuf<char> h_up, h_down;
  Event ev[2];  // around the launch
  float kernel_ms = 0.f;
  float stage_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // the last lins_rendezvous_window_step: detect, assemble, align, consensus, the whole call (host clock)
};
ConsensusStore* archive_consensus(lins_ctx* ctx);  // lins_archive_capi.hip: the context's, before lins_archive_init as well

struct TeamStore {
  std::vector<int> keyed;  // [slot]: ring keys are current below this id; empty until the first team call
  DevBuf<uint4> d_key;     // two a frame; allocated by the first team call
  int chunk = kTmChunk;
  DevBuf<char> d_up, d_down;  // (bytes)
  PinBuf<char> h_up, h_down;
  Event ev[4];  // before the keys, between keys and shortlist, between merge and pairs, behind the pairs
  float key_ms = 0.f, shortlist_ms = 0.f, pair_ms = 0.f;
  uint64_t scanned = 0;
  int built = 0;  // frames the last call keyed
  ConsensusStore consensus;
  void drop() { keyed.clear(), d_key.reset(); }
  void drop_slot(int slot) {
    if (!keyed.empty()) keyed[slot] = 0;
  }
};

struct PlaceStore {
  bool on = false;
  lins_place_params prm{};
  int chunk = kPlChunk;
  std::vector<int> described;  // [slot]: descriptors are current below this id
  DevBuf<float> d_D, d_rec;
  DevBuf<char> d_up, d_down;  // (bytes)
  PinBuf<char> h_up, h_down;
  Event ev[4];  // before the build, between build and search, behind the search, behind the select
  float build_ms = 0.f, search_ms = 0.f, select_ms = 0.f;
  uint64_t pairs = 0;
  int built = 0;  // frames the last call described
  TeamStore team;  // the ring keys: marks drop wherever `described` drops
};

// (host side) the store and the archive it describes; LINS_E_STATE before lins_archive_init
struct ArchivePlace {
  PlaceStore* store;
  const float4* d_arena;
  int n_slots, max_frames;
  const std::vector<std::vector<ArFrame>>* frames;
};
int archive_place(lins_ctx* ctx, ArchivePlace* v);  // lins_archive_capi.hip

}  // namespace lins
