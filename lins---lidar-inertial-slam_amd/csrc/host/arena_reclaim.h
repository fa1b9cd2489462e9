// arena_reclaim.h — the plan of the key-frame archive's compaction (include/lins_lifecycle.h), one text for both
// libraries: lins_archive_release_slots (lins_archive_capi.hip) executes it on the device, liblins_host.so exports it as
// lins_host_arena_reclaim_plan (host/arena_reclaim.cpp) and tests/test_reclaim_host.py executes it on a numpy array.
//
// Input: the arena's blocks in ascending offset order (not overlapping), each kept or dropped, and a chunk C >= 1.
// Every kept block behind the first dropped one moves down by the points dropped in front of it: a stable compaction
// (order kept, dst <= src).  The moves are cut into passes of at most C points; a block may be split over passes.
//   direct pass   its destination range [D_p, D_p + m_p) ends at or before its first source: no lane of one arena-to-arena
//                 launch reads what another writes
//   staged pass   otherwise: out to a staging buffer of C points, then in
// Invariant (why executing the passes in order is a compaction): after pass p has written [D_p, D_p + m_p), every
// surviving point not yet moved has its source at or beyond D_p + m_p.  Proof: the point moved next has dst = D_p + m_p
// (destinations are handed out consecutively) and dst <= src; sources ascend with destinations.  So a pass overwrites
// only dropped points, points moved by an earlier pass, and — a staged pass — its own sources, which are in the staging
// buffer by then.
#pragma once
#include <vector>

#include "../../../include/lins_lifecycle.h"

namespace lins_reclaim {

inline bool blocks_ok(int n_blocks, const lins_arena_block* b) {
  if (n_blocks < 0 || (n_blocks && !b)) return false;
  long long end = 0;
  for (int i = 0; i < n_blocks; ++i) {
    if (b[i].off < end || b[i].n < 0) return false;
    end = b[i].off + b[i].n;
  }
  return true;
}

// where block i starts after the compaction (a dropped block: -1)
inline std::vector<long long> new_offsets(int n_blocks, const lins_arena_block* b) {
  std::vector<long long> off((size_t)n_blocks, -1);
  bool dropped = false;
  long long at = 0;
  for (int i = 0; i < n_blocks; ++i) {
    if (!b[i].keep) {
      if (!dropped) dropped = true, at = b[i].off;
      continue;
    }
    off[i] = dropped ? at : b[i].off;
    if (dropped) at += b[i].n;
  }
  return off;
}

// the segments of all passes in arena order; returns the number of passes
inline int plan(int n_blocks, const lins_arena_block* b, long long chunk, std::vector<lins_arena_segment>& segs) {
  segs.clear();
  const std::vector<long long> to = new_offsets(n_blocks, b);
  int pass = 0;
  long long in_pass = 0;  // points of the pass being filled
  size_t first = 0;       // its first segment
  auto close = [&]() {    // direct: the pass's destination range ends at or before its first source
    if (first == segs.size()) return;
    const lins_arena_segment& a = segs[first];
    const int direct = a.dst + in_pass <= a.src;
    for (size_t i = first; i < segs.size(); ++i) segs[i].direct = direct;
    first = segs.size(), in_pass = 0, pass += 1;
  };
  for (int i = 0; i < n_blocks; ++i) {
    if (!b[i].keep || to[i] == b[i].off) continue;  // dropped, or in front of the first dropped block
    for (long long done = 0; done < b[i].n;) {
      const long long cnt = b[i].n - done < chunk - in_pass ? b[i].n - done : chunk - in_pass;
      segs.push_back(lins_arena_segment{b[i].off + done, to[i] + done, cnt, pass, 0});
      done += cnt, in_pass += cnt;
      if (in_pass == chunk) close();
    }
  }
  close();
  return pass;
}

}  // namespace lins_reclaim
