#!/usr/bin/env python
"""Device time of the team search (include/lins_team.h) against the exhaustive search a caller had before it.

Fixture: 256 slots x 2 000 small synthetic places (as tools/place_rate.py) and one slot of 256 query frames; min_gap_s < 0
and the queries' slot outside the target list, so that every frame of every target slot is a candidate.
  key build     the key launch over every frame of the 64 / 256 target slots (descriptors already built)
  team search   lins_place_team_topk_batch for 1, 64 and 256 queries and M = 16 / 32 / 64 (k = 4): shortlist launches and
                pair launch, HIP-event ms
  exhaustive    the same queries answered by lins_place_search_batch once per target slot (n queries each), the sum of
                the calls' HIP-event search times: what the parent commit offers, on the same build
What the figures leave out: both sides are DEVICE-stage time.  The team figure has neither the host's rank selection
(select_team over n x M row keys, the admissible count over the query's own slot) nor the download of the n x M keys; the
exhaustive figure has neither its calls' downloads nor the minimum over the slots.  The archive is 64 distinct places
repeated, so most key distances tie: the order is decided by (slot, id), and recall on such an archive says nothing.
Median [min .. max] of 5 runs after one warm-up.
  tools/team_place_rate.py [output file]            -> profiles/team_place_rate.txt"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
REPS, SLOTS, FRAMES, QUERIES = 5, 256, 2000, 256
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def stat(v):
    import numpy as np
    v = np.array(v)
    return f"{np.median(v):9.3f} ms [{v.min():9.3f} .. {v.max():9.3f}]"

def context(pkg, ieskf):
    import place_cases as pc
    small = [pc.frame(pc.place(1000 + i, n=150)) for i in range(64)]
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    c.archive_init(SLOTS + 1, FRAMES, (SLOTS * FRAMES + QUERIES) * 150)
    for s in range(SLOTS):
        for i in range(FRAMES):
            c.archive_push(s, *small[(i * 7 + s) % 64], (0, 0, 0, 0, 0, 0), time=float(i))
    for i in range(QUERIES):
        c.archive_push(SLOTS, *small[(i * 5 + 1) % 64], (0, 0, 0, 0, 0, 0), time=1e6)
    assert c.place_init() == 0 and c.place_sync(list(range(SLOTS + 1))) == 0
    return c

def main(out_path):
    import numpy as np
    import __graft_entry__ as g
    g.build()
    pkg, ieskf, team = (importlib.import_module(PKG + m) for m in ("", ".ieskf", ".team"))
    say(f"team search over slots x {FRAMES} frames: HIP-event ms, median [min .. max] of {REPS} runs after 1 warm-up; k = 4, min_sep 0")
    with context(pkg, ieskf) as c:
        for ns in (64, SLOTS):
            targets = list(range(ns))
            # the key launch alone: lins_place_init drops the keys (and the descriptors, built again outside the timing)
            key = []
            for _ in range(REPS + 1):
                assert c.place_init() == 0 and c.place_sync(targets + [SLOTS]) == 0
                assert team.topk(c, [], targets) == []
                st = team.stats(c)
                assert st["frames_keyed"] == ns * FRAMES
                key.append(st["key_ms"])
            team.key(c, SLOTS, 0)  # (the queries' slot is keyed outside the timing too)
            say(f"{ns:4d} slots: key build of {ns * FRAMES} frames   {stat(key[1:])}")
            for nq in (1, 64, QUERIES):
                ex = []
                for _ in range(REPS + 1):
                    total = 0.0
                    for s in targets:
                        r = c.place_search([(SLOTS, q, s, 1e6, -1.0) for q in range(nq)])
                        assert isinstance(r, list)
                        total += c.place_stats()["search_ms"]
                    ex.append(total)
                ex = ex[1:]
                say(f"  {nq:4d} queries   exhaustive: lins_place_search_batch per target slot, summed   {stat(ex)}")
                for M in (16, 32, 64):
                    sh, pr = [], []
                    for _ in range(REPS + 1):
                        r = team.topk(c, [(SLOTS, q, 1e6, -1.0) for q in range(nq)], targets, shortlist=M, k=4)
                        st = team.stats(c)
                        assert isinstance(r, list) and st["scanned"] == nq * ns * FRAMES and st["frames_keyed"] == 0 and all(len(x) == 4 for x in r)
                        sh.append(st["shortlist_ms"]); pr.append(st["pair_ms"])
                    both = [a + b for a, b in zip(sh[1:], pr[1:])]
                    say(f"      M = {M:2d}   shortlist {stat(sh[1:])}   pairs {stat(pr[1:])}   both {stat(both)}   "
                        f"exhaustive / both {np.median(ex) / np.median(both):8.1f}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")

if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "team_place_rate.txt"))
