#!/usr/bin/env python
"""Device time of the top-K place search and of the loop thread's step by appearance (include/lins_place.h).

Block 1: lins_place_topk_batch — the search with its row buffer on plus the select launch — against
lins_place_search_batch alone, for 1 x 8000, 64 x 2000 and 256 x 8000 entries x candidates and K = 1, 4, 8 (min_sep 25;
small synthetic places as in tools/place_rate.py, min_gap_s < 0 so that every frame is a candidate).  HIP-event times,
median [min .. max] of 5 runs after one warm-up.
Block 2: one lins_loop_step_place (DETECT_PLACE, k = 4, min_sep = search_num) against one lins_loop_step at 64 and 256
slots on the fixture of tools/loop_step_rate.py (the 12-frame loop case in every slot, freshly pushed before every run),
wall time around the call, and the step's device sequences.
  tools/place_topk_rate.py [output file]            -> profiles/place_topk_rate.txt

A/B of the search a caller already has: --ab OTHER_LIB runs lins_place_search_batch of this tree's library and of
OTHER_LIB (a liblins_ieskf.so built from the parent commit) alternating, each in a process of its own, two rounds, on
the three shapes; they must agree within the runs' own min .. max spread.
  tools/place_topk_rate.py --ab ab/parent/liblins_ieskf.so [output file]   -> profiles/place_topk_ab.txt"""
import importlib, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "lins---lidar-inertial-slam_amd"
REPS = 5
SHAPES = ((1, 8000), (64, 2000), (256, 8000))  # entries x candidates
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

def stat(v):
    import numpy as np
    v = np.array(v)
    return f"{np.median(v):9.3f} ms [{v.min():9.3f} .. {v.max():9.3f}]"

def place_context(pkg, ieskf):
    import place_cases as pc
    small = [pc.frame(pc.place(1000 + i, n=150)) for i in range(64)]
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    c.archive_init(3, 8000, (2000 + 8000 + 256) * 150)
    for s, n in enumerate((2000, 8000)):
        for i in range(n):
            c.archive_push(s, *small[(i * 7 + s) % 64], (0, 0, 0, 0, 0, 0), time=float(i))
    for i in range(256):
        c.archive_push(2, *small[(i * 5 + 1) % 64], (0, 0, 0, 0, 0, 0), time=1e6)
    assert c.place_init() == 0 and c.place_sync([0, 1, 2]) == 0
    return c

def search_ms(c, ne, n):
    q = [(2, k, 0 if n == 2000 else 1, 1e6, -1.0) for k in range(ne)]
    ms = []
    for _ in range(REPS + 1):
        r = c.place_search(q)
        st = c.place_stats()
        assert st["pairs"] == ne * n and st["frames_built"] == 0 and all(x["candidates"] == n for x in r)
        ms.append(st["search_ms"])
    return ms[1:]

def topk_ms(c, ne, n, k, min_sep=25):
    q = [(2, i, 0 if n == 2000 else 1, 1e6, -1.0) for i in range(ne)]
    search, select = [], []
    for _ in range(REPS + 1):
        r = c.place_topk(q, k, min_sep)
        st = c.place_stats()
        assert st["pairs"] == ne * n and st["frames_built"] == 0 and all(len(x) == k for x in r)
        search.append(st["search_ms"]); select.append(c.place_select_ms())
    return search[1:], select[1:]

def main_search_only():
    pkg = importlib.import_module(PKG); ieskf = importlib.import_module(PKG + ".ieskf")
    with place_context(pkg, ieskf) as c:
        for ne, n in SHAPES:
            print(f"search {ne:4d} x {n:5d}   device {stat(search_ms(c, ne, n))}", flush=True)

def main_ab(other, out_path):
    say("lins_place_search_batch, HIP-event ms, median [min .. max] of 5 runs after 1 warm-up: the parent commit's library and this")
    say("branch's alternating in one visit (one MI355X), each run a process of its own; place_search_kernel is not edited")
    for rnd in range(2):
        for name, lib in (("parent", other), ("branch", "")):
            env = dict(os.environ)
            env.pop("LINS_IESKF_LIB", None)
            if lib:
                env["LINS_IESKF_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--search-only"], env=env, stdout=subprocess.PIPE, timeout=600, check=True)
            for l in out.stdout.decode().splitlines():
                if l.startswith("search"):
                    say(f"  {name}  {l}")
    open(out_path, "w").write("\n".join(lines) + "\n")

def main_rate(out_path):
    import numpy as np
    import __graft_entry__ as g
    g.build()
    pkg, ieskf, sm = (importlib.import_module(PKG + m) for m in ("", ".ieskf", ".streams_map"))
    import loop_step_cases as lsc
    say(f"top-K place search: HIP-event ms, median [min .. max] of {REPS} runs after 1 warm-up; min_sep 25")
    with place_context(pkg, ieskf) as c:
        for ne, n in SHAPES:
            alone = search_ms(c, ne, n)
            say(f"{ne:4d} entries x {n:5d} candidates   lins_place_search_batch alone          {stat(alone)}")
            for k in (1, 4, 8):
                se, sl = topk_ms(c, ne, n, k)
                both = [a + b for a, b in zip(se, sl)]
                say(f"    K = {k}   search with the row on {stat(se)}   select {stat(sl)}   both {stat(both)}   "
                    f"both / alone {np.median(both) / np.median(alone):6.3f}")
    say("")
    say("lins_loop_step_place (DETECT_PLACE, k 4, min_sep = search_num) against lins_loop_step: wall ms around the one call")
    prm = lsc.params(ieskf.lib())
    pl = lsc.defs.loop_place_params(ieskf.lib())
    for ns in (64, 256):
        slots = list(range(ns))
        with ieskf.IeskfContext(pkg.default_params(), max_batch=ns, max_targets=1024) as a, \
                ieskf.IeskfContext(pkg.default_params(), max_batch=ns, max_targets=1024) as b:
            for c in (a, b):
                c.streams_init(ns)
            w = dict(step=[], place=[], detect=[], select=[], assemble=[], icp=[], solve=[])
            closed = cands = 0
            for r in range(REPS + 1):
                for c in (a, b):  # freshly pushed state: every init drops what the last run left
                    lsc.init(c, ns)
                    sm.init(c, ns)
                    for s in slots:
                        lsc.push(c, s, "loop")
                assert b.place_init(up_axis=2) == 0 and b.place_sync(slots) == 0  # (described at push time, as a mapping thread would)
                entries = [lsc.defs.loop_step_entry(s, lsc.centre(), lsc.NOW, stream=s) for s in slots]
                t0 = time.perf_counter()
                ra = a.loop_step(entries, prm)
                t1 = time.perf_counter()
                rb = b.loop_step_place(entries, prm, pl)
                t2 = time.perf_counter()
                assert isinstance(rb, list)
                if r:
                    st, ps = b.loop_step_stats(), b.place_stats()
                    w["step"].append((t1 - t0) * 1e3), w["place"].append((t2 - t1) * 1e3)
                    w["detect"].append(ps["search_ms"]), w["select"].append(b.place_select_ms())
                    w["assemble"].append(st["assemble_ms"]), w["icp"].append(st["icp_ms"]), w["solve"].append(st["solve_ms"])
                    closed += st["closed"]; cands += sum(x["n_candidates"] for x in rb)
            say(f"{ns} slots of 12 frames: {cands / REPS:.0f} candidates verified and {closed / REPS:.1f} loops closed per step by appearance; "
                f"lins_loop_step closes {sum(x['outcome'] == 3 for x in ra)}")
            say(f"  lins_loop_step, wall                  {stat(w['step'])}")
            say(f"  lins_loop_step_place, wall            {stat(w['place'])}   / lins_loop_step {np.median(w['place']) / np.median(w['step']):.3f}")
            say(f"    top-K search (HIP events)           {stat(w['detect'])}")
            say(f"    top-K select (HIP events)           {stat(w['select'])}")
            say(f"    assembly (HIP events)               {stat(w['assemble'])}")
            say(f"    alignment of every rank (HIP events){stat(w['icp'])}")
            say(f"    solve (HIP events)                  {stat(w['solve'])}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write("\n".join(lines) + "\n")

if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--search-only"]:
        main_search_only()
    elif args[:1] == ["--ab"]:
        main_ab(args[1], args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "place_topk_ab.txt"))
    else:
        main_rate(args[0] if args else os.path.join(ROOT, "profiles", "place_topk_rate.txt"))
