"""The case in which the descriptor's winner is the WRONG place (tests/test_place_verify_inputs.py on the CPU,
tests/test_gpu_loop_step_place.py on the device; not a test): tests/place_loop_cases.py with its three wall pieces
lowered to 0.15 m and 900 points on them, everything else as there.  The low pieces no longer tell frame 1 from frame 7,
its twin under the room's half turn: by appearance the twin leads, the ICP from the twin's guess converges under the
reference's fitness bar, and a pipeline that verifies only the winner closes the loop 15 m wrong.  The shortlist of the
K best separated candidates, every one verified, picks the right frame by its fitness."""
import functools

import numpy as np

import local_map_synth as lms
import loop_icp_cases as licp
import place_loop_cases as plc

host = plc.host
F = np.float32
N, REVISITED, SEED, UP = plc.N, plc.REVISITED, plc.SEED, plc.UP
RADIUS, GAP, H, NOW, LOOP_VARIANCE = plc.RADIUS, plc.GAP, plc.H, plc.NOW, plc.LOOP_VARIANCE
TWIN = (REVISITED + N // 2) % N  # where the room's half turn takes the revisited frame
K, MIN_SEP = 4, 4                # the step's defaults on this case: min_sep = the window's half-width
MAX_FITNESS = 0.3                # historyKeyframeFitnessScore
HEIGHT, EXTRA = 0.15, 900
PIECES = tuple((org, u, (0.0, 0.0, HEIGHT)) for org, u, _ in plc.PIECES)


def scan(seed, pose):
    """place_loop_cases.scan with this module's PIECES and EXTRA"""
    corner, surf, outlier = lms.room_scan(seed, pose, **licp.SMALL)
    rng = np.random.default_rng(seed + 77)
    k = rng.integers(0, len(PIECES), EXTRA)
    a, b = rng.uniform(0, 1, EXTRA), rng.uniform(0, 1, EXTRA)
    org, u, v = (np.array([p[i] for p in PIECES], np.float64)[k] for i in range(3))
    pm = org + a[:, None] * u + b[:, None] * v + rng.normal(0, 0.01, (EXTRA, 3))
    extra = np.concatenate([lms.to_sensor(pm, pose), rng.uniform(0, 100, (EXTRA, 1))], 1).astype(F)
    return corner, np.concatenate([surf, extra]), outlier


@functools.lru_cache(maxsize=None)
def case():
    """(frames [(corner, surf, outlier, stored pose)], true pose of the last frame, its stored pose), as place_loop_cases.case"""
    poses = lms.trajectory(N, seed=SEED)
    true = (poses[REVISITED].astype(np.float64) + plc.TRUE_OFFSET).astype(F)
    wrong = (true.astype(np.float64) + plc.STORED_ERROR).astype(F)
    seen = [poses[i] for i in range(N - 1)] + [true]
    stored = [poses[i] for i in range(N - 1)] + [wrong]
    return [scan(7000 + i, seen[i]) + (stored[i],) for i in range(N)], true, wrong


@functools.lru_cache(maxsize=None)
def host_chain():
    """the chain on the CPU restatement -> dict(row (every candidate's smallest distance), ranks (lins_host_place_topk),
    icp (one result per rank), chosen, final (the poses after the solve with the chosen loop), final_top1 (with rank 0's))"""
    frames, true, wrong = case()
    prm = host.place_params(up_axis=UP)
    D = [host.place_descriptor(*f[:3], params=prm) for f in frames]
    times = np.arange(N, dtype=np.float64)
    r = dict(row=[float(host.place_distance(D[-1], D[i]).min()) for i in range(N - 1)])
    r["ranks"], r["candidates"] = host.place_topk(D[-1], D, times, NOW, GAP, K, MIN_SEP, skip_id=N - 1)
    src = host.submap(frames, [N - 1], 3, 0.0, 1)[0]
    r["icp"], r["pose_from"] = [], []
    for c in r["ranks"]:
        T0 = host.place_guess(wrong, frames[c["id"]][3], c["shift"], UP)
        tgt = host.submap(frames, plc.window(c["id"], N - 1), 3, 0.4, 0)[0]
        r["icp"].append(host.loop_icp_from(src, tgt, T0))
        r["pose_from"].append(host.loop_pose_from(r["icp"][-1]["transform"], wrong))
    r["chosen"] = host.loop_choose([i["converged"] for i in r["icp"]], [i["fitness"] for i in r["icp"]], MAX_FITNESS)
    if r["chosen"] >= 0:
        j = r["chosen"]
        r["final"] = plc.solved(frames, [(N - 1, r["ranks"][j]["id"], r["pose_from"][j], LOOP_VARIANCE)])
    r["final_top1"] = plc.solved(frames, [(N - 1, r["ranks"][0]["id"], r["pose_from"][0], LOOP_VARIANCE)])
    return r
