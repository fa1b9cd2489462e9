"""The fixture of a rendezvous over a window (tests/test_rendezvous_window_inputs.py on the CPU,
tests/test_gpu_rendezvous_window.py on the device; not a test): the three robots of tests/rendezvous_cases.py and a fourth.
  slot 3   maps another building, as slot 2 does — twelve small synthetic places — but two of its frames, 9 and 11, happen
           to LOOK like the room: they are scans of the room (taken near slot 0's frames 3 and 8), stored at poses that
           claim map frames three metres apart: frame i's stored pose is G_i^-1 composed with where the scan was truly
           taken, G_9 a yaw of -40 degrees with t = (-4, 2, 0), G_11 the same yaw with t = (-1, 2, 0).
A single frame cannot tell slot 3's alias from slot 1's meeting: each aligns under the fitness bar.  Over a window slot 1's
frames agree on X = G of tests/rendezvous_cases.py and slot 3's two frames contradict each other.

host_window_chain() is the explicit chain on the CPU restatement for the last `window` frames of a slot."""
import functools

import numpy as np

import local_map_synth as lms
import place_cases as pc
import place_loop_cases as plc
import rendezvous_cases as rc
import team_cases as tc

host, team = rc.host, rc.team
F = np.float32
N, UP, H, GAP, NOW, M, K = rc.N, rc.UP, rc.H, rc.GAP, rc.NOW, rc.M, rc.K
ALIAS = {9: 3, 11: 8}  # slot 3's frame -> the frame of slot 0's trajectory it was taken near
ALIAS_OFFSET = np.array([0.3, 0.2, 0.0, 0.0, 0.0, 0.3])
ALIAS_YAW, ALIAS_T = np.deg2rad(-40.0), {9: np.array([-4.0, 2.0, 0.0]), 11: np.array([-1.0, 2.0, 0.0])}
MAX_T, MIN_COS = 1.0, 0.99619469809174555  # lins_rendezvous_consensus_default_params


def G_alias(i):
    T = np.eye(4)
    c, s = np.cos(ALIAS_YAW), np.sin(ALIAS_YAW)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = ALIAS_T[i]
    return T


@functools.lru_cache(maxsize=None)
def slots():
    """slot -> [(corner, surf, outlier, stored pose)] for the four slots"""
    fr = dict(rc.slots()[0])
    rng = np.random.default_rng(19)
    d = [pc.frame(pc.place(4000 + i, n=400, up=UP)) + (np.concatenate([rng.uniform(-5, 5, 3), rng.uniform(-0.1, 0.1, 3)]).astype(F),) for i in range(N)]
    pa = lms.trajectory(N, seed=plc.SEED)
    for i, j in ALIAS.items():
        true = (pa[j].astype(np.float64) + ALIAS_OFFSET).astype(F)
        d[i] = plc.scan(9000 + i, true) + (rc.compose(np.linalg.inv(G_alias(i)), true),)
    fr[3] = d
    return fr


@functools.lru_cache(maxsize=None)
def descs():
    names = dict(rc.descs())
    prm = host.place_params(up_axis=UP)
    names[3] = [tc.register(("rendezvous window", 3, i), host.place_descriptor(*f[:3], params=prm)) for i, f in enumerate(slots()[3])]
    return names


def queries(window, stride=1, latest=N - 1):
    return [latest - j * stride for j in range(window) if latest - j * stride >= 0]


def angle_deg(Xa, Xb):
    """the rotation between two transforms"""
    c = (np.trace(np.asarray(Xa)[:3, :3].T @ np.asarray(Xb)[:3, :3]) - 1.0) / 2.0
    return float(np.degrees(np.arccos(min(1.0, max(-1.0, c)))))


def apart(Xa, pa, Xb, pb):
    """how far two transforms put the places the robot stood apart: the larger of |Xa p - Xb p| over the two positions"""
    return max(float(np.linalg.norm((np.asarray(Xa) @ np.append(p, 1.0) - np.asarray(Xb) @ np.append(p, 1.0))[:3]))
               for p in (np.asarray(pa, np.float64), np.asarray(pb, np.float64)))


@functools.lru_cache(maxsize=None)
def host_frame_chain(slot, frame, which=(0, 1, 2), shortlist=M, k=K, max_fitness=0.3):
    """detect, drop, assemble and align for ONE query frame on the CPU restatement -> [dict(cand, icp, admissible)], the ranks
    inside the asking slot dropped"""
    fr, names = slots(), descs()
    tg = [(s, [tc._DESCS[n] for n in names[s]], np.arange(N, dtype=np.float64)) for s in which]
    ranks = team.host_topk(tc._DESCS[names[slot][frame]], slot, frame, NOW, GAP, tg, shortlist=shortlist, k=k, min_sep=H)
    src = host.submap(fr[slot], [frame], 3, 0.0, 1)[0]
    out = []
    for x in ranks:
        if x["slot"] == slot:
            continue
        tgt = host.submap(fr[x["slot"]], plc.window(x["id"], N - 1), 3, 0.4, 0)[0]
        icp = host.loop_icp_from(src, tgt, team.host_guess(fr[slot][frame][3], fr[x["slot"]][x["id"]][3], x["shift"], UP))
        out.append(dict(cand=x, icp=icp, admissible=int(host.loop_accept(icp["converged"], icp["fitness"], max_fitness) and np.isfinite(icp["fitness"]))))
    return out


def table_of(slot, per_query):
    """[(query j, frame, [dict(cand, icp, admissible)])] -> the consensus table, in (query, rank) order"""
    fr = slots()
    return [dict(X=h["icp"]["transform"] if h["admissible"] else np.zeros((4, 4)), p=np.asarray(fr[slot][frame][3][:3], np.float64),
                 fitness=h["icp"]["fitness"] if h["admissible"] else 0.0, query=j, rank=r, target_slot=h["cand"]["slot"], admissible=h["admissible"])
            for j, frame, hs in per_query for r, h in enumerate(hs)]


@functools.lru_cache(maxsize=None)
def host_window_chain(slot, window=5, which=(0, 1, 2)):
    """the explicit chain for the last `window` frames of `slot` on the CPU restatement -> dict(frames, hyp (flat, each with
    query, frame, rank, cand, icp, admissible), table, verdict (host.rendezvous_consensus))"""
    per = [(j, f, host_frame_chain(slot, f, which)) for j, f in enumerate(queries(window))]
    flat = [dict(h, query=j, frame=f, rank=r) for j, f, hs in per for r, h in enumerate(hs)]
    tab = table_of(slot, per)
    return dict(frames=[f for _, f, _ in per], hyp=flat, table=tab, verdict=host.rendezvous_consensus(tab, max_translation=MAX_T, min_cos_rotation=MIN_COS))
