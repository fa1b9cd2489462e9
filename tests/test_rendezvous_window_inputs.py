"""The fairness of the window fixture (tests/rendezvous_window_cases.py), on the CPU restatement alone: what
tests/test_gpu_rendezvous_window.py expects of the device must be there to be found.  These are conditions on the
FIXTURE; if one fails the fixture changes, not the bar.  Targets (0, 1, 2), M = 8, K = 4, the default bars (1 m, 5 degrees).
  - slot 3's latest frame ALONE is accepted: the lone-frame chain says FOUND into a map it never saw (measured: fitness
    0.0658 into slot 1, 0.0674 into slot 0) — the failure the window removes;
  - slot 3 over a window of 5: exactly the hypotheses of frames 9 and 11 are admissible, and every pair of them into the
    same slot lies beyond TWICE max_translation (measured: >= 2.99 m, <= 0.23 degrees), so no star can hold both;
  - slot 1 over a window of 5 (frames 11 .. 7): rank 0 of every frame is its true counterpart in slot 0 (fitness 0.059 ..
    0.097); the five agree pairwise within HALF of both bars (measured: <= 0.057 m, <= 0.27 degrees); every other rank has
    fitness >= 1.27; the support is 5, the winner frame 7 (the smallest fitness), and the winner's X puts its frame's origin
    within place_loop_cases.bound()[0] of the truth (measured: 0.043 m);
  - slot 2: nothing is admissible."""
import numpy as np

import place_loop_cases as plc
import rendezvous_cases as rc
import rendezvous_window_cases as rwc

N = rwc.N


def test_slot_3_is_built_as_described():
    fr = rwc.slots()
    assert sorted(fr) == [0, 1, 2, 3] and all(len(fr[s]) == N for s in fr)
    for s in (0, 1, 2):
        assert fr[s] is rc.slots()[0][s]
    g9, g11 = rwc.G_alias(9), rwc.G_alias(11)
    assert abs(np.linalg.norm(g9[:3, 3] - g11[:3, 3]) - 3.0) < 1e-12
    for i in (9, 11):  # the stored pose composed with G_i is where the scan was taken
        true = rc.matrix(fr[3][i][3])
        assert np.abs(rwc.G_alias(i) @ true - rc.matrix((rwc.lms.trajectory(N, seed=plc.SEED)[rwc.ALIAS[i]].astype(np.float64) + rwc.ALIAS_OFFSET).astype(np.float32))).max() < 2e-5


def test_slot_3s_latest_frame_alone_is_accepted():
    hs = rwc.host_frame_chain(3, N - 1)
    ok = [(h["cand"]["slot"], h["cand"]["id"], h["icp"]["fitness"]) for h in hs if h["admissible"]]
    print("slot 3, frame 11 alone:", [(h["cand"]["slot"], h["cand"]["id"], h["icp"]["converged"], h["icp"]["fitness"]) for h in hs])
    assert len(ok) >= 1 and all(f <= 0.3 for _, _, f in ok)
    assert rc.host.loop_choose([h["icp"]["converged"] for h in hs], [h["icp"]["fitness"] for h in hs], 0.3) >= 0  # lins_rendezvous_step: FOUND
    # ... and a window of one with min_support 1 says the same
    one = rwc.host_window_chain(3, 1)["verdict"]
    assert one["winner"] >= 0 and one["support"] == 1


def test_slot_3_over_a_window_contradicts_itself():
    r = rwc.host_window_chain(3, 5)
    adm = [h for h in r["hyp"] if h["admissible"]]
    print("slot 3, window 5:", [(h["frame"], h["cand"]["slot"], h["cand"]["id"], h["admissible"], round(h["icp"]["fitness"], 4)) for h in r["hyp"]])
    assert {h["frame"] for h in adm} == {9, 11}  # (the aliasing frames and no other)
    p = {f: np.asarray(rwc.slots()[3][f][3][:3], np.float64) for f in (9, 11)}
    pairs = [(a, b) for a in adm for b in adm if a["frame"] == 9 and b["frame"] == 11 and a["cand"]["slot"] == b["cand"]["slot"]]
    assert pairs
    for a, b in pairs:
        d, ang = rwc.apart(a["icp"]["transform"], p[9], b["icp"]["transform"], p[11]), rwc.angle_deg(a["icp"]["transform"], b["icp"]["transform"])
        print("  frames 9 / 11 into slot %d: %.3f m, %.3f degrees apart" % (a["cand"]["slot"], d, ang))
        assert d > 2.0 * rwc.MAX_T
    assert r["verdict"]["support"] == 1 and r["verdict"]["n_admissible"] == len(adm)


def test_slot_1_over_a_window_agrees_on_G():
    r = rwc.host_window_chain(1, 5)
    assert r["frames"] == [11, 10, 9, 8, 7]
    first = [h for h in r["hyp"] if h["rank"] == 0]
    rest = [h for h in r["hyp"] if h["rank"] > 0]
    print("slot 1, window 5, rank 0:", [(h["frame"], h["cand"]["slot"], h["cand"]["id"], round(h["icp"]["fitness"], 4)) for h in first])
    assert [(h["cand"]["slot"], h["cand"]["id"]) for h in first] == [(0, f) for f in r["frames"]]
    assert all(h["admissible"] and h["icp"]["fitness"] <= 0.3 for h in first)
    assert all(not h["admissible"] and h["icp"]["fitness"] > 1.0 for h in rest), [h["icp"]["fitness"] for h in rest]
    fr = rwc.slots()[1]
    worst_d = worst_a = 0.0
    for a in first:
        for b in first:
            if a["frame"] < b["frame"]:
                worst_d = max(worst_d, rwc.apart(a["icp"]["transform"], fr[a["frame"]][3][:3], b["icp"]["transform"], fr[b["frame"]][3][:3]))
                worst_a = max(worst_a, rwc.angle_deg(a["icp"]["transform"], b["icp"]["transform"]))
    print("  the five pairwise: <= %.3f m, <= %.3f degrees" % (worst_d, worst_a))
    assert worst_d <= 0.5 * rwc.MAX_T and worst_a <= 0.5 * np.degrees(np.arccos(rwc.MIN_COS))
    v = r["verdict"]
    w = r["hyp"][v["winner"]]
    assert v["support"] == 5 and v["n_admissible"] == 5 and [r["hyp"][i]["frame"] for i in v["members"]] == r["frames"]
    assert w["icp"]["fitness"] == min(h["icp"]["fitness"] for h in first) and w["frame"] == 7
    e = rc.origin_error(w["icp"]["transform"], w["frame"])
    print("  the winner: frame %d, origin error %.4f m (bound %.4f m)" % (w["frame"], e, plc.bound()[0]))
    assert e <= plc.bound()[0]


def test_slot_2_has_nothing_admissible():
    r = rwc.host_window_chain(2, 5)
    assert r["hyp"] and not any(h["admissible"] for h in r["hyp"])
    assert r["verdict"] == dict(winner=-1, support=0, n_admissible=0, members=[])
