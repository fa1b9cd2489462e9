"""What the GPU tests of the loop-closure ICP rest on, asserted on the CPU (tests/loop_icp_cases.py holds the problems).

The stop round must not hang on the last bits: on every whole-loop problem, at every round of the restatement's trace,
  * |t_delta|^2, |mse - mse_prev| and |mse - mse_prev| / mse_prev are outside [1/2, 2] x their thresholds;
  * the rotation quantity 0.5 (trace R_delta - 1) is at least 1e-9 away from its threshold 0.99999.
The rotation quantity cannot be held to the [1/2, 2] window: 0.99999 x [1/2, 2] contains the quantity of EVERY rotation
below 60 degrees, so no run that converges is ever outside it; and its complement 1 - q crosses 1e-5 x [1/2, 2] on every
one of 150 seeds scanned, because theta_delta shrinks by less than a factor 2 a round.  What keeps the device's rounding
from moving the stop round is distance from the threshold in units of the possible difference: the device is held to
loop_icp_cases.BAR_T = 2.5e-14 in every entry of T and delta, so a quantity 1e-9 away — four decades more than the
trace of a delta within the bar can move — decides the same way on both sides.  The seeds in loop_icp_cases were CHOSEN
so that all of this holds (about half of the seeds scanned pass)."""
import numpy as np

import loop_icp_cases as cases
import loop_icp_np as lnp


def test_no_stop_quantity_of_any_round_is_near_its_threshold(host):
    th = cases.THRESHOLDS
    for k, (s, t) in enumerate(cases.all_whole_loop_clouds()):
        rounds, res = host.loop_icp_trace(s, t)
        assert res["converged"] == 1 and 3 <= len(rounds) <= 40, (k, len(rounds))
        assert res["fitness"] <= 0.3  # (the caller's acceptance, LM:1140-1141)
        for r, rd in enumerate(rounds):
            q = rd["stop"]
            assert abs(q[0] - th["rotation"]) >= 1e-9, (k, r, q)
            for v, name in ((q[1], "translation"), (q[2], "abs_mse"), (q[3], "rel_mse")):
                assert not (0.5 * th[name] <= v <= 2 * th[name]), (k, r, name, v)


def test_tie_and_edge_fixtures_contain_what_they_claim():
    by = {n: (s, t) for n, s, t in cases.search_cases()}
    # ties: the two smallest d of a query are equal, at differing indices
    for name, at_least in (("lattice", 128), ("duplicates", 64)):
        s, t = by[name]
        d = ((s[:, None, :3] - t[None, :, :3]) ** 2).astype(np.float32)
        d = ((d[..., 0] + d[..., 1]) + d[..., 2]).astype(np.float32)
        two = np.sort(d, 1)[:, :2]
        assert (two[:, 0] == two[:, 1]).sum() >= at_least, name
    # queries outside the box by one and by three cells, and 99.9 m away (inside the cap of 100 m)
    s, t = by["outside"]
    lo, hi = np.floor(t[:, :3].min(0)), np.floor(t[:, :3].max(0))
    cells_out = np.maximum(np.maximum(lo - np.floor(s[:, :3]), np.floor(s[:, :3]) - hi), 0).max(1)
    assert set(cells_out[:6].astype(int)) == {1, 3} and cells_out[6] >= 90
    idx, d, _ = lnp.correspondences(s, t, np.eye(4), 100.0)
    assert idx[6] >= 0 and 94.0 ** 2 < d[6] <= 100.0 ** 2
    # a query beyond 100 m: no correspondence under the cap, one without it
    s, t = cases.beyond_cap_case()
    assert lnp.correspondences(s, t, np.eye(4), 100.0)[0].tolist()[0] == -1 and lnp.correspondences(s, t, np.eye(4), 0.0)[0][0] >= 0
    # boxes one cell thick
    for a in range(3):
        t = by[f"slab{a}"][1]
        assert np.ptp(np.floor(t[:, a])) == 0 and np.ptp(np.floor(t[:, (a + 1) % 3])) >= 5
    assert [len(by[f"ng={n}"][1]) for n in (0, 1, 5, 511, 512, 513)] == [0, 1, 5, 511, 512, 513]


def test_the_archive_case_is_the_references_two_compositions():
    frames, specs, wrong, true = cases.archive_case()
    s, t = cases.archive_clouds()
    assert len(frames) == 12 and specs[0]["flags"] == 1 and specs[0]["leaf"] == 0.0 and specs[1]["leaf"] == np.float32(0.4) or specs[1]["leaf"] == 0.4
    assert len(s) == len(frames[11][0]) + len(frames[11][1]) - 7 and len(s) % 32 != 0 and len(t) > 2000
    assert np.allclose(wrong.astype(np.float64) - true, lnp.ERR, atol=1e-6)
