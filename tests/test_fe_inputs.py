"""The feature-stage cases of tests/fe_cases.py are what they claim, and the CPU statements of the stage agree on them:
fe_cases.model (float64, plain Python, the arrays alone), the product's host restatement (host/frontend.cpp under the package's csrc/ — what
tests/test_gpu_features.py holds frontend_kernel against, bit for bit), the independent checker
(oracle/frontend_oracle.cpp) and the reference's own StateEstimator (oracle/_ref).  Only the cases of fc.TIE_CASES let equal
curvatures decide a pick (asserted for every other case): for those the reference, whose std::sort leaves that order open,
is compared outside the rings where they do (fc.TIE_RINGS) — the cases' docstrings say what was dropped."""
import os

import numpy as np
import pytest

import fe_cases as fc
from test_frontend_oracle import assert_same_features

NAMES = list(fc.CASES)
_MODELS = {}
CLOUDS = ("corner_sharp", "corner_less_sharp", "surf_flat", "surf_less_flat")


def model(name):
    if name not in _MODELS:
        _MODELS[name] = fc.model(fc.case(name))
    return _MODELS[name]


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r

    if not r.available():
        if os.environ.get("LINS_REQUIRE_REF") == "1":
            pytest.fail("LINS_REQUIRE_REF=1 and oracle/_ref/liblins_ref.so is neither built nor buildable here")
        pytest.skip("oracle/_ref/liblins_ref.so not built and the reference's sources are not present")
    r.lib()
    return r


def segmented(host, c):
    return host.segmented_from_arrays(c["cloud"], c["range"], c["col"], c["ground"], c["n"], c["start_ring"], c["end_ring"],
                                      c["orientation"], c["n_outlier"])


def restated(host, name, _cache={}):
    if name not in _cache:
        _cache[name] = host.frontend_extract_segmented(segmented(host, fc.case(name)))
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_case_stays_inside_what_image_projection_emits(name):
    c = fc.case(name)
    n, count = c["n"], 0
    ring_of = np.floor(c["cloud"][:, 3]).astype(int)
    assert n <= fc.CLOUD_MAX and (np.diff(ring_of) >= 0).all()  # ring-major
    for r in range(fc.ROWS):
        k = np.nonzero(ring_of == r)[0]
        assert c["start_ring"][r] == count + 4 and c["end_ring"][r] == count + len(k) - 6
        assert (np.diff(c["col"][k].astype(int)) > 0).all() and (c["col"][k] < fc.COLS).all()
        count += len(k)
    assert count == n
    assert len(np.unique(c["cloud"][:, :3], axis=0)) == n  # a picked point's coordinates say which point it is
    m = model(name)
    assert m["ori_margin"] >= 1e-3  # rad between any orientation test taken and its threshold


@pytest.mark.parametrize("name", NAMES)
def test_claims_hold_in_the_float64_model(name):
    c, m = fc.case(name), model(name)
    cl = c["claims"]
    sec = {(s["ring"], s["j"]): s for s in m["sectors"]}
    every_pick = set(m["less_sharp"]) | set(m["flat"])
    if name not in fc.TIE_CASES:
        assert not any(s["edge_ties"] or s["plane_ties"] for s in m["sectors"])
    for key, want in cl.get("edge_picks", {}).items():
        assert sec[key]["less_sharp"] == want, key
    for key, want in cl.get("flat_picks", {}).items():
        assert sec[key]["flat"] == want, key
    for key, want in cl.get("first_edge", {}).items():
        s = sec[key]
        assert s["less_sharp"][0] == want == s["ep"] and s["sharp"][0] == want
        assert sum(m["curv"][x] > m["curv"][want] for x in s["less_sharp"][1:]) == 19  # all stronger, and more were left
        assert sum(m["curv"][x] > m["curv"][want] for x in s["ecand0"]) >= 20
    for x, want in cl.get("curvature", {}).items():
        assert m["curv"][x] == want
    for key, want in cl.get("n_sharp", {}).items():
        assert len(sec[key]["sharp"]) == want
    for key, want in cl.get("n_less_sharp", {}).items():
        assert len(sec[key]["less_sharp"]) == want
    for key, want in cl.get("n_edge_candidates", {}).items():
        assert len(sec[key]["ecand0"]) >= want and len(set(m["curv"][sec[key]["ecand0"]])) == len(sec[key]["ecand0"])
    assert set(cl.get("picked", [])) <= every_pick
    assert not set(cl.get("not_picked", [])) & every_pick
    assert m["occluded"][cl.get("occluded", [])].all()
    if "occluded_exactly" in cl:
        assert np.nonzero(m["occluded"])[0].tolist() == sorted(cl["occluded_exactly"])
    for r, want in cl.get("live", {}).items():
        assert sum(sec[(r, j)]["live"] for j in range(6)) == want, r
    for r, want in cl.get("kept", {}).items():
        assert len(m["kept"][r]) == want, r
    for key, want in cl.get("m", {}).items():
        assert sec[key]["live"] and sec[key]["ep"] - sec[key]["sp"] == want, key
    for key, want in cl.get("n_ec0", {}).items():
        assert len(sec[key]["ecand0"]) == want == sec[key]["n_ec"], key  # (ep is no candidate there: nothing dropped)
    for key, want in cl.get("path", {}).items():
        assert sec[key]["path"] == want, key
    if "tie_picks" in cl:
        across = lambda ties: sum(len(t["lanes"]) >= 2 for t in ties)  # decided among equal keys held by different lanes
        for path in ("lane", "mask"):
            ss = [s for s in m["sectors"] if s.get("path") == path]
            assert sum(across(s["edge_ties"]) for s in ss) >= cl["tie_picks"][path], path
        assert sum(across(s["plane_ties"]) for s in m["sectors"]) >= cl["tie_picks"]["plane"]
        blocks = lambda ties: max([len(t["blocks"]) for s in m["sectors"] for t in s[ties]] or [0])
        assert blocks("edge_ties") >= 2 and blocks("plane_ties") >= 2  # twins in different 64-element blocks too
    if "kept_includes" in cl:
        kept = set(np.concatenate(m["kept"]).tolist())
        assert set(cl["kept_includes"]) <= kept and not set(cl["kept_excludes"]) & kept
        assert set(m["flat"].tolist()) <= kept and not set(m["less_sharp"].tolist()) & kept
    for r, (narrow, packs) in cl.get("voxel_keys", {}).items():
        v = m["voxels"][r]
        assert (v["narrow"], v["packs"]) == (narrow, packs), r
    for r, want in cl.get("volume", {}).items():
        v = m["voxels"][r]
        assert v["volume"] == want and (v["index"].max() >= 2 ** 21) == (not v["narrow"])
        assert np.argmax(v["index"]) < np.argmin(v["index"])  # the far corner comes first: the sort moves it
    for r in cl.get("one_point_per_voxel", []):
        assert (m["voxels"][r]["counts"] == 1).all()
    if "rounding_decides" in cl:
        v = m["voxels"][cl["rounding_decides"]]
        assert v["rounding_decides"] >= 10 and (v["ijk"][:, 0] < 0).sum() >= 40 and (v["counts"] > 1).any()
    if "chunks" in cl:
        assert sum((len(k) + 63) // 64 for k in m["kept"]) == cl["chunks"]
        group = max(1, (cl["chunks"] + 31) // 32)  # chunks a wave takes in a row
        assert group == (2 if cl["placed"] else 1)
        ch0 = np.cumsum([0] + [(len(k) + 63) // 64 for k in m["kept"]])
        for r, want in cl["mult"].items():
            assert m["voxels"][r]["counts"].tolist() == want, r
            assert (np.diff(m["voxels"][r]["index"]) <= 0).all()  # the points come in descending voxel order
        inside = lambda r, b: (ch0[r] + b // 64) % group != 0  # the border at sorted position b of ring r lies inside a pair
        runs = lambda r: np.concatenate([[0], np.cumsum(m["voxels"][r]["counts"])])
        for name_, (r, a, b) in cl["placed"].items():
            rs = runs(r)
            k = int(np.searchsorted(rs, a))
            assert rs[k] == a and rs[k + 1] == b, name_  # it is one run
            crossed = [x for x in range(64, len(m["kept"][r]), 64) if a < x < b]
            if name_ == "ends_on_lane_63":
                assert b % 64 == 0 and b < len(m["kept"][r]) and not crossed
            elif name_ == "last_reaches_lane_63":
                assert b == len(m["kept"][r]) and b % 64 == 0 and len(m["kept"][r + 1]) > 0 and (ch0[r + 1]) % group != 0
            elif name_ in ("carried", "carried_odd_ring"):
                assert len(crossed) == 1 and inside(r, crossed[0])
            elif name_ == "alone":
                assert len(crossed) == 1 and not inside(r, crossed[0])
            elif name_ == "both":
                assert len(crossed) == 2 and inside(r, crossed[0]) and not inside(r, crossed[1])
            elif name_ == "alone_twice":
                assert len(crossed) == 2 and not inside(r, crossed[0]) and inside(r, crossed[1])
            else:
                raise AssertionError(name_)
    if cl.get("flip_seen"):
        f = m["flip"]
        assert f in m["kept"][0] and abs(m["second"][f] - m["first"][f]) > 6  # rad: the other half's correction differs
        v = m["voxels"][0]
        assert (v["counts"] == 1).all()  # its tag stands alone in the less-flat cloud


def test_the_half_turn_cases_take_every_branch_of_undistortPcl():
    """0 / 3: no correction in the first / second half; 1, 2: + 2 pi, - 2 pi in the first; 4, 5: in the second.  The flip
    lies inside ring 0, at point 0, or nowhere (n).  That the flip point itself is corrected as first half is decided by
    half_turns_long_turn (claim flip_seen)."""
    seen = set()
    for name in NAMES:
        m = model(name)
        seen |= set(np.unique(m["branch"]).tolist())
    assert seen == {0, 1, 2, 3, 4, 5}
    assert model("half_turns_flip_at_0")["flip"] == 0 and model("centroid_carry")["flip"] == fc.case("centroid_carry")["n"]
    assert 0 < model("half_turns_pi")["flip"] < 300 and 0 < model("half_turns_minus_pi")["flip"] < 300


def assert_restatement_is_the_model(c, m, f):
    cloud = c["cloud"]
    for k, idx in (("corner_sharp", m["sharp"]), ("corner_less_sharp", m["less_sharp"]), ("surf_flat", m["flat"])):
        assert f[k].shape == (len(idx), 4), k
        assert np.array_equal(f[k][:, :3], cloud[idx][:, :3]), k
        assert (np.abs(f[k][:, 3] - m["tag"][idx]) <= 2.5e-7 * np.maximum(1.0, m["tag"][idx])).all(), k
    cent = [v["centroids"] for v in m["voxels"] if v is not None]
    cent = np.concatenate(cent) if cent else np.zeros((0, 3), np.float32)
    assert f["surf_less_flat"].shape == (len(cent), 4)
    assert np.array_equal(f["surf_less_flat"][:, :3], cent)
    tags = []
    for kk, v in zip(m["kept"], m["voxels"]):
        if v is not None:
            t = m["tag"][kk][v["order"]]
            tags += [t[a:a + k].mean() for a, k in zip(np.cumsum(v["counts"]) - v["counts"], v["counts"])]
    tags = np.array(tags)
    k = np.concatenate([v["counts"] for v in m["voxels"] if v is not None]) if len(tags) else np.zeros(0)
    # (the restatement adds a voxel's k tags in f32 one after the other: k roundings of 2^-24 on top of the tag's own bar)
    assert (np.abs(f["surf_less_flat"][:, 3] - tags) <= (2.5e-7 + k * 2.0 ** -24) * np.maximum(1.0, tags)).all()


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_equals_the_model(host, name):
    """picks by index, centroids bit for bit, tags to the f32 rounding of a tag (the model's arctangent is numpy's)"""
    assert_restatement_is_the_model(fc.case(name), model(name), restated(host, name))


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_equals_the_independent_checker(host, oracle, name):
    assert_same_features(oracle.fe_features(fc.case(name)), restated(host, name))


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_and_checker_equal_the_references_stage(pkg, host, oracle, ref, name):
    """the bars of tests/test_gpu_ref.py: the same picks in the same order (no tie to excuse: bit for bit), the less-flat
    cloud within 4e-6 — on every ring outside fc.TIE_RINGS.  `ties` besides: as many picks, equally curved, per position."""
    c = fc.case(name)
    fr = ref.extract_features(pkg.default_params(), c)
    tied = fc.TIE_RINGS.get(name, ())
    ring_of = lambda x: np.floor(x[:, 3] + 0.5 * (x[:, 3] < 0)).astype(int)
    clear = lambda x: x[~np.isin(ring_of(x), tied)]  # what lies in rings where no tie decides anything
    where = {c["cloud"][i, :3].tobytes(): i for i in range(c["n"])}
    curv = model(name)["curv"]
    for f in (restated(host, name), oracle.fe_features(c)):
        for k in CLOUDS[:3]:
            a, b = clear(fr[k]), clear(f[k])
            assert a.shape == b.shape and np.array_equal(a[:, :3].view(np.int32), b[:, :3].view(np.int32)), k
            if name == "ties":  # every sector keeps all its picks whichever twin is taken: as many, equally curved
                assert fr[k].shape == f[k].shape, k
                ia, ib = [[where[np.ascontiguousarray(p[:3]).tobytes()] for p in x[k]] for x in (fr, f)]
                assert np.array_equal(curv[ia], curv[ib]), k
        a, b = clear(fr["surf_less_flat"]), clear(f["surf_less_flat"])
        assert a.shape == b.shape and np.abs(a - b).max(initial=0) <= 4e-6
