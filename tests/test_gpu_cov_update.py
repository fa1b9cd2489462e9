"""The covariance update of the iterated update (SE:594-598) ALONE on the device, on built priors (tests/cov_cases.py): every
case through the program of every update path — joseph_epilogue as instantiated in the three LDS kernel families ("lds",
"lds1", "mr") and ieskf_joseph_kernel ("joseph": the any-size path), lins_debug_cov_update, one launch per path — against
the long-double textbook form in the posterior's own scale: e <= 16 eps / shrink + 16 eps per case, exact symmetry, the
smallest eigenvalue in the reference's correlation scaling, and the exact claims (uncorrelated block, A = 0, zero-variance
rows, diverged pass-through) bit for bit; the same bits wherever a case stands in a batch; the epilogue against the
stand-alone kernel.  tests/test_cov_inputs.py asserts what the cases claim and runs the oracle's joseph_reduced through
the same checks on the CPU.  (The host library has no covariance update of its own: lins_host_perform_ieskf runs the
device's.)

Measured on an MI355X (profiles/cov_update_gpu_tests.txt): the three epilogues e <= 1.57 (eps /
shrink + eps), worst at rank/3 — 1.3e-6 at shrink 1e-10; the stand-alone kernel e <= 1.7e-13 whatever the shrink; the
epilogue against the stand-alone kernel up to 1.9 eps / shrink.  An epilogue whose - (C Y) P_S: term is dropped for rows
>= 9 fails six of these tests; one that builds M from Y instead of Y^T passes all of them, rightly: with a symmetric prior
the symmetrised result is the same matrix."""
import time

import numpy as np
import pytest

import cov_cases as cc

pytestmark = pytest.mark.gpu
PATHS = cc.PATHS_DEVICE


@pytest.fixture(scope="module")
def ctx(pkg, ieskf):
    t0 = time.perf_counter()
    c = ieskf.IeskfContext(pkg.default_params(), max_batch=1, max_targets=1024)
    yield c
    c.close()
    print(f"\ntests/test_gpu_cov_update.py: {time.perf_counter() - t0:.2f} s from context creation to the last test")


def run(ctx, path, cs):
    """the cases of one r2 in one launch"""
    P, sums, div = cc.batch(cs)
    assert len({c["r2"] for c in cs}) == 1
    return ctx.debug_cov_update(path, P, sums, cs[0]["r2"], div)


@pytest.fixture(scope="module")
def outputs(ctx):
    """every case on every path: one launch per path and r2, the cases in their order"""
    out = {}
    for path in PATHS:
        for r2 in sorted({c["r2"] for c in cc.cases()}):
            cs = [c for c in cc.cases() if c["r2"] == r2]
            for c, got in zip(cs, run(ctx, path, cs)):
                out[path, c["name"]] = got
    return out


@pytest.mark.parametrize("path", PATHS)
def test_every_case_within_its_bar(outputs, path):
    worst = (0.0, "")
    for c in cc.cases():
        e = cc.check_output(c, outputs[path, c["name"]], path)
        if e is not None:
            print(f"{path:6s} {c['name']:32s} shrink {c['shrink']:.3e}  e = {e:.3e} = {e / (cc.EPS / c['shrink'] + cc.EPS):6.3f} (eps / shrink + eps)  bar {c['bar']:.3e}")
            worst = max(worst, (e / (cc.EPS / c["shrink"] + cc.EPS), c["name"]))
    print(f"{path}: worst constant c of e = c (eps / shrink + eps): {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("path", PATHS[:3])
def test_epilogue_against_the_stand_alone_kernel(outputs, path):
    """the rank-6 form against the product form, in the posterior's scale: both are within the bar of the reference, so
    within twice the bar of each other — the difference is of the rank-6 form's order, eps / shrink, and is written down"""
    worst = (0.0, "")
    for c in cc.cases():
        if c["diverged"]:
            continue
        a, b = outputs[path, c["name"]], outputs["joseph", c["name"]]
        d = cc.diff(a, b, c["ref"])
        rel = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"{path:6s} {c['name']:32s} epilogue - stand-alone: e = {d:.3e} = {d * c['shrink'] / cc.EPS:6.3f} eps / shrink;  max|dP| / max|P| = {rel:.2e}")
        assert d <= 2 * c["bar"], (c["name"], d)
        worst = max(worst, (d * c["shrink"] / cc.EPS, c["name"]))
    print(f"{path} epilogue against the stand-alone kernel: worst {worst[0]:.3f} eps / shrink at {worst[1]}")


@pytest.mark.parametrize("path", PATHS)
def test_bits_do_not_depend_on_the_batch(ctx, outputs, path):
    """one case at positions 0, 1 and n - 1 of batches of 1, 3 and 65, diverged and live cases around it"""
    c = cc.by_name("ladder/prior/1e-06")
    want = outputs[path, c["name"]].tobytes()
    fill = [f for f in cc.cases() if f["r2"] == c["r2"] and f is not c]
    for n in (1, 3, 65):
        for pos in sorted({0, min(1, n - 1), n - 1}):
            cs = [fill[(3 * k + pos) % len(fill)] for k in range(n)]
            cs[pos] = c
            got = run(ctx, path, cs)
            assert got[pos].tobytes() == want, (path, n, pos)
            for k in (0, n // 2, n - 1):  # and the cases around it are their own
                assert got[k].tobytes() == outputs[path, cs[k]["name"]].tobytes(), (path, n, pos, k)


def test_bad_arguments_are_refused(ctx, ieskf):
    c = cc.by_name("rank/0")
    with pytest.raises(ValueError):
        ctx.debug_cov_update("mr", c["P"][None, :17], c["sums"][None], c["r2"])
    with pytest.raises(ValueError):
        ctx.debug_cov_update("nowhere", c["P"][None], c["sums"][None], c["r2"])
