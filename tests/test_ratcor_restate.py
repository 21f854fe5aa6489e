"""CPU: tests/ratcor_restate.py (the correction monomials restated in NumPy over the CPU oracle) pinned to the reference's own outputs
(tests/golden/ref_ratcor_*, tools/make_golden_ratcor.py).

The deviation of the restatement from the reference is MEASURED per quantity: the generator stored it as `restate_vs_ref` (fields relative
to their largest element, scalars relative to their value), this test recomputes it, prints it and asserts that it has not grown (twice the
stored value or 16 units in the last place, whichever is larger).  Z phi is what is left of Q^2 (A R)^2 phi after phi has been taken
away, seven to nine digits below it, and the later deltas of a series are squares of such remainders: their deviations are far above
rounding, which is why the GPU tests take their bounds from these numbers (8 x, never below tests.util.TOL: ratcor_restate.gpu_bound)
and not from a fixed tolerance.  The counts -- applications of Z, solver iterations -- must be the reference's exactly."""
import json
import os

import numpy as np
import pytest

from oracle.nd_restate import cplx
from tests import ratcor_restate as rr
from tests.util import random_gauge, random_spinor

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = 2.0 ** -52


def _grown(now, stored):
    return now > max(2.0 * stored, 16 * ULP)


@pytest.fixture(scope="module", params=["4x4", "8x8"])
def case(request):
    from oracle.oraclebind import Oracle
    tag = request.param
    s = json.load(open(os.path.join(GOLD, "ref_ratcor_scalars_%s.json" % tag)))
    orc = Oracle(s["T"], s["L"], s["L"], s["L"], kappa=s["kappa"], mu=0.0, threads=8)
    if tag == "4x4":
        arrs = np.load(os.path.join(GOLD, "ref_ratcor_4x4.npz"))
        base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
        orc.set_gauge(base["gauge"])
        eta = (cplx(base["k_s"]), cplx(base["k_c"]))
    else:
        arrs = None
        orc.set_gauge(random_gauge(s["gauge_seed"], orc.VPR))
        eta = tuple(cplx(random_spinor(k, orc.Vh)) for k in s["eta_seeds"])
    return tag, s, orc, eta, arrs


def test_fixture_is_what_the_generator_promises(case):
    tag, s, orc, eta, arrs = case
    assert sorted(s["types"]) == sorted(rr.TYPES)
    for name, t in s["types"].items():
        f = t["fit"]
        assert f["np"] == 8 and len(f["mu"]) == len(f["rmu"]) == 8 and f["A"] > 0
        assert 2 <= f["heatbath"]["napp"] <= 5 and 2 <= f["acc"]["napp"] <= 5           # the swap is exercised, the cap of six is not near
        assert f["heatbath"]["deltas"][-1] < f["accprec"] <= f["heatbath"]["deltas"][-2]
        assert f["acc"]["deltas"][-1] < f["accprec"] <= f["acc"]["deltas"][-2]
        lo, hi = f["interval"]
        x = np.geomspace(lo, hi, 2001)
        r = f["A"] * (1.0 + sum(c / (x + m * m) for c, m in zip(f["rmu"], f["mu"])))
        assert np.abs(np.sqrt(x) * r - 1.0).max() <= f["fit_error"] * (1 + 1e-9)       # the recorded coefficients are the recorded fit
        assert abs(f["acc"]["dH"]) < 1e-9 * f["heatbath"]["energy0"]                    # the correction does its job: dH is rounding


# the doublet in NumPy at 8^4 takes a minute per type: its stored deviations are the generator's, re-measured here at 4^4 only
RESTATED = {"4x4": rr.TYPES, "8x8": ("ratcor", "cloverratcor")}


def test_restatement_against_the_reference(case):
    for name in RESTATED[case[0]]:
        _restatement_against_the_reference(case, name)


def _restatement_against_the_reference(case, name):
    tag, s, orc, eta, arrs = case
    t = s["types"][name]
    dev, counts = rr.deviations(rr.RatCor(orc, name, s), t["nd"], t, eta[:2 if t["nd"] else 1], arrs, name)
    f = t["fit"]
    assert counts == {"arb_iters": t["arb"]["iters"], "fit_iters": f["iters"], "heatbath_napp": f["heatbath"]["napp"],
                      "heatbath_iters": f["heatbath"]["iters"], "acc_napp": f["acc"]["napp"], "acc_iters": f["acc"]["iters"]}
    stored = t["restate_vs_ref"]
    print("%s %s restatement vs reference: %s" % (tag, name, dev))
    assert sorted(dev) == sorted(stored)
    for k, v in dev.items():
        if isinstance(v, list):
            assert len(v) == len(stored[k]) and not any(_grown(a, b) for a, b in zip(v, stored[k])), (k, v, stored[k])
        else:
            assert not _grown(v, stored[k]), (k, v, stored[k])
    # what rounding alone explains stays at rounding: one application of Z with coefficients that leave Z phi of the size of phi
    assert dev["arb_delta"] < 1e-14 and dev["energy0"] < 1e-14 and dev["energy1"] < 1e-14
    if arrs is not None:
        assert dev["arb_Z"] < 1e-13 and dev["pf"] < 1e-13 and dev["w"] < 1e-13
