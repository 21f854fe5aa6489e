"""CPU: the NumPy restatement of BiCGstab (tests/bicg_restate.py) over the CPU oracle's operators, pinned to the reference's own
solver/bicgstab_complex.c (tests/golden/ref_bicg_*, tools/make_golden_bicg.py).

Counts are pinned for the KIND_M operators only: on the indefinite Q operators the count moves with the last bits of the scalar
products (the reference needs 43 iterations where the restatement needs 47).  Every converged case must meet the true-residual bound
(the stopping bound times the fixture's margin = 10 x the reference's largest true-to-recursive ratio) and lie within
2 sqrt(bound) / sigma_min(A) of the reference's solution: both solutions have a residual of at most sqrt(bound)."""
import json
import os

import numpy as np
import pytest

from oracle.nd_restate import cplx
from tests import bicg_restate as br
from tests.util import random_gauge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
S4 = json.load(open(os.path.join(GOLD, "ref_bicg_scalars_4x4.json")))
S8 = json.load(open(os.path.join(GOLD, "ref_bicg_scalars_8x6x4x12.json")))


@pytest.fixture(scope="module")
def fx4():
    return np.load(os.path.join(GOLD, "ref_bicg_4x4.npz")), np.load(os.path.join(GOLD, "ref_mms_4x4.npz"))["gauge"]


def test_fixture_sizes_and_coverage():
    size = sum(os.path.getsize(os.path.join(GOLD, n)) for n in ("ref_bicg_4x4.npz", "ref_bicg_scalars_4x4.json", "ref_bicg_scalars_8x6x4x12.json"))
    assert size < 1 << 20
    c = S4["cases"]
    assert {v["op"] for v in c.values()} == set(br.KIND_M + br.KIND_Q)           # one case per operator id
    assert {v["rel_prec"] for v in c.values()} == {0, 1}
    assert any(v["guess"] for v in c.values()) and c["mtm_plus_sym_cut"]["iters"] == -1
    assert S8["dims"] == [8, 6, 4, 12] and S4["margin"] == S8["margin"]
    ratios = [v["ratio"] for s in (S4, S8) for v in s["cases"].values() if "ratio" in v]
    assert S4["margin"] == 10.0 * max(ratios)
    assert all(v["sigma_min"] > 0 for v in c.values())


def run(S, gauge, name):
    case = S["cases"][name]
    dims = tuple(S["dims"])
    V = int(np.prod(dims))
    orc = br.oracle_for(dims, gauge, S["kappa"], S["c_sw"], case)
    A = br.operator(orc, case["op"])
    Q, P0 = br.case_fields(case, V)
    it, P, hist = br.bicgstab_complex(A, cplx(P0), cplx(Q), case["max_iter"], case["eps_sq"], case["rel_prec"])
    true = float(np.sum(np.abs(cplx(Q) - A(P)) ** 2))
    return case, it, P, hist, true, br.bound_of(case, Q)


@pytest.mark.parametrize("name", sorted(S4["cases"]))
def test_restatement_reproduces_the_4x4_fixture(fx4, name):
    f, gauge = fx4
    case, it, P, hist, true, bound = run(S4, gauge, name)
    if case["iters"] == -1:
        assert it == -1 and len(hist) == case["max_iter"]
        return
    if case["kind"] == "M":
        assert it == case["iters"]
    assert 0 < it <= 10 * case["iters"]
    assert hist[-1] <= bound and true <= bound * S4["margin"], (true, bound)
    dist = np.sqrt(np.sum(np.abs(P - cplx(f[name + "_P"])) ** 2))
    assert dist <= 2.0 * np.sqrt(bound) / case["sigma_min"], (dist, bound, case["sigma_min"])


@pytest.mark.parametrize("name", sorted(S8["cases"]))
def test_restatement_reproduces_the_8x6x4x12_scalars(name):
    gauge = random_gauge(123456, int(np.prod(S8["dims"])))
    case, it, P, hist, true, bound = run(S8, gauge, name)
    if case["iters"] == -1:
        assert it == -1
        return
    if case["kind"] == "M":
        assert it == case["iters"]
    assert 0 < it <= 10 * case["iters"]
    assert hist[-1] <= bound and true <= bound * S8["margin"], (true, bound)
