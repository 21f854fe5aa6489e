"""CPU: tests/poly_restate.py (the polynomial monomial NDPOLY restated in NumPy over the CPU oracle) pinned to the reference's own
outputs (tests/golden/ref_poly_*, tools/make_golden_poly.py).

The deviation of the restatement from the reference is MEASURED per quantity: the generator stored it as `restate_vs_ref` (relative to
the largest element of a field, relative to the value of an energy), this test recomputes it, prints it and asserts that it has not
grown (twice the stored value or 16 units in the last place, whichever is larger).  A chain of 48 factors and Clenshaw sums of degree
98 amplify rounding, so the GPU tests take their bound from these numbers (8 x, never below tests.util.TOL): tests/poly_restate.py::gpu_bound.
Any mistake in a coefficient, a root index or the order of the correction steps shows at 1e-6 or above."""
import json
import os

import numpy as np
import pytest

from oracle.nd_restate import cplx, real
from tests import poly_restate
from tests.poly_restate import roots_of
from tests.util import random_gauge, random_spinor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ULP = 2.0 ** -52
SEED_6x4 = 66


def load(tag):
    return json.load(open(os.path.join(GOLD, "ref_poly_scalars_%s.json" % tag)))


def inputs(tag):
    """(scalars, dims, gauge, S, phi, stored fields or None)"""
    s = load(tag)
    dims = (s["T"], s["L"], s["L"], s["L"])
    V = int(np.prod(dims))
    f = None
    if tag == "4x4":
        f = np.load(os.path.join(GOLD, "ref_poly_4x4.npz"))
        g = np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"][:V])
    else:
        assert s["gauge"] == "tests.util.random_gauge(%d, V)" % SEED_6x4
        g = random_gauge(SEED_6x4, V)
    N = V // 2
    S = random_spinor(31, N), random_spinor(32, N)
    phi = random_spinor(33, N), random_spinor(34, N)
    return s, dims, g, S, phi, f


@pytest.fixture(scope="module", params=["4x4", "6x4"])
def case(request):
    from oracle.oraclebind import Oracle
    s, dims, g, S, phi, f = inputs(request.param)
    orc = Oracle(*dims, kappa=s["kappa"], mu=0.0)
    gg = np.zeros((orc.VPR, 4, 3, 3, 2))
    gg[:orc.V] = g
    orc.set_gauge(gg)
    return request.param, s, orc, poly_restate.Poly(orc, s["mubar"], s["epsbar"], s["invmaxev"]), S, phi, f


def _rel(x, y):
    return float(np.abs(x - y).max() / np.abs(y).max())


def _grown(now, stored):
    return now > max(2.0 * stored, 16 * ULP)


def test_fixture_content():
    assert sum(os.path.getsize(os.path.join(GOLD, n)) for n in ("ref_poly_4x4.npz", "ref_poly_scalars_4x4.json", "ref_poly_scalars_6x4.json")) < 1 << 20
    f = np.load(os.path.join(GOLD, "ref_poly_4x4.npz"))
    assert sorted(f.files) == sorted(["S_up", "S_dn", "ptilde_up", "ptilde_dn", "phi_up", "phi_dn", "force", "eta_up", "eta_dn", "pf_up", "pf_dn"])
    assert f["force"].shape == (256, 4, 8) and f["pf_up"].shape == (128, 4, 3, 2)
    assert np.array_equal(f["S_up"], random_spinor(31, 128)) and np.array_equal(f["phi_dn"], random_spinor(34, 128))
    for tag in ("4x4", "6x4"):
        s = load(tag)
        n = s["MDPolyDegree"]
        assert n == 49 and len(s["MDPolyCoefs"]) == n and len(s["MDPolyRoots"]) == 2 * n - 2
        assert len(s["PtildeCoefs"]) == s["PtildeDegree"] >= 2 * n
        assert s["evmin"] == s["StildeMin"] / s["StildeMax"] and s["evmax"] == 1.0
        assert s["invmaxev"] == 1.0 / np.sqrt(s["StildeMax"]) and s["Cpol"] == np.sqrt(s["LocNormConst"])
        assert len(s["Ener"]) == 8 and 1 <= s["corrections"] <= 7 and s["energy1"] == s["Ener"][s["corrections"]]
        assert s["energy1_all_seven"] == s["Ener"][7] and s["phi_energy1"] == s["phi_Ener"][s["phi_corrections"]]
        # what the monomial is for: P approximates (Q Q^dagger)^(-1/2) on the interval, so |B pf|^2 of the heatbath's pf is |eta|^2 again
        assert abs(s["Ener"][0] - s["energy0"]) < 1e-3 * s["energy0"]
    # the coefficients depend on the interval only, not on the lattice
    assert load("4x4")["MDPolyCoefs"] == load("6x4")["MDPolyCoefs"] and load("4x4")["PtildeCoefs"] == load("6x4")["PtildeCoefs"]


def test_four_term_combination_adds_left_to_right():
    a, b, c, d = (np.array([x]) for x in (1.0, 2.0 ** -53, 2.0 ** -53, -1.0))
    assert poly_restate.comb4(a, b, c, d, 1.0, 1.0, 1.0, 1.0)[0] == 0.0          # ((1 + u) + u) - 1 with u = half an ulp: both are lost
    assert poly_restate.comb4(b, c, a, d, 1.0, 1.0, 1.0, 1.0)[0] == 2.0 ** -52   # ((u + u) + 1) - 1: they are kept


def test_clenshaw_is_the_chebyshev_sum():
    """on a diagonal `operator` Clenshaw's recursion is sum_j c_j T_j(z) - c_0 / 2 element by element; lengths 1, 2, 3 and 9"""
    rng = np.random.default_rng(3)
    lam = rng.uniform(0.05, 1.0, (6, 4, 3))
    Qsq = lambda xs, xc: (lam * xs, lam * xc)
    Ss, Sc = rng.standard_normal((6, 4, 3)) + 0j, rng.standard_normal((6, 4, 3)) + 0j
    evmin, evmax = 0.04, 1.0
    z = (2 * lam - evmin - evmax) / (evmax - evmin)
    for n in (1, 2, 3, 9):
        c = rng.standard_normal(n)
        want = sum(c[j] * np.cos(j * np.arccos(z)) for j in range(n)) - 0.5 * c[0]
        Rs, Rc = poly_restate.Ptilde_ndpsi(Qsq, list(c), Ss, Sc, evmin, evmax)
        assert np.abs(Rs - want * Ss).max() < 1e-13 and np.abs(Rc - want * Sc).max() < 1e-13


def test_ptilde_and_force_against_the_reference(case):
    tag, s, orc, po, S, phi, f = case
    stored = s["restate_vs_ref"]
    q = po.Ptilde(s["PtildeCoefs"], cplx(S[0]), cplx(S[1]), s["evmin"], s["evmax"])
    sq = float((real(q[0]) ** 2).sum() + (real(q[1]) ** 2).sum())
    assert abs(sq - s["ptilde_sqnorm"]) <= 1e-12 * s["ptilde_sqnorm"]
    df = po.derivative(cplx(phi[0]), cplx(phi[1]), roots_of(s), s["Cpol"], np.zeros((orc.VPR, 4, 8)))[:orc.V]
    assert abs(float((df ** 2).sum()) - s["force_sqnorm"]) <= 1e-11 * s["force_sqnorm"]
    assert abs(float(np.abs(df).max()) - s["force_absmax"]) <= 1e-11 * s["force_absmax"]
    if f is not None:
        d_pt = max(_rel(real(q[0]), f["ptilde_up"]), _rel(real(q[1]), f["ptilde_dn"]))
        d_f = _rel(df, f["force"])
        print("%s restatement vs reference: Ptilde %.3e (stored %.3e), force %.3e (stored %.3e)" % (tag, d_pt, stored["ptilde"], d_f, stored["force"]))
        assert not _grown(d_pt, stored["ptilde"]) and not _grown(d_f, stored["force"])
        assert d_pt < 1e-12 and d_f < 1e-11


def test_heatbath_and_acceptance_against_the_reference(case):
    tag, s, orc, po, S, phi, f = case
    stored = s["restate_vs_ref"]
    roots = roots_of(s)
    e1, steps, en = po.acc(cplx(phi[0]), cplx(phi[1]), roots, s["Cpol"], s["MDPolyCoefs"], s["PtildeCoefs"], s["evmin"], s["evmax"], s["PrecisionHfinal"])
    assert steps == s["phi_corrections"] and abs(e1 - s["phi_energy1"]) <= max(2 * stored["phi_Ener"][steps], 16 * ULP) * abs(e1)
    d = [abs(x - y) / abs(y) for x, y in zip(en[:steps + 1], s["phi_Ener"])]
    print("%s Ener[j] on phi, restatement vs reference: %s (stored %s)" % (tag, d, stored["phi_Ener"]))
    assert not any(_grown(a, b) for a, b in zip(d, stored["phi_Ener"]))
    assert max(d) < 1e-10
    if f is None:
        return
    e0, hu, hd = po.heatbath(cplx(f["eta_up"]), cplx(f["eta_dn"]), roots, s["Cpol"], s["PtildeCoefs"], s["evmin"], s["evmax"])
    d_pf = max(_rel(real(hu), f["pf_up"]), _rel(real(hd), f["pf_dn"]))
    d_e0 = abs(e0 - s["energy0"]) / s["energy0"]
    print("%s heatbath: pf %.3e (stored %.3e), energy0 %.3e (stored %.3e)" % (tag, d_pf, stored["pf"], d_e0, stored["energy0"]))
    assert not _grown(d_pf, stored["pf"]) and not _grown(d_e0, stored["energy0"])
    e1, steps, en = po.acc(cplx(f["pf_up"]), cplx(f["pf_dn"]), roots, s["Cpol"], s["MDPolyCoefs"], s["PtildeCoefs"], s["evmin"], s["evmax"], s["PrecisionHfinal"])
    assert steps == s["corrections"]
    d = [abs(x - y) / abs(y) for x, y in zip(en[:steps + 1], s["Ener"])]
    print("%s Ener[j] on the heatbath's pf: %s (stored %s)" % (tag, d, stored["Ener"]))
    assert not any(_grown(a, b) for a, b in zip(d, stored["Ener"]))
    # the stop rule: a precision above the first difference stops after one correction, and the energy is Ener[1]
    e1, steps, en1 = po.acc(cplx(f["pf_up"]), cplx(f["pf_dn"]), roots, s["Cpol"], s["MDPolyCoefs"], s["PtildeCoefs"], s["evmin"], s["evmax"], np.inf)
    assert steps == 1 and e1 == en1[1] == en[1] and en1[2:] == [0.0] * 6
