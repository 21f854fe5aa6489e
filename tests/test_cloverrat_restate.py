"""CPU: tests/cloverrat_restate.py, the reference of the GPU tests of the tr-log energies and of the clover rational monomial, pinned to
the reference's own outputs (tests/golden/ref_cloverrat_4x4.npz, ref_cloverrat_scalars_{4x4,8x8}.json, made by
tools/make_golden_cloverrat.py).

* 4^4, on the seed-123456 links and spinors of tests/golden/ref_nd_4x4.npz: sw_trace / sw_trace_nd, the force statements of
  rat_monomial.c for CLOVERRAT with and without the tr-log term, the heatbath and the acceptance energy, and the iteration count and
  solution norms of cg_mms_tm on Qsw_pm_psi (tests/mms_restate.py over the oracle's operator);
* 8^4, on tests.util.random_gauge / random_spinor with the seeds the fixture records: the traces and the iteration count;
* the bound of tests/test_gpu_trlog.py, TOL * sum |per-site term|: the reference's own values lie within it of the restatement
  (the distances the tool measured are in the scalars files, and are measured again here).
"""
import json
import os

import numpy as np
import pytest

from oracle.oraclebind import Oracle
from tests import cloverrat_restate as cr
from tests import mms_restate as mms
from tests import ndsw_restate as sw
from tests.util import TOL, random_gauge, random_spinor, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SITES = slice(0, None, 2)      # tools/make_golden_cloverrat.py stores per-site outputs on every second site, and the norm over all


def _scalars(tag):
    return json.load(open(os.path.join(GOLD, "ref_cloverrat_scalars_%s.json" % tag)))


@pytest.fixture(scope="module")
def fx4():
    f = np.load(os.path.join(GOLD, "ref_cloverrat_4x4.npz"))
    base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))      # the gauge field and the four spinors: same seed, same calls
    s = _scalars("4x4")
    orc = Oracle(4, 4, 4, 4, kappa=s["kappa"], mu=0.0)
    orc.set_gauge(base["gauge"])
    m = cr.CloverRat(orc, s["kappa"], s["c_sw"])
    k = {n: cr.cplx(base[n]) for n in ("k_s", "k_c", "j_s", "j_c")}
    return orc, m, f, s, k


@pytest.fixture(scope="module")
def fx8():
    s = _scalars("8x8")
    orc = Oracle(8, 8, 8, 8, kappa=s["kappa"], mu=0.0, threads=8)
    orc.set_gauge(random_gauge(s["gauge_seed"], orc.VPR))
    return orc, cr.CloverRat(orc, s["kappa"], s["c_sw"]), s


def test_fixture_is_what_the_tool_writes():
    size = os.path.getsize(os.path.join(GOLD, "ref_cloverrat_4x4.npz"))
    assert size <= os.path.getsize(os.path.join(GOLD, "ref_ndsw_4x4.npz"))
    s, n = _scalars("4x4"), json.load(open(os.path.join(GOLD, "ref_ndsw_scalars_4x4.json")))
    assert s["c_sw"] != 0 and s["seed"] == n["seed"] and (s["kappa"], s["c_sw"]) == (n["kappa"], n["c_sw"])
    assert s["points"] == {k: list(v[:2]) for k, v in sw.POINTS.items()} and s["trace_mu"] != 0


def _check_traces(orc, s):
    cl = cr.clover_of(orc, s["kappa"], s["c_sw"])
    mu = s["trace_mu"]
    want = {"sw_trace_EE_0": cr.sw_trace(cl, cr.EE, 0.0), "sw_trace_EE_mu": cr.sw_trace(cl, cr.EE, mu), "sw_trace_OO_mu": cr.sw_trace(cl, cr.OO, mu)}
    for name, (mb, eb) in s["points"].items():
        want["sw_trace_nd_EE_" + name] = cr.sw_trace_nd(cl, cr.EE, mb, eb)
    assert set(want) == set(s["traces"])
    for name, (w, scale) in want.items():
        dist = abs(s["traces"][name] - w) / scale
        print("%s: reference %.15e, restatement %.15e, distance / scale %.2e (the tool measured %.2e)" % (name, s["traces"][name], w, dist, s["trace_distance"][name]))
        assert dist <= TOL                                              # the reference's own value satisfies the GPU tests' bound
        assert s["trace_distance"][name] <= TOL
        assert abs(scale - s["trace_scale"][name]) <= 1e-12 * scale
    # eps = 0: sw_trace_nd is sw_trace (clover_det.c:199-200)
    a, b = cr.sw_trace(cl, cr.EE, mu), cr.sw_trace_nd(cl, cr.EE, mu, 0.0)
    assert abs(a[0] - b[0]) <= TOL * a[1]
    assert abs(float((orc.sw_term(s["kappa"], s["c_sw"]) ** 2).sum()) - s["sw_norm"]) <= 2 * TOL * s["sw_norm"]


def test_traces_reproduce_the_4x4_scalars(fx4):
    _check_traces(fx4[0], fx4[3])


def test_traces_reproduce_the_8x8_scalars(fx8):
    _check_traces(fx8[0], fx8[2])


def test_monomial_bodies_reproduce_the_fixture(fx4):
    orc, m, f, s, k = fx4
    assert m.fails == 0
    chi, eta = [k[n] for n in s["chi"]], k[s["eta"]]
    for trlog in (0, 1):
        df = np.zeros((orc.VPR, 4, 8))
        m.force(chi, s["rmu"], trlog, df)
        assert rel_err(df[:orc.V], f["cloverrat_derivative_trlog%d" % trlog]) < TOL, trlog
    assert np.abs(f["cloverrat_derivative_trlog1"] - f["cloverrat_derivative_trlog0"]).max() > 0
    e0, pf = m.heatbath(eta, chi, s["nu"], s["rnu"])
    assert abs(e0 - s["cloverrat_energy0"]) < TOL * abs(e0)
    ref = cr.cplx(f["cloverrat_pf"])
    assert np.sqrt(np.sum(np.abs(pf[SITES] - ref) ** 2) / np.sum(np.abs(ref) ** 2)) < TOL
    n = float(np.vdot(pf, pf).real)
    assert abs(n - s["norms"]["cloverrat_pf"]) <= 2 * TOL * n
    e1 = m.acc(eta, chi, s["rmu"])
    assert abs(e1 - s["cloverrat_energy1"]) < TOL * abs(e1)


def _check_solver(m, src, s):
    g = s["cg_mms_tm"]
    it, reached, P, drops, left = mms.cg_mms_tm(m.Qsq, src, g["shifts"], g["max_iter"], g["eps_sq"], g["rel_prec"])
    assert it == g["iters"]
    for j, (p, want) in enumerate(zip(P, g["sol_norms"])):
        assert abs(float(np.vdot(p, p).real) - want) <= 1e-10 * want, j


def test_solver_reproduces_the_4x4_scalars(fx4):
    orc, m, f, s, k = fx4
    _check_solver(m, k["k_s"], s)


def test_solver_reproduces_the_8x8_scalars(fx8):
    orc, m, s = fx8
    _check_solver(m, cr.cplx(random_spinor(s["source_seed"], orc.Vh)), s)
