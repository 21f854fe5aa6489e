"""CPU: tests/ndsw_restate.py, the clover-doublet reference of the GPU tests, pinned to the reference's own outputs
(tests/golden/ref_ndsw_4x4.npz, ref_ndsw_scalars_{4x4,8x8}.json, made by tools/make_golden_ndsw.py).

* 4^4: over the CPU oracle's Hopping_Matrix and sw_term it reproduces sw_invert_nd, the three site-local functions, the six
  operators, sw_deriv_nd and the three NDCLOVERRAT bodies (tolerances of test_nd_restate.py / test_rat_restate.py), and the
  restated solvers on Qsw_pm_ndpsi reproduce the fixture's iteration counts, drops and solution norms;
* 8^4: the iteration counts, the drop schedule and the solution norms of ref_ndsw_scalars_8x8.json;
* the conditioning premise of the GPU tests: on every shape and at every (mubar, epsbar) point they use, the largest condition
  number of (1+T)^2 + mubar^2 - epsbar^2 stays below 10^3.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.oraclebind import Oracle
from tests import ndsw_restate as sw
from tests.util import TOL, random_gauge, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SITES = slice(0, None, 2)      # tools/make_golden_ndsw.py stores per-site outputs on every second site, and the norm over all


def _pair_err(a, b, ra, rb):
    num = np.sqrt(np.sum(np.abs(a - ra) ** 2) + np.sum(np.abs(b - rb) ** 2))
    return num / np.sqrt(np.sum(np.abs(ra) ** 2) + np.sum(np.abs(rb) ** 2))


@pytest.fixture(scope="module")
def fx4():
    f = np.load(os.path.join(GOLD, "ref_ndsw_4x4.npz"))
    base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))      # the gauge field and the four spinors: same seed, same calls
    s = json.load(open(os.path.join(GOLD, "ref_ndsw_scalars_4x4.json")))
    orc = Oracle(4, 4, 4, 4, kappa=s["kappa"], mu=0.0)
    orc.set_gauge(base["gauge"])
    cl = sw.clover_of(orc, s["kappa"], s["c_sw"])
    swi = cl.sw_invert_nd(s["mshift"])
    H = sw.hop_over(orc.Hopping_Matrix, orc.Vh)
    k = {n: sw.cplx(base[n]) for n in ("k_s", "k_c", "j_s", "j_c")}
    return orc, cl, swi, H, f, s, k


def _check(f, s, name, got):
    ls, lc = got
    e = _pair_err(ls[SITES], lc[SITES], sw.cplx(f[name + "_s"]), sw.cplx(f[name + "_c"]))
    n = float(np.vdot(ls, ls).real + np.vdot(lc, lc).real)
    assert e < TOL, (name, e)
    assert abs(n - s["norms"][name]) <= 2 * TOL * n, (name, n, s["norms"][name])


def test_fixture_is_what_the_tool_writes():
    size = os.path.getsize(os.path.join(GOLD, "ref_ndsw_4x4.npz"))
    assert size <= os.path.getsize(os.path.join(GOLD, "ref_rat_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_ndsw_scalars_4x4.json")))
    assert s["c_sw"] != 0 and (s["mubar"], s["epsbar"], s["invmaxev"]) == sw.FIXTURE
    assert abs(s["mshift"] - (s["mubar"] ** 2 - s["epsbar"] ** 2)) < 1e-18


def test_sw_invert_nd_reproduces_the_fixture(fx4):
    orc, cl, swi, H, f, s, k = fx4
    assert cl.fails == 0
    assert rel_err(swi[SITES], f["sw_inv_nd"]) < TOL
    assert abs(float((swi ** 2).sum()) - s["sw_inv_nd_norm"]) <= 2 * TOL * s["sw_inv_nd_norm"]
    assert abs(float((orc.sw_term(s["kappa"], s["c_sw"]) ** 2).sum()) - s["sw_norm"]) <= 2 * TOL * s["sw_norm"]
    # (1+T)^2 + shift times the inverse is 1
    a = cl.m[0] @ cl.m[0] + s["mshift"] * np.eye(6)
    assert np.abs(a @ cl.inv - np.eye(6)).max() < 1e-13


def test_site_local_functions_reproduce_the_fixture(fx4):
    orc, cl, swi, H, f, s, k = fx4
    mb, eb = s["mubar"], s["epsbar"]
    a = sw.assign_mul_one_sw_pm_imu_eps(cl, sw.EE, k["k_s"], k["k_c"], mb, eb)
    _check(f, s, "assign_mul_one_sw_pm_imu_eps", a)
    lc, ls = sw.clover_inv_nd(cl, sw.EE, a[1], a[0])
    _check(f, s, "clover_inv_nd", (ls, lc))
    lc, ls = sw.clover_gamma5_nd(cl, sw.OO, k["k_c"], k["k_s"], k["j_c"], k["j_s"], mb, -eb)
    _check(f, s, "clover_gamma5_nd", (ls, lc))


def test_operators_reproduce_the_fixture(fx4):
    orc, cl, swi, H, f, s, k = fx4
    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    ks, kc = k["k_s"], k["k_c"]
    t = s["tau1_args"]
    _check(f, s, "Qsw_ndpsi", sw.Qsw_ndpsi(cl, H, ks, kc, mb, eb, c))
    _check(f, s, "Qsw_dagger_ndpsi", sw.Qsw_dagger_ndpsi(cl, H, ks, kc, mb, eb, c))
    _check(f, s, "Qsw_pm_ndpsi", sw.Qsw_pm_ndpsi(cl, H, ks, kc, mb, eb, c))
    _check(f, s, "H_eo_sw_ndpsi", sw.H_eo_sw_ndpsi(cl, H, ks, kc, mb, eb))
    _check(f, s, "Msw_ee_inv_ndpsi", sw.Msw_ee_inv_ndpsi(cl, ks, kc, mb, eb))
    _check(f, s, "Qsw_tau1_sub_const_ndpsi", sw.Qsw_tau1_sub_const_ndpsi(cl, H, ks, kc, complex(*t["z"]), t["Cpol"], t["invev"], mb, eb))


def test_sw_deriv_nd_reproduces_the_fixture(fx4):
    orc, cl, swi, H, f, s, k = fx4
    swm, swp = np.zeros((orc.V, 4, 3, 3, 2)), np.zeros((orc.V, 4, 3, 3, 2))
    sw.sw_deriv_nd(cl, sw.EE, swm, swp)
    lex = cl.lex[0]
    assert rel_err(swm[lex][SITES], f["sw_deriv_nd_swm"]) < TOL and rel_err(swp[lex][SITES], f["sw_deriv_nd_swp"]) < TOL
    for got, want in zip((float((swm ** 2).sum()), float((swp ** 2).sum())), s["sw_deriv_nd_norms"]):
        assert abs(got - want) <= 2 * TOL * want
    assert np.abs(swm[cl.lex[1]]).max() == 0 and np.abs(swp[cl.lex[1]]).max() == 0


def test_monomial_bodies_reproduce_the_fixture(fx4):
    orc, cl, swi, H, f, s, k = fx4
    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    chi = [(k[a], k[b]) for a, b in s["chi"]]
    eta = (k[s["eta"][0]], k[s["eta"][1]])
    m = sw.NdCloverRat(orc, cl, mb, eb)
    for trlog in (0, 1):
        df = np.zeros((orc.VPR, 4, 8))
        m.force(chi, s["mu"], s["rmu"], c, s["kappa"], s["c_sw"], trlog, df)
        assert rel_err(df[:orc.V], f["ndcloverrat_derivative_trlog%d" % trlog]) < TOL, trlog
    assert np.abs(f["ndcloverrat_derivative_trlog1"] - f["ndcloverrat_derivative_trlog0"]).max() > 0
    e0, pu, pd = m.heatbath(eta[0], eta[1], chi, s["nu"], s["rnu"], c)
    assert abs(e0 - s["ndcloverrat_energy0"]) < TOL * abs(e0)
    _check(f, s, "ndcloverrat_pf", (pu, pd))
    e1 = m.acc(eta[0], eta[1], chi, s["rmu"])
    assert abs(e1 - s["ndcloverrat_energy1"]) < TOL * abs(e1)


def _solve(cl, H, ks, kc, s):
    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    from oracle import nd_restate as nd
    op = lambda u, d: sw.Qsw_pm_ndpsi(cl, H, u, d, mb, eb, c)
    g, m = s["cg_her_nd"], s["cg_mms_tm_nd"]
    z = np.zeros_like(ks)
    it_her, xu, xd = nd.cg_her_nd(op, z, z, ks, kc, g["max_iter"], g["eps_sq"], g["rel_prec"])
    it_mms, P, drops, left = nd.cg_mms_tm_nd(op, ks, kc, m["shifts"], m["max_iter"], m["eps_sq"], m["rel_prec"])
    nsq = lambda u, d: float(np.vdot(u, u).real + np.vdot(d, d).real)
    return {"her_iters": it_her, "her_norm": nsq(xu, xd), "mms_iters": it_mms, "drops": drops, "left": left,
            "mms_norms": [nsq(u, d) for u, d in P]}


def _check_solvers(got, s):
    g, m = s["cg_her_nd"], s["cg_mms_tm_nd"]
    assert got["her_iters"] == g["iters"]
    assert abs(got["her_norm"] - g["sol_norm"]) <= 1e-10 * g["sol_norm"]
    assert got["mms_iters"] == m["iters"]
    assert got["drops"] == m["drops"] and got["left"] == len(m["shifts"]) - len(m["drops"])
    for j, (a, b) in enumerate(zip(got["mms_norms"], m["sol_norms"])):
        assert abs(a - b) <= 1e-10 * b, (j, a, b)


def test_solvers_reproduce_the_4x4_scalars(fx4):
    orc, cl, swi, H, f, s, k = fx4
    _check_solvers(_solve(cl, H, k["k_s"], k["k_c"], s), s)


def _child8():
    """Runs in its own process (the reference keeps one lattice in C globals): the 8^4 inputs of tools/make_golden_ndsw.py."""
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    s = json.load(open(os.path.join(GOLD, "ref_ndsw_scalars_8x8.json")))
    T, L = s["T"], s["L"]
    r = RefLattice(T, L, L, L, kappa=s["kappa"], mu=0.0, nfields=8)
    r.random_fields(s["seed"])
    for j in (1, 2, 3):
        r.lib.tmref_random_spinor_eo(j)
    orc = Oracle(T, L, L, L, kappa=s["kappa"], mu=0.0)
    orc.set_gauge(r.gauge().copy())
    N = orc.Vh
    cl = sw.clover_of(orc, s["kappa"], s["c_sw"])
    cl.sw_invert_nd(s["mshift"])
    H = sw.hop_over(orc.Hopping_Matrix, N)
    ks, kc = sw.cplx(r.spinor(0, N).copy()), sw.cplx(r.spinor(1, N).copy())
    print(json.dumps(_solve(cl, H, ks, kc, s)))


def test_solvers_reproduce_the_8x8_scalars():
    from oracle.refbind import ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libtmref.so not built (needs the reference tree at build time)")
    code = "import sys; sys.path.insert(0, %r); from tests.test_ndsw_restate import _child8; _child8()" % ROOT
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    _check_solvers(json.loads(out.stdout.strip().splitlines()[-1]), json.load(open(os.path.join(GOLD, "ref_ndsw_scalars_8x8.json"))))


def test_every_gpu_case_is_well_conditioned():
    """The premise of the GPU tests: no (1+T)^2 + mubar^2 - epsbar^2 they invert is near-singular."""
    s = json.load(open(os.path.join(GOLD, "ref_ndsw_scalars_4x4.json")))
    worst = {}
    shapes = [sh for sh, _ in sw.SHAPES] + [(4, 4, 4, 4), (8, 8, 8, 8)] + sw.FORCE_SHAPES[1:] + [sw.DRIVER_SHAPE]
    for shape in shapes:
        orc = Oracle(*shape, kappa=sw.KAPPA, mu=0.0, theta=sw.THETA, threads=8)
        orc.set_gauge(random_gauge(sw.shape_seed(shape), orc.VPR))
        cl = sw.clover_of(orc, sw.KAPPA, sw.C_SW)
        for name, (mb, eb, _) in sw.POINTS.items():
            worst[(shape, name)] = cl.cond(mb * mb - eb * eb)
            if shape == (4, 2, 6, 2):
                worst[(shape, "refusals")] = cl.cond(sw.REFUSAL_SHIFT)
    # the reference's own gauge field (tests/test_gpu_ndsw_solvers.py::test_iteration_counts_of_the_reference, tests/ndsw_dropin_child.py)
    base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
    orc = Oracle(4, 4, 4, 4, kappa=s["kappa"], mu=0.0)
    orc.set_gauge(base["gauge"])
    worst[("fixture gauge", "fixture")] = sw.clover_of(orc, s["kappa"], s["c_sw"]).cond(s["mshift"])
    assert max(worst.values()) < sw.COND_MAX, max(worst.items(), key=lambda kv: kv[1])
    assert any(eb > mb for mb, eb, _ in sw.POINTS.values()) and any(eb == 0 for _, eb, _ in sw.POINTS.values())
    assert s["mshift"] > 0 > sw.POINTS["eps_gt_mu"][0] ** 2 - sw.POINTS["eps_gt_mu"][1] ** 2
