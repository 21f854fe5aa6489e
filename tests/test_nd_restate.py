"""CPU: oracle/nd_restate.py, the doublet reference of the GPU shape tests, pinned to the reference's own outputs.

* 4^4: composed with the CPU oracle's Hopping_Matrix, it reproduces every operator output of tests/golden/ref_nd_4x4.npz,
  and its cg_her_nd / cg_mms_tm_nd reproduce the fixture's iteration counts, shift drops and solutions;
* 8^4: on the inputs tools/make_golden_nd.py made (the reference's RANLUX fields, seed 123456), it reproduces the
  iteration counts, the drop schedule and the solution norms of tests/golden/ref_nd_scalars_8x8.json.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nd_restate as nd
from oracle.oraclebind import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _pair_err(a, b, ra, rb):
    num = np.sqrt(np.sum(np.abs(a - ra) ** 2) + np.sum(np.abs(b - rb) ** 2))
    return num / np.sqrt(np.sum(np.abs(ra) ** 2) + np.sum(np.abs(rb) ** 2))


@pytest.fixture(scope="module")
def fx4():
    f = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_nd_scalars_4x4.json")))
    orc = Oracle(4, 4, 4, 4, kappa=s["kappa"], mu=0.0)
    orc.set_gauge(f["gauge"])
    H = nd.hop_over(orc.Hopping_Matrix, orc.Vh)
    return H, f, s


def _ref(f, name):
    return nd.cplx(f[name + "_s"]), nd.cplx(f[name + "_c"])


def test_operators_reproduce_the_4x4_fixture(fx4):
    H, f, s = fx4
    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    ks, kc, js, jc = (nd.cplx(f[k]) for k in ("k_s", "k_c", "j_s", "j_c"))
    got = {
        "Qtm_ndpsi": nd.Qtm_ndpsi(H, ks, kc, mb, eb, c),
        "Qtm_dagger_ndpsi": nd.Qtm_dagger_ndpsi(H, ks, kc, mb, eb, c),
        "Qtm_pm_ndpsi": nd.Qtm_pm_ndpsi(H, ks, kc, mb, eb, c),
        "M_ee_inv_ndpsi": nd.m_ee_inv(ks, kc, mb, eb),
        "M_oo_sub_g5_ndpsi": nd.m_oo_sub_g5(ks, kc, js, jc, mb, eb),
        "H_eo_tm_ndpsi_0": nd.H_eo_tm_ndpsi(H, ks, kc, 0, mb, eb),
        "H_eo_tm_ndpsi_1": nd.H_eo_tm_ndpsi(H, ks, kc, 1, mb, eb),
    }
    errs = {k: _pair_err(*v, *_ref(f, k)) for k, v in got.items()}
    assert all(e < 1e-13 for e in errs.values()), errs


def test_cg_her_nd_reproduces_the_4x4_fixture(fx4):
    H, f, s = fx4
    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    g = s["cg_her_nd"]
    ks, kc = nd.cplx(f["k_s"]), nd.cplx(f["k_c"])
    z = np.zeros_like(ks)
    it, xu, xd = nd.cg_her_nd(lambda u, d: nd.Qtm_pm_ndpsi(H, u, d, mb, eb, c), z, z, ks, kc, g["max_iter"], g["eps_sq"], g["rel_prec"])
    assert it == g["iters"]
    assert _pair_err(xu, xd, nd.cplx(f["cg_her_nd_up"]), nd.cplx(f["cg_her_nd_dn"])) < 1e-10


def test_cg_mms_tm_nd_reproduces_the_4x4_fixture(fx4):
    H, f, s = fx4
    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    m = s["cg_mms_tm_nd"]
    ks, kc = nd.cplx(f["k_s"]), nd.cplx(f["k_c"])
    it, P, drops, left = nd.cg_mms_tm_nd(lambda u, d: nd.Qtm_pm_ndpsi(H, u, d, mb, eb, c), ks, kc, m["shifts"], m["max_iter"],
                                         m["eps_sq"], m["rel_prec"])
    assert it == m["iters"]
    assert drops == m["drops"] and left == len(m["shifts"]) - len(m["drops"])
    for k, (u, d) in enumerate(P):
        assert _pair_err(u, d, nd.cplx(f["cg_mms_up_%d" % k]), nd.cplx(f["cg_mms_dn_%d" % k])) < 1e-10, k


def _child8():
    """Runs in its own process (the reference keeps one lattice in C globals): the 8^4 inputs of tools/make_golden_nd.py,
    the restatement over the oracle's Hopping_Matrix, and the scalars of ref_nd_scalars_8x8.json."""
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    s = json.load(open(os.path.join(GOLD, "ref_nd_scalars_8x8.json")))
    T, L = s["T"], s["L"]
    r = RefLattice(T, L, L, L, kappa=s["kappa"], mu=0.0, nfields=8)
    r.random_fields(s["seed"])
    for k in (1, 2, 3):
        r.lib.tmref_random_spinor_eo(k)
    orc = Oracle(T, L, L, L, kappa=s["kappa"], mu=0.0)
    orc.set_gauge(r.gauge().copy())
    N = orc.Vh
    H = nd.hop_over(orc.Hopping_Matrix, N)
    ks, kc = nd.cplx(r.spinor(0, N).copy()), nd.cplx(r.spinor(1, N).copy())
    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    f = lambda u, d: nd.Qtm_pm_ndpsi(H, u, d, mb, eb, c)
    g, m = s["cg_her_nd"], s["cg_mms_tm_nd"]
    z = np.zeros_like(ks)
    it_her, xu, xd = nd.cg_her_nd(f, z, z, ks, kc, g["max_iter"], g["eps_sq"], g["rel_prec"])
    it_mms, P, drops, left = nd.cg_mms_tm_nd(f, ks, kc, m["shifts"], m["max_iter"], m["eps_sq"], m["rel_prec"])
    nsq = lambda u, d: float(np.vdot(u, u).real + np.vdot(d, d).real)
    print(json.dumps({"her_iters": it_her, "her_norm": nsq(xu, xd), "mms_iters": it_mms, "drops": drops, "left": left,
                      "mms_norms": [nsq(u, d) for u, d in P]}))


def test_solvers_reproduce_the_8x8_scalars():
    from oracle.refbind import ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libtmref.so not built (needs the reference tree at build time)")
    code = "import sys; sys.path.insert(0, %r); from tests.test_nd_restate import _child8; _child8()" % ROOT
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    got = json.loads(out.stdout.strip().splitlines()[-1])
    s = json.load(open(os.path.join(GOLD, "ref_nd_scalars_8x8.json")))
    g, m = s["cg_her_nd"], s["cg_mms_tm_nd"]
    assert got["her_iters"] == g["iters"]
    assert abs(got["her_norm"] - g["sol_norm"]) <= 1e-10 * g["sol_norm"]
    assert got["mms_iters"] == m["iters"]
    assert got["drops"] == m["drops"] and got["left"] == len(m["shifts"]) - len(m["drops"])
    for k, (a, b) in enumerate(zip(got["mms_norms"], m["sol_norms"])):
        assert abs(a - b) <= 1e-10 * b, (k, a, b)
