"""CPU: the NumPy restatement of the rational monomials' loop bodies (tests/rat_restate.py) pinned to the reference's own
outputs on the 4^4 fixture (tests/golden/ref_rat_4x4.npz, tools/make_golden_rat.py)."""
import json
import os

import numpy as np
import pytest

from oracle.nd_restate import cplx, hop_over, real
from oracle.oraclebind import Oracle
from tests import rat_restate
from tests.util import TOL, rel_err

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_rat_4x4.npz")), json.load(open(os.path.join(GOLD, "ref_rat_scalars_4x4.json")))


@pytest.fixture(scope="module")
def rat(fx):
    f, s = fx
    orc = Oracle(s["T"], s["L"], s["L"], s["L"], kappa=s["kappa"], mu=0.0)
    orc.set_gauge(np.ascontiguousarray(f["gauge"]))
    return rat_restate.Rat(orc, s["mubar"], s["epsbar"])


def chi_nd(f, s):
    return [(cplx(f["chi_up_%d" % j]), cplx(f["chi_dn_%d" % j])) for j in range(s["np"])]


def test_fixture_sizes_and_coverage(fx):
    f, s = fx
    size = sum(os.path.getsize(os.path.join(GOLD, n)) for n in ("ref_rat_4x4.npz", "ref_rat_scalars_4x4.json"))
    assert size < 1 << 20
    assert s["np"] == 3 and all(len(s[k]) == 3 for k in ("mu", "rmu", "nu", "rnu"))
    assert s["mubar"] != 0 and s["epsbar"] != 0 and s["invmaxev"] not in (0.0, 1.0)
    want = {"gauge", "eta_up", "eta_dn", "Q_tau1_s", "Q_tau1_c", "ndrat_derivative", "ndrat_pf_up", "ndrat_pf_dn", "rat_derivative", "rat_pf"}
    want |= {"chi_%s_%d" % (fl, j) for fl in ("up", "dn") for j in range(3)}
    assert want == set(f.files)
    assert {"ndrat_energy0", "ndrat_energy1", "rat_energy0", "rat_energy1"} <= set(s)
    assert np.abs(f["ndrat_derivative"]).max() > 0 and np.abs(f["rat_derivative"]).max() > 0


def test_Q_tau1_sub_const_ndpsi(fx, rat):
    f, s = fx
    H = hop_over(rat.orc.Hopping_Matrix, rat.N)
    ls, lc = rat_restate.Q_tau1_sub_const_ndpsi(H, cplx(f["chi_up_0"]), cplx(f["chi_dn_0"]), -1j * s["mu"][0], 1., s["invmaxev"], s["mubar"], s["epsbar"])
    assert rel_err(real(ls), f["Q_tau1_s"]) < TOL and rel_err(real(lc), f["Q_tau1_c"]) < TOL


def test_ndrat_bodies(fx, rat):
    f, s = fx
    chi = chi_nd(f, s)
    df = rat.ndrat_force(chi, s["mu"], s["rmu"], s["invmaxev"], np.zeros((rat.orc.VPR, 4, 8)))
    assert rel_err(df[:rat.orc.V], f["ndrat_derivative"]) < TOL
    eu, ed = cplx(f["eta_up"]), cplx(f["eta_dn"])
    e0, pu, pd = rat.ndrat_heatbath(eu, ed, chi, s["nu"], s["rnu"], s["invmaxev"])
    assert abs(e0 - s["ndrat_energy0"]) < TOL * abs(e0)
    assert rel_err(real(pu), f["ndrat_pf_up"]) < TOL and rel_err(real(pd), f["ndrat_pf_dn"]) < TOL
    e1 = rat.ndrat_acc(eu, ed, chi, s["rmu"])
    assert abs(e1 - s["ndrat_energy1"]) < TOL * abs(e1)


def test_rat_bodies(fx, rat):
    f, s = fx
    chi = [c[0] for c in chi_nd(f, s)]
    rat.orc.set_mu(0.3)   # rat works at g_mu = 0 whatever the oracle is set to, and puts it back
    df = rat.rat_force(chi, s["rmu"], np.zeros((rat.orc.VPR, 4, 8)))
    assert rat.orc.mu == 0.3
    assert rel_err(df[:rat.orc.V], f["rat_derivative"]) < TOL
    eta = cplx(f["eta_up"])
    e0, pf = rat.rat_heatbath(eta, chi, s["nu"], s["rnu"])
    assert abs(e0 - s["rat_energy0"]) < TOL * abs(e0)
    assert rel_err(real(pf), f["rat_pf"]) < TOL
    e1 = rat.rat_acc(eta, chi, s["rmu"])
    assert abs(e1 - s["rat_energy1"]) < TOL * abs(e1)
    rat.orc.set_mu(0.0)
