"""CPU: the single-flavour multi-shift CG (solver/cg_mms_tm.c) -- C-ABI exports, the drop-in declaration, and the NumPy
restatement (tests/mms_restate.py) pinned to the reference's own outputs (tests/golden/ref_mms_*, tools/make_golden_mms.py).

The restatement runs over Qtm_pm_psi, Qsw_pm_psi and Q_pm_psi of the CPU oracle (oracle/oraclebind.py; Q_pm_psi composed here
from its D_psi and gamma5 as tm_operators.c:380-388 does).  4^4: every fixture case's return value, drop schedule, shifts left,
reached precision and solutions.  8^4: counts, drops and solution norms; that case takes its gauge field from the reference
(oracle/_ref) and is skipped without it."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle.nd_restate import cplx, real
from oracle.oraclebind import Oracle
from tests import mms_restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_core_symbols_exported():
    syms = _exports(os.path.join(LIB, "libtmlqcd_hip.so"))
    assert {"tmhip_cg_mms_tm", "tmhip_mms_active_shifts", "tmhip_mms_form"} <= syms


def test_dropin_declares_and_exports_cg_mms_tm():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    # solver/cg_mms_tm.h:31
    assert re.search(r"int\s+cg_mms_tm\(\s*spinor\s*\*\*\s*const\s+P\s*,\s*spinor\s*\*\s*const\s+Q\s*,\s*tmlqcd_solver_params\s*\*\s*solver_params\s*,"
                     r"\s*double\s*\*\s*cgmms_reached_prec\s*\)\s*;", hdr)
    assert "cg_mms_tm" in _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))


def test_op_enum_appended():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    assert "TMHIP_OP_QSW_PM = 5" in hdr and "TMHIP_OP_Q_PM_FULL = 6" in hdr


def operator(orc, name, mu, sw=None):
    """A(x) on complex fields: Qtm_pm_psi / Qsw_pm_psi (one parity) or Q_pm_psi (full lattice, lexicographic)"""
    orc.set_mu(mu)
    if name == "Q_pm_psi":
        V = orc.V

        def A(x):
            k, l, t = real(x), np.zeros((V, 4, 3, 2)), np.zeros((V, 4, 3, 2))
            orc.set_mu(-mu); orc.D_psi(l, k); orc.gamma5(t, l, V)
            orc.set_mu(mu); orc.D_psi(l, t); orc.gamma5(l, l, V)
            return cplx(l)
        return A

    def A(x):
        l = np.zeros((orc.Vh, 4, 3, 2))
        orc.op(name, l, real(x))
        return cplx(l)
    return A


def oracle_for(T, L, gauge, kappa, c_sw, case):
    orc = Oracle(T, L, L, L, kappa=kappa, mu=case["g_mu"])
    orc.set_gauge(np.ascontiguousarray(gauge))
    if case["op"] == "Qsw_pm_psi":
        sw = orc.sw_term(kappa, c_sw)
        swi, fails = orc.sw_invert(sw, 0, case["g_mu"])
        assert fails == 0
        orc.set_clover(sw, swi)
    return orc


def _rel(a, b):
    return np.sqrt(np.sum(np.abs(a - b) ** 2) / np.sum(np.abs(b) ** 2))


@pytest.fixture(scope="module")
def fx4():
    return np.load(os.path.join(GOLD, "ref_mms_4x4.npz")), json.load(open(os.path.join(GOLD, "ref_mms_scalars_4x4.json")))


def test_fixture_sizes_and_coverage(fx4):
    f, s = fx4
    size = sum(os.path.getsize(os.path.join(GOLD, n)) for n in ("ref_mms_4x4.npz", "ref_mms_scalars_4x4.json"))
    assert size < 1 << 20
    c = s["cases"]
    assert c["qtm"]["drops"] and c["qtm"]["g_mu"] != 0 and len(c["qtm"]["shifts"]) == 5
    assert c["qsw"]["op"] == "Qsw_pm_psi" and s["c_sw"] > 0 and c["qsw"]["g_mu"] != 0
    assert c["qpm_full"]["op"] == "Q_pm_psi" and c["qpm_full"]["g_mu"] == 0 and len(c["qpm_full"]["shifts"]) == 4
    assert c["qtm_rel"]["rel_prec"] == 1 and c["qtm_cut"]["iters"] == -1
    assert all(v["sloppy_after"] == 0 for v in c.values())   # cg_mms_tm.c:192


@pytest.mark.parametrize("name", ["qtm", "qsw", "qpm_full", "qtm_rel", "qtm_cut"])
def test_restatement_reproduces_the_4x4_fixture(fx4, name):
    f, s = fx4
    case = s["cases"][name]
    orc = oracle_for(4, 4, f["gauge"], s["kappa"], s["c_sw"], case)
    A = operator(orc, case["op"], case["g_mu"])
    Q = cplx(f["q_full"] if case["op"] == "Q_pm_psi" else f["q_eo"])
    it, reached, P, drops, left = mms_restate.cg_mms_tm(A, Q, case["shifts"], case["max_iter"], case["eps_sq"], case["rel_prec"])
    assert it == case["iters"]
    assert drops == case["drops"] and left == case["active_at_exit"]
    assert abs(reached - case["reached_prec"]) <= 1e-6 * case["reached_prec"]
    for k in range(len(case["shifts"])):
        assert _rel(P[k], cplx(f["%s_P%d" % (name, k)])) < 1e-10, k


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %r)
from oracle.refbind import RefLattice
r = RefLattice(8, 8, 8, 8, kappa=0.125, mu=0.02, nfields=40)
r.random_fields(123456)
r.lib.tmref_random_spinor_eo(0)
np.save(sys.argv[1], r.gauge().copy())
np.save(sys.argv[2], r.spinor(0, r.V // 2).copy())
"""


def test_restatement_reproduces_the_8x8_scalars(tmp_path):
    from oracle.refbind import ref_available
    if not ref_available():
        pytest.skip("oracle/_ref (the reference's RANLUX gauge field) not built")
    s = json.load(open(os.path.join(GOLD, "ref_mms_scalars_8x8.json")))
    g, q = str(tmp_path / "g.npy"), str(tmp_path / "q.npy")
    subprocess.run([sys.executable, "-c", _CHILD % ROOT, g, q], check=True)   # the reference keeps its state in C globals: own process
    gauge, q_eo = np.load(g), np.load(q)
    V = 8 ** 4
    q_full = np.random.default_rng(20261016).standard_normal((V, 4, 3, 2))    # make_golden_mms.py's full-lattice source
    for name, case in s["cases"].items():
        orc = oracle_for(8, 8, gauge, s["kappa"], s["c_sw"], case)
        A = operator(orc, case["op"], case["g_mu"])
        Q = cplx(q_full if case["op"] == "Q_pm_psi" else q_eo)
        it, reached, P, drops, left = mms_restate.cg_mms_tm(A, Q, case["shifts"], case["max_iter"], case["eps_sq"], case["rel_prec"])
        assert it == case["iters"], name
        assert drops == case["drops"], name
        for k, n in enumerate(case["sol_norms"]):
            assert abs(np.sum(np.abs(P[k]) ** 2) - n) <= 1e-9 * n, (name, k)
