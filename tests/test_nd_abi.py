"""CPU: the non-degenerate doublet's interface and fixtures (no GPU needed).

* every tmhip_*nd* entry point is exported by libtmlqcd_hip.so, every reference-named doublet symbol is declared in
  include/tmlqcd_dropin.h and exported by libtmlqcd_dropin.so;
* tests/golden/ref_nd_4x4.npz is self-consistent: the NumPy restatement of M_ee_inv_ndpsi / M_oo_sub_g5_ndpsi
  (operator/tm_operators_nd.c:639-757, oracle/nd_restate.py), composed with the reference's own Hopping_Matrix (oracle/_ref/libtmref.so,
  through oracle/refbind.py), reproduces the fixture's Qtm_pm_ndpsi, Qtm_ndpsi and Qtm_dagger_ndpsi.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle.nd_restate import cplx as _c, m_ee_inv, m_oo_sub_g5, real as _r

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
GOLD = os.path.join(ROOT, "tests", "golden")

CORE = ["tmhip_set_nd", "tmhip_M_ee_inv_ndpsi", "tmhip_M_oo_sub_g5_ndpsi", "tmhip_Qtm_ndpsi", "tmhip_Qtm_dagger_ndpsi",
        "tmhip_Qtm_pm_ndpsi", "tmhip_H_eo_tm_ndpsi", "tmhip_cg_her_nd", "tmhip_cg_mms_tm_nd", "tmhip_nd_active_shifts"]
DROPIN = ["Qtm_ndpsi", "Qtm_dagger_ndpsi", "Qtm_pm_ndpsi", "M_ee_inv_ndpsi", "H_eo_tm_ndpsi", "mul_one_pm_itau2",
          "cg_her_nd", "cg_mms_tm_nd"]


def _exports(so):
    path = os.path.join(LIB, so)
    if not os.path.exists(path):
        pytest.skip("%s not built" % so)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_core_entry_points_are_exported():
    missing = [n for n in CORE if n not in _exports("libtmlqcd_hip.so")]
    assert not missing, missing


def test_core_entry_points_are_declared():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    missing = [n for n in CORE if not re.search(r"\b%s\s*\(" % n, hdr)]
    assert not missing, missing


def test_dropin_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    undeclared = [n for n in DROPIN if not re.search(r"\b%s\s*\(" % n, hdr)]
    assert not undeclared, undeclared
    missing = [n for n in DROPIN if n not in _exports("libtmlqcd_dropin.so")]
    assert not missing, missing


def test_fixture_scalars_describe_the_runs():
    s = json.load(open(os.path.join(GOLD, "ref_nd_scalars_4x4.json")))
    assert s["invmaxev"] != 1.0 and s["mubar"] != 0.0 and s["epsbar"] != 0.0
    assert s["cg_her_nd"]["iters"] > 0
    m = s["cg_mms_tm_nd"]
    assert len(m["shifts"]) >= 4 and m["iters"] > 0
    assert m["drops"], "the fixture must exercise the shift drop of cg_mms_tm_nd.c:158-167"
    s8 = json.load(open(os.path.join(GOLD, "ref_nd_scalars_8x8.json")))
    assert s8["cg_her_nd"]["iters"] > 0 and s8["cg_mms_tm_nd"]["iters"] > 0


def _child():
    """Runs in its own process (the reference keeps one lattice in C globals)."""
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    f = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_nd_scalars_4x4.json")))
    r = RefLattice(4, 4, 4, 4, kappa=s["kappa"], mu=0.0, nfields=8)
    r.gauge()[:] = f["gauge"]
    r.mark_gauge_dirty()
    N = r.V // 2

    def H(ieo, x):
        r.spinor(0, N)[:] = _r(x)
        r.lib.Hopping_Matrix(ieo, r.sp(1), r.sp(0))
        return _c(r.spinor(1, N).copy())

    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    ks, kc = _c(f["k_s"]), _c(f["k_c"])
    # Qtm_pm_ndpsi, :195-238
    d2, d3 = m_ee_inv(H(0, kc), H(0, ks), mb, eb)
    e2, e3 = m_oo_sub_g5(kc, ks, H(1, d2), H(1, d3), -mb, -eb)
    d5, d4 = m_ee_inv(H(0, e2), H(0, e3), -mb, eb)
    ls, lc = m_oo_sub_g5(e3, e2, H(1, d4), H(1, d5), -mb, -eb)
    pm = (c * c * ls, c * c * lc)
    # Qtm_ndpsi, :68-89
    x3, x2 = m_ee_inv(H(0, ks), H(0, kc), mb, eb)
    q = m_oo_sub_g5(ks, kc, H(1, x3), H(1, x2), -mb, -eb)
    # Qtm_dagger_ndpsi, :130-152
    y2, y3 = m_ee_inv(H(0, kc), H(0, ks), mb, eb)
    qd = m_oo_sub_g5(ks, kc, H(1, y3), H(1, y2), mb, -eb)
    errs = {}
    for name, (a, b) in (("Qtm_pm_ndpsi", pm), ("Qtm_ndpsi", (c * q[0], c * q[1])), ("Qtm_dagger_ndpsi", (c * qd[0], c * qd[1]))):
        ref = np.concatenate([f[name + "_s"].ravel(), f[name + "_c"].ravel()])
        got = np.concatenate([_r(a).ravel(), _r(b).ravel()])
        errs[name] = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    # the site-local blocks alone
    js, jc = _c(f["j_s"]), _c(f["j_c"])
    for name, (a, b) in (("M_ee_inv_ndpsi", m_ee_inv(ks, kc, mb, eb)), ("M_oo_sub_g5_ndpsi", m_oo_sub_g5(ks, kc, js, jc, mb, eb))):
        ref = np.concatenate([f[name + "_s"].ravel(), f[name + "_c"].ravel()])
        errs[name] = float(np.linalg.norm(np.concatenate([_r(a).ravel(), _r(b).ravel()]) - ref) / np.linalg.norm(ref))
    print(json.dumps(errs))


def test_fixture_matches_numpy_composition_with_reference_hopping():
    sys.path.insert(0, ROOT)
    from oracle.refbind import ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libtmref.so not built (needs the reference tree at build time)")
    code = "import sys; sys.path.insert(0, %r); from tests.test_nd_abi import _child; _child()" % ROOT
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    errs = json.loads(out.stdout.strip().splitlines()[-1])
    bad = {k: v for k, v in errs.items() if not v < 1e-13}
    assert not bad, errs
