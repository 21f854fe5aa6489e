"""CPU: the interface and the fixtures of the fp32 doublet and of rg_mixed_cg_her_nd (no GPU needed).

* every new tmhip_* entry point is declared in include/tmlqcd_hip.h, exported by libtmlqcd_hip.so and mirrored in tmlqcd_amd/hip.py;
  every reference-named symbol is declared in include/tmlqcd_dropin.h and exported by libtmlqcd_dropin.so;
* the operator table gives Qtm_pm_ndpsi an fp32 twin and Qsw_pm_ndpsi none;
* tests/golden/ref_nd32_* (tools/make_golden_nd32.py) describe their runs.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
GOLD = os.path.join(ROOT, "tests", "golden")

CORE = ["tmhip_Qtm_pm_ndpsi_32", "tmhip_M_ee_inv_ndpsi_32", "tmhip_M_oo_sub_g5_ndpsi_32", "tmhip_rg_mixed_cg_her_nd"]
DROPIN = ["Qtm_pm_ndpsi_32", "M_ee_inv_ndpsi_32", "M_oo_sub_g5_ndpsi_32", "rg_mixed_cg_her_nd"]
CONVERGING = [0.1, 0.01, 1e-3, 1e-5]


def _exports(so):
    path = os.path.join(LIB, so)
    if not os.path.exists(path):
        pytest.skip("%s not built" % so)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_core_entry_points_are_exported():
    missing = [n for n in CORE if n not in _exports("libtmlqcd_hip.so")]
    assert not missing, missing


def test_core_entry_points_are_declared_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    missing = [n for n in CORE if not re.search(r"\b%s\s*\(" % n, hdr)]
    assert not missing, missing
    py = open(os.path.join(ROOT, "tmlqcd_amd", "hip.py")).read()
    unmirrored = [n for n in CORE if '"%s":' % n not in py]
    assert not unmirrored, unmirrored


def test_dropin_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    undeclared = [n for n in DROPIN if not re.search(r"\b%s\s*\(" % n, hdr)]
    assert not undeclared, undeclared
    missing = [n for n in DROPIN if n not in _exports("libtmlqcd_dropin.so")]
    assert not missing, missing


def test_headers_no_longer_deny_the_fp32_twins():
    assert "no fp32 twins" not in open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    assert "Not here: the fp32 twins" not in open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()


def test_operator_table_has_the_fp32_twin_of_the_twisted_mass_doublet_only():
    text = open(os.path.join(ROOT, "tmlqcd_amd", "csrc", "op_table.h")).read()
    rows = re.findall(r"X\((\w+),\s*(\w+),\s*(\w+),\s*(\w+),\s*(\d),", text.split("#define TMHIP_ND_OP_TABLE(X)")[1])
    fp32 = {name: int(col) for _, name, _, _, col in rows}
    assert fp32 == {"Qtm_pm_ndpsi": 1, "Qsw_pm_ndpsi": 0}, fp32


@pytest.mark.parametrize("tag", ["4x4", "8x8"])
def test_fixture_scalars_describe_the_runs(tag):
    s = json.load(open(os.path.join(GOLD, "ref_nd32_scalars_%s.json" % tag)))
    n = json.load(open(os.path.join(GOLD, "ref_nd_scalars_%s.json" % tag)))
    for k in ("T", "L", "kappa", "seed", "mubar", "epsbar", "invmaxev"):           # the parameters of ref_nd_*
        assert s[k] == n[k], k
    assert (s["max_iter"], s["eps_sq"], s["rel_prec"]) == (5000, 1e-20, 1)
    assert s["cg_her_nd"]["iters"] > 0
    assert 0 < s["op32_vs_op64"] < 4e-7                                             # fp32 rounding, not a different operator
    runs = {r["delta"]: r for r in s["rg_mixed_cg_her_nd"]}
    assert sorted(runs) == sorted(CONVERGING + [0.5])
    for delta in CONVERGING:
        r = runs[delta]
        assert r["iters"] > 0 and r["iters"] == r["iter_out"] + r["iter_in_sp"] + r["iter_in_dp"], r
        assert r["iter_in_dp"] == 0 and not r["switched_to_dp"], r
        assert r["true_residual_rel"] <= s["eps_sq"] and r["distance_to_cg_her_nd"] < 1e-9, r
        assert r["iters"] > s["cg_her_nd"]["iters"]                                 # restarts cost iterations, they do not save any
    assert runs[0.5]["iters"] == -1 and runs[0.5]["switched_to_dp"]                 # N_outer used up: the fail-safe branch, then -1
    assert runs[1e-5]["iter_out"] < runs[0.1]["iter_out"]                           # a smaller delta restarts less often


def test_fixture_fields_are_consistent():
    f = np.load(os.path.join(GOLD, "ref_nd32_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_nd32_scalars_4x4.json")))
    N = s["T"] * s["L"] ** 3 // 2
    for fl in ("up", "dn"):
        assert f["q_" + fl].shape == (N, 4, 3, 2) and f["q_" + fl].dtype == np.float64
        assert np.array_equal(f["q32_" + fl], f["q_" + fl].astype(np.float32))      # assign_to_32 rounds to nearest
    for name in ("Qtm_pm_ndpsi_32", "M_ee_inv_ndpsi_32", "M_oo_sub_g5_ndpsi_32"):
        for fl in ("s", "c"):
            a = f["%s_%s" % (name, fl)]
            assert a.shape == (N, 4, 3, 2) and a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0
    for delta in CONVERGING:
        for fl in ("up", "dn"):
            a, x = f["rg_%s_%g" % (fl, delta)], f["cg_her_nd_" + fl]
            assert np.abs(a - x).max() < 1e-8 * np.abs(x).max(), (delta, fl)
    assert "rg_up_0.5" not in f.files
