"""CPU: the interface and the fixtures of mixed_cg_mms_tm_nd (no GPU needed).

* tmhip_mixed_cg_mms_tm_nd is declared in include/tmlqcd_hip.h, exported by libtmlqcd_hip.so and mirrored in tmlqcd_amd/hip.py with
  the argument list of the header; mixed_cg_mms_tm_nd is declared in include/tmlqcd_dropin.h and exported by libtmlqcd_dropin.so;
* the options "mms32_fused" and "nd_mms_mixed" are documented in the header and known to tmhip_set_option;
* the operator table still has two doublet rows with solver column TMHIP_S_ND, and only Qtm_pm_ndpsi has an fp32 twin;
* tests/golden/ref_mixed_mms_* (tools/make_golden_mixed_mms.py) satisfy the conditions they were made under.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
GOLD = os.path.join(ROOT, "tests", "golden")


def _exports(so):
    path = os.path.join(LIB, so)
    if not os.path.exists(path):
        pytest.skip("%s not built" % so)
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_symbols_are_exported_and_declared():
    assert "tmhip_mixed_cg_mms_tm_nd" in _exports("libtmlqcd_hip.so")
    assert "mixed_cg_mms_tm_nd" in _exports("libtmlqcd_dropin.so")
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    assert re.search(r"\bint tmhip_mixed_cg_mms_tm_nd\s*\(", hdr)
    assert "mixed_cg_mms_tm_nd.c:69-511" in hdr                      # the reference lines it follows
    dh = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    assert re.search(r"\bint mixed_cg_mms_tm_nd\s*\(spinor \*\*const Pup, spinor \*\*const Pdn, spinor \*const Qup, spinor \*const Qdn, tmlqcd_solver_params \*", dh)


def test_ctypes_signature_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    m = re.search(r"int tmhip_mixed_cg_mms_tm_nd\s*\(([^;]*)\);", hdr)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    kinds = []
    for a in args:
        if "**" in a:
            kinds.append("pp")
        elif "*" in a:
            kinds.append("pd" if a.startswith("const double") else ("pi" if a.startswith("int") else "p"))
        else:
            kinds.append("d" if a.startswith("double") else "i")
    assert kinds == ["p", "pp", "pp", "p", "p", "pd", "i", "i", "d", "i", "i", "pi", "pi", "pi"], kinds
    from tmlqcd_amd import hip
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    want = {"p": vp, "pp": C.POINTER(vp), "pd": C.POINTER(d), "i": i, "d": d, "pi": C.POINTER(i)}
    lib = hip.load_library()
    assert list(lib.tmhip_mixed_cg_mms_tm_nd.argtypes) == [want[k] for k in kinds]
    assert hasattr(hip.Lattice, "mixed_cg_mms_tm_nd")


def test_options_are_documented_and_known():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    ctx = open(os.path.join(ROOT, "tmlqcd_amd", "csrc", "context.hip")).read()
    for name in ("mms32_fused", "nd_mms_mixed"):
        assert '"%s"' % name in hdr, name
        assert 'strcmp(name, "%s")' % name in ctx, name
    assert re.search(r"opt_nd_mms_mixed = 0", ctx)                    # default: nothing changes


def test_operator_table_is_unchanged():
    text = open(os.path.join(ROOT, "tmlqcd_amd", "csrc", "op_table.h")).read()
    rows = re.findall(r"X\((\w+),\s*(\w+),\s*(\w+),\s*(\w+),\s*(\d),\s*([^)]*)\)", text.split("#define TMHIP_ND_OP_TABLE(X)")[1])
    assert {r[1]: int(r[4]) for r in rows} == {"Qtm_pm_ndpsi": 1, "Qsw_pm_ndpsi": 0}
    assert all(r[5].strip() == "TMHIP_S_ND" for r in rows), rows


@pytest.mark.parametrize("tag", ["4x4", "8x8"])
def test_fixture_invariants(tag):
    s = json.load(open(os.path.join(GOLD, "ref_mixed_mms_scalars_%s.json" % tag)))
    n = json.load(open(os.path.join(GOLD, "ref_nd_scalars_%s.json" % tag)))
    for k in ("T", "L", "kappa", "seed", "mubar", "epsbar", "invmaxev"):           # the parameters of ref_nd_*
        assert s[k] == n[k], k
    assert s["shifts"] == json.load(open(os.path.join(GOLD, "ref_nd_scalars_8x8.json")))["cg_mms_tm_nd"]["shifts"]
    runs = s["runs"]
    assert all(r["iters"] > 0 for r in runs)                                        # every run converges
    assert any(r["reliable_updates"] for r in runs)                                 # one with a reliable update
    assert any(r["removals"] for r in runs)                                         # one that removes a shift
    fb = [r for r in runs if r["fallback"]]
    assert len(fb) == 1 and fb[0]["source_norm"] < 1e-4 and not fb[0]["reliable_updates"]
    assert any(r["nshifts"] == 1 for r in runs)
    for r in runs:
        assert not r["got_larger"]
        assert len(r["true_residual_rel"]) == len(r["distance_to_cg_mms_tm_nd"]) == r["nshifts"]
        for j, k in r["reliable_updates"]:
            assert 0 <= j < r["iters"] and 0 <= k < r["nshifts"]
        for j, left in r["removals"]:
            assert j % 10 == 0 and 0 < j <= r["iters"] and 1 <= left < r["nshifts"]
        if not r["fallback"]:
            # shift 0 stops on the iterated fp32 residual before its last x update (mixed_cg_mms_tm_nd.c:307-313): within a decade of the target
            target = r["eps_sq"] if r["rel_prec"] else r["eps_sq"] / r["source_norm"]
            assert r["true_residual_rel"][0] < 10 * target, r["name"]


def test_stored_solutions_4x4():
    s = json.load(open(os.path.join(GOLD, "ref_mixed_mms_scalars_4x4.json")))
    g = np.load(os.path.join(GOLD, "ref_mixed_mms_4x4.npz"))
    ref = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
    assert os.path.getsize(os.path.join(GOLD, "ref_mixed_mms_4x4.npz")) < 640 * 1024
    run = s["runs"][0]
    for k in range(run["nshifts"]):
        for fl in ("up", "dn"):
            a, x = g["%s_%s_%d" % (run["name"], fl, k)], g["cg_mms_%s_%d" % (fl, k)]
            assert a.shape == x.shape == ref["k_s"].shape and a.dtype == np.float64
        du = g["%s_up_%d" % (run["name"], k)] - g["cg_mms_up_%d" % k]
        dd = g["%s_dn_%d" % (run["name"], k)] - g["cg_mms_dn_%d" % k]
        dist = np.sqrt(((du ** 2).sum() + (dd ** 2).sum()) / ((g["cg_mms_up_%d" % k] ** 2).sum() + (g["cg_mms_dn_%d" % k] ** 2).sum()))
        assert abs(dist - run["distance_to_cg_mms_tm_nd"][k]) <= 1e-12 * dist + 1e-18, k
