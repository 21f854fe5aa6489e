"""CPU: the NumPy restatement of mixed_cg_mms_tm_nd (tests/mixed_mms_restate.py) against the reference's own runs.

tests/golden/ref_mixed_mms_* were made by the reference's object code (tools/make_golden_mixed_mms.py).  The restatement runs on
the CPU oracle's Qtm_pm_ndpsi rounded to float32 once per application, which is not the reference's fp32 operator (half spinors,
another operation order): iteration counts are held to the rule of tests/test_gpu_nd32.py, the numbers of reliable updates and of
removed shifts must be the reference's.  What passes here is the yardstick of the device solver on the shapes without a reference run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nd_restate as nd
from tests import mixed_mms_restate as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _check(s, gauge, q_up, q_dn, L):
    from oracle.oraclebind import Oracle
    orc = Oracle(L, L, L, L, kappa=s["kappa"], mu=0.0, threads=8)
    orc.set_gauge(np.ascontiguousarray(gauge))
    f64, f32 = mr.operators(orc, s["mubar"], s["epsbar"], s["invmaxev"])
    qu, qd = nd.cplx(np.ascontiguousarray(q_up)), nd.cplx(np.ascontiguousarray(q_dn))
    for run in s["runs"]:
        ret, P, info, X = mr.restate_run(f64, f32, qu, qd, s["shifts"], run, s["max_iter"])
        dist = [mr.distance(P[k], X[k]) for k in range(run["nshifts"])]
        print("%d^4 %-10s ret %d (reference %d) updates %s removals %s" % (L, run["name"], ret, run["iters"], info["updates"], info["removals"]))
        print("     distance / reference's: %s" % ["%.2f" % (a / b) if b else "-" for a, b in zip(dist, run["distance_to_cg_mms_tm_nd"])])
        assert info["fallback"] == run["fallback"], run["name"]
        assert ret > 0 and mr.count_rule(ret, run["iters"]), (run["name"], ret, run["iters"])
        if run["fallback"]:
            continue
        assert len(info["updates"]) == len(run["reliable_updates"]), (run["name"], info["updates"], run["reliable_updates"])
        assert len(info["removals"]) == len(run["removals"]), (run["name"], info["removals"], run["removals"])
        assert info["active"] == run["nshifts"] - len(run["removals"])


def test_restatement_reproduces_the_reference_runs_4x4():
    s = json.load(open(os.path.join(GOLD, "ref_mixed_mms_scalars_4x4.json")))
    f = np.load(os.path.join(GOLD, "ref_nd32_4x4.npz"))
    _check(s, np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))["gauge"], f["q_up"], f["q_dn"], 4)


def test_restatement_reproduces_the_stored_solutions_4x4():
    """the run whose solutions are stored: the restatement's P against the reference's P, both fp32 runs -- within the sum of their
    distances to the fp64 solve"""
    from oracle.oraclebind import Oracle
    s = json.load(open(os.path.join(GOLD, "ref_mixed_mms_scalars_4x4.json")))
    f, g = np.load(os.path.join(GOLD, "ref_nd32_4x4.npz")), np.load(os.path.join(GOLD, "ref_mixed_mms_4x4.npz"))
    orc = Oracle(4, 4, 4, 4, kappa=s["kappa"], mu=0.0, threads=8)
    orc.set_gauge(np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))["gauge"]))
    f64, f32 = mr.operators(orc, s["mubar"], s["epsbar"], s["invmaxev"])
    run = s["runs"][0]
    ret, P, info, X = mr.restate_run(f64, f32, nd.cplx(f["q_up"]), nd.cplx(f["q_dn"]), s["shifts"], run, s["max_iter"])
    for k in range(run["nshifts"]):
        ref = (nd.cplx(g["%s_up_%d" % (run["name"], k)]), nd.cplx(g["%s_dn_%d" % (run["name"], k)]))
        x64 = (nd.cplx(g["cg_mms_up_%d" % k]), nd.cplx(g["cg_mms_dn_%d" % k]))
        assert mr.distance(X[k], x64) < 1e-9, k                        # the oracle's fp64 solve is the reference's
        assert mr.distance(P[k], ref) <= mr.distance(P[k], x64) + run["distance_to_cg_mms_tm_nd"][k], k


def test_restatement_reproduces_the_reference_runs_8x8(tmp_path):
    from oracle.refbind import ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libtmref.so not built (needs the reference tree at build time): the 8^4 inputs are its random fields")
    out = str(tmp_path / "in8.npz")
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_nd32 import _child8; _child8(%r)" % (ROOT, out)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    f = np.load(out)
    s = json.load(open(os.path.join(GOLD, "ref_mixed_mms_scalars_8x8.json")))
    _check(s, f["gauge"], f["q_up"], f["q_dn"], 8)
