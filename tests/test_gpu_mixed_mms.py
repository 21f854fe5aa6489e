"""GPU: tmhip_mixed_cg_mms_tm_nd (solver/mixed_cg_mms_tm_nd.c on the device) against the reference's own runs.

tests/golden/ref_mixed_mms_4x4.npz and ref_mixed_mms_scalars_{4x4,8x8}.json were made by the reference's object code
(tools/make_golden_mixed_mms.py) on the links of ref_nd_4x4.npz and the sources of ref_nd32_*.  The reference's fp32 path has another
operation order (half spinors, reduction order), so an update may move by an iteration; per shift the distance to the fp64
multi-shift solution and the true residual, both evaluated in fp64 on the CPU, must stay within FACTOR of what the reference's own
run recorded for that shift.

Measured on an MI355X (device / reference, worst shift of each run): see DESIGN.md section 4, "Mixed multi-shift".
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nd_restate as nd
from tests import mixed_mms_restate as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FACTOR = 4.0          # two fp32 runs that differ only in summation order; a wrong coefficient or a missed update is off by orders of magnitude


class _Fx:
    def __init__(self, L, gauge, q_up, q_dn, s, X=None):
        from oracle.oraclebind import Oracle
        from tmlqcd_amd import Lattice
        self.s, self.L = s, L
        self.lat = Lattice(L, L, L, L, kappa=s["kappa"], mu=0.0)
        self.lat.set_gauge(np.ascontiguousarray(gauge))
        self.lat.set_nd(s["mubar"], s["epsbar"], s["invmaxev"])
        self.orc = Oracle(L, L, L, L, kappa=s["kappa"], mu=0.0, threads=8)
        self.orc.set_gauge(np.ascontiguousarray(gauge))
        self.N = self.lat.Vh
        self.f64, _ = mr.operators(self.orc, s["mubar"], s["epsbar"], s["invmaxev"])
        self.q = (np.ascontiguousarray(q_up), np.ascontiguousarray(q_dn))
        self.qc = (nd.cplx(self.q[0]), nd.cplx(self.q[1]))
        if X is None:   # the fp64 multi-shift solution, computed once: the CPU oracle's (equal to the reference's to 1e-9, test_mixed_mms_restate.py)
            _, X, _, _ = nd.cg_mms_tm_nd(self.f64, self.qc[0], self.qc[1], s["shifts"], s["max_iter"], s["cg_mms_tm_nd"]["eps_sq"], s["cg_mms_tm_nd"]["rel_prec"])
        self.X = X
        self.runs = {r["name"]: r for r in s["runs"]}

    def solve(self, run, max_iter=None, fp64=False):
        """-> (iterations, (updates, removed), active, [(up, dn) float64 arrays per shift])"""
        lat, s = self.lat, self.s
        sh = s["shifts"][:run["nshifts"]]
        qu, qd = lat.field(run["source_scale"] * self.q[0]), lat.field(run["source_scale"] * self.q[1])
        P = [(lat.field(np.full_like(self.q[0], 3.0)), lat.field(np.full_like(self.q[0], -2.0))) for _ in sh]   # zeroed inside
        try:
            if fp64:
                it, _ = lat.cg_mms_tm_nd(qu, qd, sh, max_iter or s["max_iter"], run["eps_sq"], run["rel_prec"], P=P)
                counts = (0, 0)
            else:
                it, counts, _ = lat.mixed_cg_mms_tm_nd(qu, qd, sh, max_iter or s["max_iter"], run["eps_sq"], run["rel_prec"], P=P)
            return it, counts, lat.nd_active_shifts(), [(p[0].download(), p[1].download()) for p in P]
        finally:
            for f in [qu, qd] + [x for p in P for x in p]:
                f.free()

    def residual_rel(self, sol, k):
        u, d = nd.cplx(sol[0]), nd.cplx(sol[1])
        au, ad = self.f64(u, d)
        s2 = self.s["shifts"][k] ** 2
        ru, rd = au + s2 * u - self.qc[0], ad + s2 * d - self.qc[1]
        return float(((np.abs(ru) ** 2).sum() + (np.abs(rd) ** 2).sum()) / ((np.abs(self.qc[0]) ** 2).sum() + (np.abs(self.qc[1]) ** 2).sum()))

    def check_run(self, name):
        run = self.runs[name]
        it, (nrel, nrem), active, sol = self.solve(run)
        print("%d^4 %-10s: %d iterations (reference %d), %d updates (%d), %d removed (%d)"
              % (self.L, name, it, run["iters"], nrel, len(run["reliable_updates"]), nrem, len(run["removals"])))
        ratios = []
        for k in range(run["nshifts"]):
            dist = mr.distance([nd.cplx(sol[k][0]), nd.cplx(sol[k][1])], self.X[k])
            res = self.residual_rel(sol[k], k)
            ratios.append((dist / run["distance_to_cg_mms_tm_nd"][k], res / run["true_residual_rel"][k]))
            print("     shift %d: distance %.3e = %.2f x reference, true residual^2 %.3e = %.2f x reference" % ((k, dist, ratios[-1][0], res, ratios[-1][1])))
        assert it > 0 and mr.count_rule(it, run["iters"]), (it, run["iters"])
        # an update that falls on the boundary of the count rule may land on either side of the last iteration
        assert abs(nrel - len(run["reliable_updates"])) <= (0 if it == run["iters"] else 1), (nrel, run["reliable_updates"])
        assert abs(nrem - len(run["removals"])) <= (0 if it == run["iters"] else 1), (nrem, run["removals"])
        assert active == run["nshifts"] - nrem
        for k, (a, b) in enumerate(ratios):
            assert a <= FACTOR, ("distance", k, a)
            assert b <= FACTOR, ("true residual", k, b)
        return sol


@pytest.fixture(scope="module")
def fx4():
    s = json.load(open(os.path.join(GOLD, "ref_mixed_mms_scalars_4x4.json")))
    f, g = np.load(os.path.join(GOLD, "ref_nd32_4x4.npz")), np.load(os.path.join(GOLD, "ref_mixed_mms_4x4.npz"))
    X = [(nd.cplx(g["cg_mms_up_%d" % k]), nd.cplx(g["cg_mms_dn_%d" % k])) for k in range(len(s["shifts"]))]   # the reference's own fp64 solve
    fx = _Fx(4, np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))["gauge"], f["q_up"], f["q_dn"], s, X)
    yield fx, g
    fx.lat.close()


@pytest.fixture(scope="module")
def fx8(tmp_path_factory):
    from oracle.refbind import ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libtmref.so not built (needs the reference tree at build time): the 8^4 inputs are its random fields")
    out = str(tmp_path_factory.mktemp("mixed_mms") / "in8.npz")
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_nd32 import _child8; _child8(%r)" % (ROOT, out)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    f = np.load(out)
    fx = _Fx(8, f["gauge"], f["q_up"], f["q_dn"], json.load(open(os.path.join(GOLD, "ref_mixed_mms_scalars_8x8.json"))))
    yield fx
    fx.lat.close()


@pytest.mark.parametrize("name", ["rel_1e-14", "rel_1e-8", "abs_1e-9"])
def test_runs_match_the_reference_4x4(fx4, name):
    fx, g = fx4
    sol = fx.check_run(name)
    if name == "rel_1e-14":   # the stored solutions: two fp32 runs, each within its own distance of the fp64 solve
        for k in range(5):
            ref = (nd.cplx(g["%s_up_%d" % (name, k)]), nd.cplx(g["%s_dn_%d" % (name, k)]))
            e = mr.distance([nd.cplx(sol[k][0]), nd.cplx(sol[k][1])], ref)
            assert e <= (1 + FACTOR) * fx.runs[name]["distance_to_cg_mms_tm_nd"][k], (k, e)


@pytest.mark.parametrize("name", ["rel_1e-14", "rel_1e-8", "abs_1e-9"])
def test_runs_match_the_reference_8x8(fx8, name):
    fx8.check_run(name)


def test_one_shift(fx4, fx8):
    fx4[0].check_run("one_shift")
    fx8.check_run("one_shift")


def test_fallback_is_byte_identical_to_cg_mms_tm_nd(fx4):
    fx, _ = fx4
    run = fx.runs["fallback"]
    assert run["fallback"] and run["source_norm"] < 1e-4
    it, counts, active, sol = fx.solve(run)
    it64, _, active64, sol64 = fx.solve(run, fp64=True)
    assert it == it64 and it > 0 and mr.count_rule(it, run["iters"]), (it, it64, run["iters"])
    assert counts[0] == 0 and active == active64 and counts[1] == run["nshifts"] - active64
    for a, b in zip(sol, sol64):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_max_iter_too_small_returns_minus_one(fx4):
    fx, _ = fx4
    it, counts, active, sol = fx.solve(fx.runs["rel_1e-14"], max_iter=8)
    assert it == -1, (it, counts)
    assert all(np.isfinite(a).all() and np.isfinite(b).all() for a, b in sol)


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], (a[:3], b[:3])
    for x, y in zip(a[3], b[3]):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()


def test_cg_batch_fused_form_and_reruns_give_identical_bytes(fx8):
    fx = fx8
    run = fx.runs["rel_1e-14"]
    base = fx.solve(run)
    assert base[0] > 0 and base[1][0] > 0 and base[1][1] > 0      # with reliable updates and removals in it
    _same(base, fx.solve(run))                                    # two runs
    for opt, val, back in (("cg_batch", 1, 4), ("mms32_fused", 0, 1)):
        fx.lat.set_option(opt, val)
        try:
            _same(base, fx.solve(run))
        finally:
            fx.lat.set_option(opt, back)
    fx.lat.set_option("cg_batch", 1)
    fx.lat.set_option("mms32_fused", 0)
    try:
        _same(base, fx.solve(run))
    finally:
        fx.lat.set_option("cg_batch", 4)
        fx.lat.set_option("mms32_fused", 1)
