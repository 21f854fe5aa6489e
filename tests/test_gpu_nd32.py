"""GPU: the fp32 doublet (operator/tm_operators_nd_32.c) and rg_mixed_cg_her_nd (solver/rg_mixed_cg_her_nd.c) against the
reference's own runs.

tests/golden/ref_nd32_4x4.npz and ref_nd32_scalars_{4x4,8x8}.json were made by the reference's object code (half-spinor build,
tools/make_golden_nd32.py) on the links of ref_nd_4x4.npz.  The fp32 reference path has another operation order (half spinors,
reduction order), so the operators are held to the project's fp32 bounds and the restart points of the solver may move by a few
iterations; the solution must agree to fp64-solver accuracy and the true residual, evaluated in fp64 on the CPU, must meet eps_sq.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import nd_restate as nd
from tests.hostprog import run_child

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL32 = 2e-6          # the fp32 bound of tests/test_gpu_mixed.py


def rel(a, b):
    """max |a - b| / max |b| over both flavours of a pair (the `rel` of tests/test_gpu_mixed.py)"""
    a, b = np.concatenate([np.ravel(x) for x in a]).astype(np.float64), np.concatenate([np.ravel(x) for x in b]).astype(np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def count_rule(it, ref):
    return abs(it - ref) <= max(3, ref // 8)          # the rule of the single-flavour solver (test_gpu_mixed.py)


class _Fx:
    def __init__(self, T, L, gauge, q_up, q_dn, s):
        from oracle.oraclebind import Oracle
        from tmlqcd_amd import Lattice
        self.s = s
        self.lat = Lattice(T, L, L, L, kappa=s["kappa"], mu=0.0)
        self.lat.set_gauge(np.ascontiguousarray(gauge))
        self.lat.set_nd(s["mubar"], s["epsbar"], s["invmaxev"])
        self.orc = Oracle(T, L, L, L, kappa=s["kappa"], mu=0.0, threads=8)
        self.orc.set_gauge(np.ascontiguousarray(gauge))
        self.N = self.lat.Vh
        self.H = nd.hop_over(self.orc.Hopping_Matrix, self.N)
        self.q = (np.ascontiguousarray(q_up), np.ascontiguousarray(q_dn))
        self.qnorm = float((self.q[0] ** 2).sum() + (self.q[1] ** 2).sum())

    def residual(self, u, d):
        """|Q - Qtm_pm_ndpsi x|^2 in fp64 on the CPU"""
        au, ad = nd.Qtm_pm_ndpsi(self.H, nd.cplx(u), nd.cplx(d), self.s["mubar"], self.s["epsbar"], self.s["invmaxev"])
        return float(((nd.real(au) - self.q[0]) ** 2).sum() + ((nd.real(ad) - self.q[1]) ** 2).sum())

    def solve(self, delta, max_iter=None, eps_sq=None, rel_prec=None):
        lat, s = self.lat, self.s
        qu, qd = lat.field(self.q[0]), lat.field(self.q[1])
        pu, pd = lat.field(np.full_like(self.q[0], 3.0)), lat.field(np.full_like(self.q[0], -2.0))   # zero start: P is zeroed inside
        try:
            it, counts = lat.rg_mixed_cg_her_nd(pu, pd, qu, qd, max_iter or s["max_iter"], eps_sq or s["eps_sq"],
                                                s["rel_prec"] if rel_prec is None else rel_prec, self.N, delta=delta)
            return it, counts, pu.download(), pd.download()
        finally:
            for f in (qu, qd, pu, pd):
                f.free()


@pytest.fixture(scope="module")
def fx4():
    f = np.load(os.path.join(GOLD, "ref_nd32_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_nd32_scalars_4x4.json")))
    gauge = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))["gauge"]
    fx = _Fx(4, 4, gauge, f["q_up"], f["q_dn"], s)
    yield fx, f, s
    fx.lat.close()


def test_assign_to_32_images_are_bit_equal(fx4):
    fx, f, s = fx4
    lat = fx.lat
    for fl in ("up", "dn"):
        d64, d32 = lat.field(np.ascontiguousarray(f["q_" + fl])), lat.field32()
        lat.assign_to_32(d32, d64, fx.N)
        assert np.array_equal(d32.download(), f["q32_" + fl]), fl
        d64.free(); d32.free()


@pytest.mark.parametrize("fused", [1, 0])
def test_operators_match_reference(fx4, fused):
    fx, f, s = fx4
    lat = fx.lat
    lat.set_option("nd_fused", fused)
    mu, eps = s["mubar"], s["epsbar"]
    ks, kc = lat.field32(np.ascontiguousarray(f["q32_up"])), lat.field32(np.ascontiguousarray(f["q32_dn"]))
    ls, lc, es, ec = lat.field32(), lat.field32(), lat.field32(), lat.field32()
    try:
        lat.Qtm_pm_ndpsi_32(ls, lc, ks, kc)
        e = rel((ls.download(), lc.download()), (f["Qtm_pm_ndpsi_32_s"], f["Qtm_pm_ndpsi_32_c"]))
        assert e < 4 * TOL32, ("Qtm_pm_ndpsi_32", e)
        lat.M_ee_inv_ndpsi_32(es, ec, ks, kc, mu, eps)
        e = rel((es.download(), ec.download()), (f["M_ee_inv_ndpsi_32_s"], f["M_ee_inv_ndpsi_32_c"]))
        assert e < TOL32, ("M_ee_inv_ndpsi_32", e)
        js, jc = lat.field32(np.ascontiguousarray(f["Qtm_pm_ndpsi_32_s"])), lat.field32(np.ascontiguousarray(f["Qtm_pm_ndpsi_32_c"]))
        lat.M_oo_sub_g5_ndpsi_32(es, ec, ks, kc, js, jc, mu, eps)                 # the fixture's j is its Qtm_pm_ndpsi_32 pair
        e = rel((es.download(), ec.download()), (f["M_oo_sub_g5_ndpsi_32_s"], f["M_oo_sub_g5_ndpsi_32_c"]))
        assert e < TOL32, ("M_oo_sub_g5_ndpsi_32", e)
        lat.Qtm_pm_ndpsi_32(ks, kc, ks, kc)                                       # l == k
        e = rel((ks.download(), kc.download()), (f["Qtm_pm_ndpsi_32_s"], f["Qtm_pm_ndpsi_32_c"]))
        assert e < 4 * TOL32, ("Qtm_pm_ndpsi_32, l == k", e)
        js.free(); jc.free()
    finally:
        lat.set_option("nd_fused", 1)
        for x in (ks, kc, ls, lc, es, ec):
            x.free()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("delta", [0.1, 0.01, 1e-3, 1e-5, 0.5])
def test_rg_mixed_cg_her_nd_against_reference_run(fx4, delta, fused):
    fx, f, s = fx4
    run = {r["delta"]: r for r in s["rg_mixed_cg_her_nd"]}[delta]
    fx.lat.set_option("nd_fused", fused)
    try:
        it, (n_out, n_sp, n_dp), u, d = fx.solve(delta)
    finally:
        fx.lat.set_option("nd_fused", 1)
    print("delta %g nd_fused %d: %d = %d + %d + %d (reference %s)" % (delta, fused, it, n_out, n_sp, n_dp, run["iters"]))
    if run["iters"] < 0:                                  # delta 0.5: N_outer used up in the fail-safe branch, like the reference
        assert it == -1 and n_dp > 0, (it, n_out, n_sp, n_dp)
        return
    assert it > 0 and it == n_out + n_sp + n_dp, (it, n_out, n_sp, n_dp)
    assert count_rule(it, run["iters"]), (it, run)
    e = rel((u, d), (f["rg_up_%g" % delta], f["rg_dn_%g" % delta]))
    res = fx.residual(u, d) / fx.qnorm
    print("   solution vs fixture %.3e, true residual^2 / |Q|^2 %.3e" % (e, res))
    assert e < 1e-8, e
    assert res <= s["eps_sq"], res


# ---------------------------------------------------------------- 8^4: the scalars of the reference's runs
def _child8(out):
    """Runs in its own process (the reference keeps one lattice in C globals): the 8^4 inputs of tools/make_golden_nd32.py."""
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    s = json.load(open(os.path.join(GOLD, "ref_nd32_scalars_8x8.json")))
    r = RefLattice(s["T"], s["L"], s["L"], s["L"], kappa=s["kappa"], mu=0.0, nfields=8)
    r.random_fields(s["seed"])
    for k in (1, 2):
        r.lib.tmref_random_spinor_eo(k)
    N = r.V // 2
    np.savez(out, gauge=r.gauge(), q_up=r.spinor(1, N), q_dn=r.spinor(2, N))


@pytest.fixture(scope="module")
def fx8(tmp_path_factory):
    from oracle.refbind import ref_available
    if not ref_available():
        pytest.skip("oracle/_ref/libtmref.so not built (needs the reference tree at build time): the 8^4 inputs are its random fields")
    out = str(tmp_path_factory.mktemp("nd32") / "in8.npz")
    code = "import sys; sys.path.insert(0, %r); from tests.test_gpu_nd32 import _child8; _child8(%r)" % (ROOT, out)
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    f = np.load(out)
    s = json.load(open(os.path.join(GOLD, "ref_nd32_scalars_8x8.json")))
    fx = _Fx(8, 8, f["gauge"], f["q_up"], f["q_dn"], s)
    yield fx, s
    fx.lat.close()


def test_rg_mixed_cg_her_nd_8x8_counts(fx8):
    fx, s = fx8
    for run in s["rg_mixed_cg_her_nd"]:
        it, (n_out, n_sp, n_dp), u, d = fx.solve(run["delta"])
        print("delta %g: %d = %d + %d + %d (reference %s)" % (run["delta"], it, n_out, n_sp, n_dp, run["iters"]))
        if run["iters"] < 0:
            assert it == -1 and n_dp > 0, (run, it, n_out, n_sp, n_dp)
            continue
        assert it > 0 and it == n_out + n_sp + n_dp, (run, it, n_out, n_sp, n_dp)
        assert count_rule(it, run["iters"]), (run, it)
        assert fx.residual(u, d) / fx.qnorm <= s["eps_sq"]


def test_rg_mixed_cg_her_nd_8x8_iteration_cap_and_absolute_precision(fx8):
    fx, s = fx8
    it, counts, u, d = fx.solve(0.1, max_iter=10)         # max_iter smaller than needed: -1 like rg_mixed_cg_her_nd.c:312-313
    assert it == -1, (it, counts)
    it, (n_out, n_sp, n_dp), u, d = fx.solve(0.1, eps_sq=1e-14, rel_prec=0)      # rel_prec = 0: target_eps_sq = eps_sq
    res = fx.residual(u, d)
    print("rel_prec 0: %d = %d + %d + %d, true residual^2 %.3e" % (it, n_out, n_sp, n_dp, res))
    assert it > 0 and it == n_out + n_sp + n_dp
    assert res <= 1e-14, res


# ---------------------------------------------------------------- drop-in
@pytest.mark.parametrize("mode", ["lazy", "resident"])
def test_dropin_symbols_equal_the_core_calls(mode):
    r = run_child("nd32_dropin_child.py", mode)
    assert r["Qtm_pm_ndpsi_32_bit_equal"] and r["M_ee_inv_ndpsi_32_bit_equal"] and r["M_oo_sub_g5_ndpsi_32_bit_equal"], r
    assert r["Qtm_pm_ndpsi_32_aliased_bit_equal"], r
    assert r["rg_iters"] == r["rg_iters_core"] and r["rg_iters"] > 0, r
    assert r["rg_solution_bit_equal"], r
