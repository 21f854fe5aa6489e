"""GPU: the non-degenerate twisted-mass doublet (operator/tm_operators_nd.c, solver/cg_her_nd.c, solver/cg_mms_tm_nd.c).

Pinned by tests/golden/ref_nd_4x4.npz (made by the reference's own object code, tools/make_golden_nd.py) in both forms of
the operator: the doublet stencil with the fused flavour mixing ("nd_fused" 1) and two single-flavour stencils plus a
mixing pass ("nd_fused" 0).
"""
import json
import os

import numpy as np
import pytest

from tests.hostprog import run_child
from tests.util import TOL, random_gauge, random_spinor, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
OPS = ("Qtm_ndpsi", "Qtm_dagger_ndpsi", "Qtm_pm_ndpsi")


def _pair_err(a, b, ra, rb):
    num = np.sqrt(np.sum((a - ra) ** 2) + np.sum((b - rb) ** 2))
    return num / np.sqrt(np.sum(ra ** 2) + np.sum(rb ** 2))


@pytest.fixture(scope="module")
def fx():
    from tmlqcd_amd import Lattice
    f = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_nd_scalars_4x4.json")))
    lat = Lattice(4, 4, 4, 4, kappa=s["kappa"], mu=0.0)
    lat.set_gauge(np.ascontiguousarray(f["gauge"]))
    lat.set_nd(s["mubar"], s["epsbar"], s["invmaxev"])
    yield lat, f, s
    lat.close()


@pytest.mark.parametrize("fused", [1, 0])
def test_operators_match_reference(fx, fused):
    lat, f, s = fx
    lat.set_option("nd_fused", fused)
    ks, kc = lat.field(np.ascontiguousarray(f["k_s"])), lat.field(np.ascontiguousarray(f["k_c"]))
    js, jc = lat.field(np.ascontiguousarray(f["j_s"])), lat.field(np.ascontiguousarray(f["j_c"]))
    ls, lc = lat.field(), lat.field()
    for name in OPS:
        getattr(lat, name)(ls, lc, ks, kc)
        assert _pair_err(ls.download(), lc.download(), f[name + "_s"], f[name + "_c"]) < TOL, name
    lat.M_ee_inv_ndpsi(ls, lc, ks, kc, s["mubar"], s["epsbar"])
    assert _pair_err(ls.download(), lc.download(), f["M_ee_inv_ndpsi_s"], f["M_ee_inv_ndpsi_c"]) < TOL
    lat.M_oo_sub_g5_ndpsi(ls, lc, ks, kc, js, jc, s["mubar"], s["epsbar"])
    assert _pair_err(ls.download(), lc.download(), f["M_oo_sub_g5_ndpsi_s"], f["M_oo_sub_g5_ndpsi_c"]) < TOL
    for ieo in (0, 1):
        lat.H_eo_tm_ndpsi(ls, lc, ks, kc, ieo)
        assert _pair_err(ls.download(), lc.download(), f["H_eo_tm_ndpsi_%d_s" % ieo], f["H_eo_tm_ndpsi_%d_c" % ieo]) < TOL, ieo
    # l == k, as tm_operators_nd.c:188 allows for Qtm_pm_ndpsi; H_eo_tm_ndpsi hops into scratch first as well
    lat.Qtm_pm_ndpsi(ks, kc, ks, kc)
    assert _pair_err(ks.download(), kc.download(), f["Qtm_pm_ndpsi_s"], f["Qtm_pm_ndpsi_c"]) < TOL
    ks.upload(np.ascontiguousarray(f["k_s"])); kc.upload(np.ascontiguousarray(f["k_c"]))
    lat.H_eo_tm_ndpsi(ks, kc, ks, kc, 0)
    assert _pair_err(ks.download(), kc.download(), f["H_eo_tm_ndpsi_0_s"], f["H_eo_tm_ndpsi_0_c"]) < TOL
    lat.set_option("nd_fused", 1)


@pytest.mark.parametrize("fused", [1, 0])
def test_cg_her_nd_matches_reference(fx, fused):
    lat, f, s = fx
    lat.set_option("nd_fused", fused)
    c = s["cg_her_nd"]
    qs, qc = lat.field(np.ascontiguousarray(f["k_s"])), lat.field(np.ascontiguousarray(f["k_c"]))
    pu, pd = lat.field().zero(), lat.field().zero()
    it = lat.cg_her_nd(pu, pd, qs, qc, c["max_iter"], c["eps_sq"], c["rel_prec"], lat.Vh)
    assert abs(it - c["iters"]) <= 1, (it, c["iters"])
    assert _pair_err(pu.download(), pd.download(), f["cg_her_nd_up"], f["cg_her_nd_dn"]) < 1e-9
    # a non-zero start (cg_her_nd.c:93-104) converges to the same solution
    it2 = lat.cg_her_nd(pu, pd, qs, qc, c["max_iter"], c["eps_sq"], c["rel_prec"], lat.Vh)
    assert 0 < it2 < it
    assert _pair_err(pu.download(), pd.download(), f["cg_her_nd_up"], f["cg_her_nd_dn"]) < 1e-9
    lat.set_option("nd_fused", 1)


@pytest.mark.parametrize("fused", [1, 0])
def test_cg_mms_tm_nd_matches_reference_with_dropped_shifts(fx, fused):
    lat, f, s = fx
    lat.set_option("nd_fused", fused)
    m = s["cg_mms_tm_nd"]
    qs, qc = lat.field(np.ascontiguousarray(f["k_s"])), lat.field(np.ascontiguousarray(f["k_c"]))
    it, P = lat.cg_mms_tm_nd(qs, qc, m["shifts"], m["max_iter"], m["eps_sq"], m["rel_prec"])
    assert abs(it - m["iters"]) <= 1, (it, m["iters"])
    assert m["drops"] and lat.nd_active_shifts() == len(m["shifts"]) - len(m["drops"])
    for k, (u, d) in enumerate(P):
        assert _pair_err(u.download(), d.download(), f["cg_mms_up_%d" % k], f["cg_mms_dn_%d" % k]) < 1e-9, k
    lat.set_option("nd_fused", 1)


def _lat16(seed):
    from tmlqcd_amd import Lattice
    L = 16
    lat = Lattice(L, L, L, L, kappa=0.1373, mu=0.0, theta=(1.0, 0.0, 0.0, 0.0))
    lat.set_gauge(random_gauge(seed, L ** 4))
    lat.set_nd(0.1375, 0.1175, 0.83)
    return lat


def test_qtm_pm_ndpsi_is_hermitian_16():
    lat = _lat16(71)
    N = lat.Vh
    xs, xc, ys, yc = (lat.field(random_spinor(s, N)) for s in (1, 2, 3, 4))
    a_s, a_c, b_s, b_c = lat.field(), lat.field(), lat.field(), lat.field()
    lat.Qtm_pm_ndpsi(a_s, a_c, ys, yc)
    lat.Qtm_pm_ndpsi(b_s, b_c, xs, xc)
    lhs = lat.scalar_prod_r(xs, a_s, N) + lat.scalar_prod_r(xc, a_c, N)
    rhs = lat.scalar_prod_r(b_s, ys, N) + lat.scalar_prod_r(b_c, yc, N)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    lat.close()


def test_doublet_stencil_equals_two_single_flavour_stencils_in_every_variant():
    lat = _lat16(72)
    N = lat.Vh
    ks, kc = lat.field(random_spinor(5, N)), lat.field(random_spinor(6, N))
    ls, lc = lat.field(), lat.field()
    variants = [{}] + [{"block": b} for b in (64, 256)] + [{"xcd": x} for x in (0, 1, 3, 4)] + [{"hopsplit": 0}, {"gauge_cache": 0}]
    for v in variants:
        for k, val in v.items():
            lat.set_option(k, val)
        out = {}
        for fused in (1, 0):
            lat.set_option("nd_fused", fused)
            for name in OPS:
                getattr(lat, name)(ls, lc, ks, kc)
                out[(fused, name)] = (ls.download(), lc.download())
            lat.H_eo_tm_ndpsi(ls, lc, ks, kc, 1)
            out[(fused, "H_eo")] = (ls.download(), lc.download())
        for name in OPS + ("H_eo",):
            a, b = out[(1, name)], out[(0, name)]
            assert _pair_err(a[0], a[1], b[0], b[1]) < 1e-14, (v, name)
        for k in v:
            lat.set_option(k, {"block": 0, "xcd": 2, "hopsplit": -1, "gauge_cache": -1}[k])
    lat.set_option("nd_fused", 1)
    lat.close()


def test_t_split_context_is_refused():
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    lat = Lattice(4, 4, 4, 4, kappa=0.125, nproc_t=2, proc_t=0)
    a, b, c, d = lat.field(), lat.field(), lat.field(), lat.field()
    for call in (lambda: lat.Qtm_pm_ndpsi(a, b, c, d), lambda: lat.cg_her_nd(a, b, c, d, 10, 1e-20, 1, lat.Vh),
                 lambda: lat.cg_mms_tm_nd(c, d, [0.1, 0.2], 10, 1e-20, 0, P=[(a, b), (lat.field(), lat.field())])):
        with pytest.raises(TmHipError):
            call()
    lat.close()


@pytest.mark.parametrize("mode", ["coherent", "lazy", "resident"])
def test_dropin_symbols_in_every_residency_mode(mode):
    errs = run_child("nd_dropin_child.py", mode)
    for k, v in errs.items():
        if k.endswith("_iters"):
            assert v <= 1, (k, v)
        elif k.startswith("cg_"):
            assert v < 1e-9, (k, v)
        else:
            assert v < TOL, (k, v)
