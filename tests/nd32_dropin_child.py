"""Child process of tests/test_gpu_nd32.py::test_dropin_symbols_equal_the_core_calls.

A host program in miniature (tests/hostprog.py) with the doublet's globals (g_mubar, g_epsbar, phmc_invmaxev): calls the
reference-named Qtm_pm_ndpsi_32, M_ee_inv_ndpsi_32, M_oo_sub_g5_ndpsi_32 on host spinor32 arrays and rg_mixed_cg_her_nd -- with
`solver_params_t` by value -- on host spinor arrays, in the residency mode given on the command line, and the same calls of the core
library on a context of its own; prints whether the results are the same bits as one JSON line.  The prototypes of the four symbols
are the table ND32 below, in the form of hostprog.PROTOTYPES.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import D, I, VP, SolverParams  # noqa: E402

F = C.c_float
ND32 = {"Qtm_pm_ndpsi_32": (None, [VP] * 4), "M_ee_inv_ndpsi_32": (None, [VP] * 4 + [F, F]), "M_oo_sub_g5_ndpsi_32": (None, [VP] * 6 + [F, F]),
        "rg_mixed_cg_her_nd": (I, [VP] * 4 + [SolverParams, I, D, I, I, VP, VP])}
DELTA = 1e-3


def main(mode):
    stub, ndg, d = hostprog.load(extra_c=hostprog.ND_GLOBALS, core_first=True)
    hostprog.set_prototypes(d, ND32)
    from tmlqcd_amd import Lattice
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_nd32_4x4.npz"))
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_nd32_scalars_4x4.json")))
    gauge = np.load(os.path.join(ROOT, "tests", "golden", "ref_nd_4x4.npz"))["gauge"]
    T = L = 4
    N = T * L ** 3 // 2
    mu, eps = s["mubar"], s["epsbar"]
    # the core calls, on a context of their own
    lat = Lattice(T, L, L, L, kappa=s["kappa"], mu=0.0)
    lat.set_gauge(np.ascontiguousarray(gauge))
    lat.set_nd(mu, eps, s["invmaxev"])
    ks, kc = lat.field32(np.ascontiguousarray(f["q32_up"])), lat.field32(np.ascontiguousarray(f["q32_dn"]))
    ls, lc, es, ec = lat.field32(), lat.field32(), lat.field32(), lat.field32()
    core = {}
    lat.Qtm_pm_ndpsi_32(ls, lc, ks, kc)
    core["Qtm_pm_ndpsi_32"] = (ls.download(), lc.download())
    lat.M_ee_inv_ndpsi_32(es, ec, ks, kc, mu, eps)
    core["M_ee_inv_ndpsi_32"] = (es.download(), ec.download())
    lat.M_oo_sub_g5_ndpsi_32(es, ec, ks, kc, ls, lc, mu, eps)
    core["M_oo_sub_g5_ndpsi_32"] = (es.download(), ec.download())
    qu, qd, pu, pd = lat.field(np.ascontiguousarray(f["q_up"])), lat.field(np.ascontiguousarray(f["q_dn"])), lat.field(), lat.field()
    it_core, _ = lat.rg_mixed_cg_her_nd(pu, pd, qu, qd, s["max_iter"], s["eps_sq"], s["rel_prec"], N, delta=DELTA)
    core["rg"] = (pu.download(), pd.download())
    lat.close()
    # the host program
    hostprog.init_lattice(stub, T, L, L, L, gauge, s["kappa"])
    ndg.nd_set(mu, eps, s["invmaxev"])
    out = {"rg_iters_core": it_core}
    same = lambda got, want: bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
    with hostprog.HostFields(stub, d, mode) as hf:
        a32 = lambda init=None: hf.arr(N, init, dtype=np.float32)
        hk_s, hk_c, hl_s, hl_c, he_s, he_c = a32(f["q32_up"]), a32(f["q32_dn"]), a32(), a32(), a32(), a32()
        d.Qtm_pm_ndpsi_32(hl_s[1], hl_c[1], hk_s[1], hk_c[1])             # spinor32 arrays are copied in and out on every call
        out["Qtm_pm_ndpsi_32_bit_equal"] = same((hl_s[0], hl_c[0]), core["Qtm_pm_ndpsi_32"])
        d.M_ee_inv_ndpsi_32(he_s[1], he_c[1], hk_s[1], hk_c[1], mu, eps)
        out["M_ee_inv_ndpsi_32_bit_equal"] = same((he_s[0], he_c[0]), core["M_ee_inv_ndpsi_32"])
        d.M_oo_sub_g5_ndpsi_32(he_s[1], he_c[1], hk_s[1], hk_c[1], hl_s[1], hl_c[1], mu, eps)
        out["M_oo_sub_g5_ndpsi_32_bit_equal"] = same((he_s[0], he_c[0]), core["M_oo_sub_g5_ndpsi_32"])
        d.Qtm_pm_ndpsi_32(hk_s[1], hk_c[1], hk_s[1], hk_c[1])             # l == k
        out["Qtm_pm_ndpsi_32_aliased_bit_equal"] = same((hk_s[0], hk_c[0]), core["Qtm_pm_ndpsi_32"])
        # rg_mixed_cg_her_nd(P_up, P_dn, Q_up, Q_dn, solver_params BY VALUE, max_iter, eps_sq, rel_prec, N, f, f32)
        hq_u, hq_d = hf.arr(N, f["q_up"]), hf.arr(N, f["q_dn"])
        hp_u, hp_d = hf.arr(N, np.full((N, 4, 3, 2), 3.0)), hf.arr(N)   # zero start: whatever P holds is overwritten
        sp = SolverParams()
        sp.mcg_delta = DELTA
        it = d.rg_mixed_cg_her_nd(hp_u[1], hp_d[1], hq_u[1], hq_d[1], sp, s["max_iter"], s["eps_sq"], s["rel_prec"], N,
                                  C.cast(d.Qtm_pm_ndpsi, VP), C.cast(d.Qtm_pm_ndpsi_32, VP))
        out["rg_iters"] = it
        out["rg_solution_bit_equal"] = same((hf.copy(hp_u), hf.copy(hp_d)), core["rg"])
    hostprog.emit(out)


if __name__ == "__main__":
    main(sys.argv[1])
