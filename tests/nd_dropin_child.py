"""Child process of tests/test_gpu_nd.py::test_dropin_symbols_in_every_residency_mode.

A host program in miniature (tests/hostprog.py): the stub globals of tests/host_stub/globals.c plus the doublet's globals (g_mubar,
g_epsbar, phmc_invmaxev) are loaded first, then libtmlqcd_dropin.so, so that its weak references bind to them -- which needs a
fresh process.  Calls the reference-named doublet symbols with host arrays in the residency mode given on the command
line and prints the relative errors against tests/golden/ref_nd_4x4.npz as one JSON line.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import VP, SolverParams, rel_l2 as rel  # noqa: E402


def main(mode):
    stub, ndg, d = hostprog.load(extra_c=hostprog.ND_GLOBALS)
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_nd_4x4.npz"))
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_nd_scalars_4x4.json")))
    T = L = 4
    V = T * L ** 3
    N = V // 2
    hostprog.init_lattice(stub, T, L, L, L, f["gauge"], s["kappa"])
    ndg.nd_set(s["mubar"], s["epsbar"], s["invmaxev"])
    errs = {}
    with hostprog.HostFields(stub, d, mode) as hf:
        arr, host = (lambda init=None: hf.arr(N, init)), hf.copy
        ks, kc = arr(f["k_s"]), arr(f["k_c"])
        ls, lc = arr(), arr()
        for name in ("Qtm_ndpsi", "Qtm_dagger_ndpsi", "Qtm_pm_ndpsi"):
            getattr(d, name)(ls[1], lc[1], ks[1], kc[1])
            errs[name] = max(rel(host(ls), f[name + "_s"]), rel(host(lc), f[name + "_c"]))
        # l == k (Qtm_pm_ndpsi.c allows it)
        a_s, a_c = arr(f["k_s"]), arr(f["k_c"])
        d.Qtm_pm_ndpsi(a_s[1], a_c[1], a_s[1], a_c[1])
        errs["Qtm_pm_ndpsi_aliased"] = max(rel(host(a_s), f["Qtm_pm_ndpsi_s"]), rel(host(a_c), f["Qtm_pm_ndpsi_c"]))
        d.M_ee_inv_ndpsi(ls[1], lc[1], ks[1], kc[1], s["mubar"], s["epsbar"])
        errs["M_ee_inv_ndpsi"] = max(rel(host(ls), f["M_ee_inv_ndpsi_s"]), rel(host(lc), f["M_ee_inv_ndpsi_c"]))
        for ieo in (0, 1):
            d.H_eo_tm_ndpsi(ls[1], lc[1], ks[1], kc[1], ieo)
            errs["H_eo_tm_ndpsi_%d" % ieo] = max(rel(host(ls), f["H_eo_tm_ndpsi_%d_s" % ieo]), rel(host(lc), f["H_eo_tm_ndpsi_%d_c" % ieo]))
        d.mul_one_pm_itau2(ls[1], lc[1], ks[1], kc[1], 1.0, N)
        errs["mul_one_pm_itau2"] = max(rel(host(ls), (f["k_s"] + f["k_c"]) / np.sqrt(2.)), rel(host(lc), (f["k_c"] - f["k_s"]) / np.sqrt(2.)))
        # cg_her_nd from a zero start
        cs = s["cg_her_nd"]
        pu, pd = arr(), arr()
        it = d.cg_her_nd(pu[1], pd[1], ks[1], kc[1], cs["max_iter"], cs["eps_sq"], cs["rel_prec"], N, C.cast(d.Qtm_pm_ndpsi, VP))
        errs["cg_her_nd"] = max(rel(host(pu), f["cg_her_nd_up"]), rel(host(pd), f["cg_her_nd_dn"]))
        errs["cg_her_nd_iters"] = abs(it - cs["iters"])
        # cg_mms_tm_nd
        ms = s["cg_mms_tm_nd"]
        n = len(ms["shifts"])
        P = [(arr(), arr()) for _ in range(n)]
        up = (VP * n)(*[p[0][1] for p in P])
        dn = (VP * n)(*[p[1][1] for p in P])
        sh = (C.c_double * n)(*ms["shifts"])
        sp = SolverParams()
        sp.max_iter, sp.rel_prec, sp.no_shifts, sp.sdim = ms["max_iter"], ms["rel_prec"], n, N
        sp.squared_solver_prec = ms["eps_sq"]
        sp.M_ndpsi = C.cast(d.Qtm_pm_ndpsi, VP)
        sp.shifts = sh
        it = d.cg_mms_tm_nd(up, dn, ks[1], kc[1], C.byref(sp))
        errs["cg_mms_tm_nd"] = max(max(rel(host(P[k][0]), f["cg_mms_up_%d" % k]), rel(host(P[k][1]), f["cg_mms_dn_%d" % k])) for k in range(n))
        errs["cg_mms_tm_nd_iters"] = abs(it - ms["iters"])
    hostprog.emit(errs)


if __name__ == "__main__":
    main(sys.argv[1])
