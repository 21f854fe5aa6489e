"""Child process of tests/test_gpu_ndcloverrat.py::test_dropin_symbols.

A host program in miniature (tests/hostprog.py): the stub globals of tests/host_stub/globals.c (with its sw / sw_inv arrays)
plus the doublet's globals are loaded first, then libtmlqcd_dropin.so.  Calls tmlqcd_hip_sw_term, sw_invert_nd, Qsw_pm_ndpsi,
cg_mms_tm_nd with M_ndpsi = &Qsw_pm_ndpsi and tmlqcd_hip_ndcloverrat_derivative with host arrays in the residency mode given on the
command line, and prints the errors against tests/golden/ref_ndsw_4x4.npz / ref_ndsw_scalars_4x4.json (and, for the monomial, against
the core library's result on the same inputs) as one JSON line.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import HF, SolverParams, rel_l2 as rel, rel_max  # noqa: E402

VP, dbl = C.c_void_p, C.c_double
SITES = slice(0, None, 2)
MU3, RMU3 = [0.21, 0.6, 1.7], [0.05, 0.4, 1.3]
SOLVE = (2000, 1e-24, 1)


def main(mode):
    stub, ndg, d = hostprog.load(extra_c=hostprog.ND_GLOBALS)
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_ndsw_4x4.npz"))
    base = np.load(os.path.join(ROOT, "tests", "golden", "ref_nd_4x4.npz"))
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_ndsw_scalars_4x4.json")))
    T = L = 4
    V = T * L ** 3
    N = V // 2
    gauge = np.ascontiguousarray(base["gauge"])
    hostprog.init_lattice(stub, T, L, L, L, gauge, s["kappa"])
    ndg.nd_set(s["mubar"], s["epsbar"], s["invmaxev"])
    swi = stub.stub_init_clover(1)                                      # the host program's sw / sw_inv (init_sw_fields)
    errs = {}
    with hostprog.HostFields(stub, d, mode, modes=("coherent", "resident")) as hf:
        arr, host = (lambda init=None: hf.arr(N, init)), hf.copy
        d.tmlqcd_hip_sw_term(s["kappa"], s["c_sw"])
        d.sw_invert_nd(s["mshift"])
        errs["sw_invert_nd_failures"] = float(d.tmlqcd_hip_sw_invert_failures())
        inv_host = np.frombuffer((dbl * (V * 8 * 18)).from_address(swi), dtype=np.float64).reshape(V, 4, 2, 3, 3, 2)
        errs["sw_invert_nd_host_copy"] = rel_max(inv_host[:N][SITES], f["sw_inv_nd"])
        ks, kc = arr(base["k_s"]), arr(base["k_c"])
        ls, lc = arr(), arr()
        d.Qsw_pm_ndpsi(ls[1], lc[1], ks[1], kc[1])
        errs["Qsw_pm_ndpsi"] = max(rel(host(ls)[SITES], f["Qsw_pm_ndpsi_s"]), rel(host(lc)[SITES], f["Qsw_pm_ndpsi_c"]))
        a_s, a_c = arr(base["k_s"]), arr(base["k_c"])
        d.Qsw_pm_ndpsi(a_s[1], a_c[1], a_s[1], a_c[1])
        errs["Qsw_pm_ndpsi_aliased"] = max(rel(host(a_s)[SITES], f["Qsw_pm_ndpsi_s"]), rel(host(a_c)[SITES], f["Qsw_pm_ndpsi_c"]))
        # cg_mms_tm_nd with M_ndpsi = &Qsw_pm_ndpsi
        ms = s["cg_mms_tm_nd"]
        n = len(ms["shifts"])
        P = [(arr(), arr()) for _ in range(n)]
        up = (VP * n)(*[p[0][1] for p in P])
        dn = (VP * n)(*[p[1][1] for p in P])
        sh = (dbl * n)(*ms["shifts"])
        sp = SolverParams()
        sp.max_iter, sp.rel_prec, sp.no_shifts, sp.sdim = ms["max_iter"], ms["rel_prec"], n, N
        sp.squared_solver_prec = ms["eps_sq"]
        sp.M_ndpsi = C.cast(d.Qsw_pm_ndpsi, VP)
        sp.shifts = sh
        it = d.cg_mms_tm_nd(up, dn, ks[1], kc[1], C.byref(sp))
        errs["cg_mms_tm_nd_iters"] = abs(it - ms["iters"])
        norms = [float((host(P[k][0]) ** 2).sum() + (host(P[k][1]) ** 2).sum()) for k in range(n)]
        errs["cg_mms_tm_nd"] = max(abs(a - b) / b for a, b in zip(norms, ms["sol_norms"]))
        # the monomial body against the core library on the same inputs
        from tmlqcd_amd import Lattice
        lat = Lattice(T, L, L, L, kappa=s["kappa"], mu=0.0)
        lat.set_gauge(gauge)
        lat.set_nd(s["mubar"], s["epsbar"], s["invmaxev"])
        lat.sw_term(gauge, s["kappa"], s["c_sw"])
        lat.sw_invert_nd(s["mshift"])
        errs["core_sw_invert_nd_failures"] = float(lat.sw_invert_failures())
        lat.derivative_zero()
        it0 = lat.ndcloverrat_derivative(lat.field(ks[0].copy()), lat.field(kc[0].copy()), MU3, RMU3, s["invmaxev"], s["kappa"], s["c_sw"], 1, *SOLVE)
        ref = lat.derivative()
        lat.close()
        df_host = np.random.default_rng(96).standard_normal((V, 4, 8))
        start = df_host.copy()
        rows = (VP * V)(*[df_host.ctypes.data + 4 * 8 * 8 * i for i in range(V)])      # su3adj **derivative
        hfield = HF(None, None, C.cast(rows, VP), 0, 0)
        mu, rmu = (dbl * 3)(*MU3), (dbl * 3)(*RMU3)
        it = d.tmlqcd_hip_ndcloverrat_derivative(C.byref(hfield), ks[1], kc[1], mu, rmu, 3, s["invmaxev"], s["kappa"], s["c_sw"], 1, *SOLVE)
        errs["ndcloverrat_derivative_iters"] = abs(it - it0)
        if mode == "resident":
            errs["ndcloverrat_derivative_held_back"] = float(np.abs(df_host - start).max())
            d.tmlqcd_hip_flush_derivative(C.byref(hfield))
        errs["ndcloverrat_derivative"] = rel_max(df_host, start + ref)
    hostprog.emit(errs)


if __name__ == "__main__":
    main(sys.argv[1])
