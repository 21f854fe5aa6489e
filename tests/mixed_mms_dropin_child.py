"""Child process of tests/test_gpu_mixed_mms_dropin.py.

A host program in miniature (tests/hostprog.py) with the doublet's globals (g_mubar, g_epsbar, phmc_invmaxev): calls the
reference-named mixed_cg_mms_tm_nd with a `solver_params_t` on host spinor arrays, in the residency mode given on the command line,
and tmhip_mixed_cg_mms_tm_nd of the core library on a context of its own; prints whether the results are the same bits as one JSON line.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import I, PSP, VP, SolverParams  # noqa: E402

PROTO = {"mixed_cg_mms_tm_nd": (I, [C.POINTER(VP), C.POINTER(VP), VP, VP, PSP])}


def main(mode):
    stub, ndg, d = hostprog.load(extra_c=hostprog.ND_GLOBALS, core_first=True)
    hostprog.set_prototypes(d, PROTO)
    from tmlqcd_amd import Lattice
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_nd32_4x4.npz"))
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_mixed_mms_scalars_4x4.json")))
    gauge = np.load(os.path.join(ROOT, "tests", "golden", "ref_nd_4x4.npz"))["gauge"]
    run = s["runs"][0]
    T = L = 4
    N = T * L ** 3 // 2
    n = run["nshifts"]
    # the core call, on a context of its own
    lat = Lattice(T, L, L, L, kappa=s["kappa"], mu=0.0)
    lat.set_gauge(np.ascontiguousarray(gauge))
    lat.set_nd(s["mubar"], s["epsbar"], s["invmaxev"])
    qu, qd = lat.field(np.ascontiguousarray(f["q_up"])), lat.field(np.ascontiguousarray(f["q_dn"]))
    it_core, counts, P = lat.mixed_cg_mms_tm_nd(qu, qd, s["shifts"], s["max_iter"], run["eps_sq"], run["rel_prec"])
    core = [(a.download(), b.download()) for a, b in P]
    lat.close()
    # the host program
    hostprog.init_lattice(stub, T, L, L, L, gauge, s["kappa"])
    ndg.nd_set(s["mubar"], s["epsbar"], s["invmaxev"])
    out = {"iters_core": it_core, "updates_core": counts[0], "removed_core": counts[1], "reference_iters": run["iters"]}
    with hostprog.HostFields(stub, d, mode) as hf:
        hq_u, hq_d = hf.arr(N, f["q_up"]), hf.arr(N, f["q_dn"])
        hp = [(hf.arr(N, np.full((N, 4, 3, 2), 3.0)), hf.arr(N)) for _ in range(n)]     # whatever P holds is overwritten
        up = (VP * n)(*[p[0][1] for p in hp])
        dn = (VP * n)(*[p[1][1] for p in hp])
        sh = (C.c_double * n)(*s["shifts"])
        sp = SolverParams()
        sp.max_iter, sp.rel_prec, sp.no_shifts, sp.sdim = s["max_iter"], run["rel_prec"], n, N
        sp.squared_solver_prec = run["eps_sq"]
        sp.M_ndpsi = C.cast(d.Qtm_pm_ndpsi, VP)
        sp.M_ndpsi32 = C.cast(d.Qtm_pm_ndpsi_32, VP)
        sp.shifts = sh
        out["iters"] = d.mixed_cg_mms_tm_nd(up, dn, hq_u[1], hq_d[1], C.byref(sp))
        out["solutions_bit_equal"] = all(bool(np.array_equal(hf.copy(hp[k][0]), core[k][0]) and np.array_equal(hf.copy(hp[k][1]), core[k][1]))
                                         for k in range(n))
        out["source_untouched"] = bool(np.array_equal(hf.copy(hq_u), f["q_up"]) and np.array_equal(hf.copy(hq_d), f["q_dn"]))
    hostprog.emit(out)


if __name__ == "__main__":
    main(sys.argv[1])
