"""Child process of tests/test_gpu_mms_dropin.py.

A host program in miniature (tests/hostprog.py): the stub globals of tests/host_stub/globals.c plus g_sloppy_precision are loaded first,
then libtmlqcd_dropin.so, so that its weak references bind to them -- which needs a fresh process.  Calls cg_mms_tm with a
tmlqcd_solver_params built as the rat monomial (M_psi = Qtm_pm_psi, sdim = VOLUME/2; solver/monomial_solve.c:176-215) and as
invert_eo.c:463-490 builds it (M_psi = Q_pm_psi, sdim = VOLUME, g_mu = 0), and once with an M_psi the library does not know (a C
function that calls Qtm_pm_psi: the generic path), in the residency mode given on the command line.  Then cg_her with that same
unknown f on the reference's 4^4 fixture (tests/golden/ref_fields_4x4.npz, made by oracle/make_golden.py:66-70): its generic path
runs in coherent mode and must hand the mode back as it found it.  Prints the relative errors against the golden files and the
other checks as one JSON line.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import VP, SolverParams, rel_l2 as rel, rel_max as max_rel  # noqa: E402


def main(mode):
    stub, ex, d = hostprog.load(extra_c=hostprog.SLOPPY_GLOBALS + hostprog.WRAPPED_QTM_PM_PSI)
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_mms_4x4.npz"))
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_mms_scalars_4x4.json")))
    T = L = 4
    V = T * L ** 3
    g = hostprog.init_lattice(stub, T, L, L, L, f["gauge"], s["kappa"])
    out = {}
    with hostprog.HostFields(stub, d, mode) as hf:
        arr, host = hf.arr, hf.copy
        for name, fn in (("qtm", d.Qtm_pm_psi), ("qpm_full", d.Q_pm_psi), ("qtm_generic", ex.wrapped_Qtm_pm_psi)):
            case = s["cases"]["qtm" if name == "qtm_generic" else name]
            n = V if name == "qpm_full" else V // 2
            stub.stub_set_mu(case["g_mu"])
            q = arr(n, f["q_full"] if name == "qpm_full" else f["q_eo"])
            k = len(case["shifts"])
            P = [arr(n, 7.0) for _ in range(k)]
            ptrs = (VP * k)(*[p[1] for p in P])
            sh = (C.c_double * k)(*case["shifts"])
            sp = SolverParams()
            sp.max_iter, sp.rel_prec, sp.no_shifts, sp.sdim = case["max_iter"], case["rel_prec"], k, n
            sp.squared_solver_prec = case["eps_sq"]
            sp.M_psi = C.cast(fn, VP)
            sp.shifts = sh
            reached = C.c_double(-1.0)
            ex.set_sloppy(1)
            it = d.cg_mms_tm(ptrs, q[1], C.byref(sp), C.byref(reached))
            key = "qtm" if name == "qtm_generic" else name
            out[name] = max(rel(host(P[j]), f["%s_P%d" % (key, j)]) for j in range(k))
            out[name + "_iters"] = abs(it - case["iters"])
            out[name + "_reached"] = reached.value / case["reached_prec"]
            out[name + "_sloppy"] = ex.get_sloppy()

        # cg_her, generic path, outside coherent mode: source = in, P = 0, the arguments the fixture was made with
        ff = np.load(os.path.join(ROOT, "tests", "golden", "ref_fields_4x4.npz"))
        ss = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_scalars_4x4.json")))
        gauge = np.ascontiguousarray(ff["gauge"])
        C.memmove(g, gauge.ctypes.data, gauge.nbytes)
        stub.stub_mark_gauge_dirty()
        stub.stub_boundary(ss["kappa"], 0.0, 0.0, 0.0, 0.0)
        stub.stub_set_mu(ss["mu"])
        q, p = arr(V // 2, ff["in"]), arr(V // 2, 0.0)
        it = d.cg_her(p[1], q[1], 1000, 1e-20, 1, V // 2, C.cast(ex.wrapped_Qtm_pm_psi, VP))
        out["cg_her_generic"] = max_rel(host(p), ff["cg_solution"])
        out["cg_her_generic_iters"] = abs(it - ss["cg_iters"])
        # the mode is still the one set above: the next operator's result is on the host at once (coherent), stays in HBM until asked
        # for (resident: the host array keeps its 7.0), or comes over through page faults as the host reads it (lazy)
        l = arr(V // 2, 7.0)
        st0, st1 = (C.c_ulong * 4)(), (C.c_ulong * 4)()
        d.Qtm_pm_psi(l[1], q[1])
        d.tmlqcd_hip_lazy_stats(st0)                # faults served before the host looks at the result ...
        untouched = bool(np.all(l[0] == 7.0))
        out["cg_her_generic_then_Qtm_pm_psi"] = max_rel(host(l), ff["Qtm_pm_psi"])
        d.tmlqcd_hip_lazy_stats(st1)                # ... and after
        out["cg_her_generic_mode_kept"] = {"coherent": not untouched and st1[0] == st0[0], "resident": untouched, "lazy": st1[0] > st0[0]}[mode]
    hostprog.emit(out)


if __name__ == "__main__":
    main(sys.argv[1])
