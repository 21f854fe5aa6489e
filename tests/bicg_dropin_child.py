"""Child process of tests/test_gpu_bicg_dropin.py.

A host program in miniature (tests/hostprog.py): the stub globals of tests/host_stub/globals.c are loaded first, then
libtmlqcd_dropin.so.  In the residency mode given on the command line (coherent or lazy) it calls, by name and with host arrays,
  - assign_add_mul_add_mul / assign_mul_bra_add_mul_ket_add on VOLUME/2, VOLUME, 37 and 0 sites,
  - bicgstab_complex with f = &Mtm_plus_sym_psi on VOLUME/2 sites and f = &D_psi on VOLUME sites, on the inputs of the 4^4 fixture
    (tests/golden/ref_bicg_*), counting the entry-point calls the library served meanwhile (tmlqcd_hip_calls),
  - bicgstab_complex with a foreign f (a callback: the drop-in's Mtm_plus_sym_psi plus 0.1 times the input), which takes the host loop,
  - cg_her with f = &Mtm_plus_sym_psi and bicgstab_complex with f = &Qtm_pm_psi on VOLUME/2 sites, three iterations each: operators of
    the library, but outside the respective solver's set, so both take the host loop too (only tmlqcd_hip_calls is counted),
and prints the results as one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.nd_restate import cplx  # noqa: E402
from tests import bicg_restate as br  # noqa: E402
from tests import hostprog  # noqa: E402
from tests.util import random_spinor  # noqa: E402

VP, dbl = C.c_void_p, C.c_double
GOLD = os.path.join(ROOT, "tests", "golden")
EPS = float(np.finfo(np.float64).eps)


def main(mode):
    s = json.load(open(os.path.join(GOLD, "ref_bicg_scalars_4x4.json")))
    f = np.load(os.path.join(GOLD, "ref_bicg_4x4.npz"))
    gauge = np.ascontiguousarray(np.load(os.path.join(GOLD, s["gauge_from"]))["gauge"])
    stub, _, d = hostprog.load()
    shape = tuple(s["dims"])
    V = int(np.prod(shape))
    N = V // 2
    hostprog.init_lattice(stub, *shape, gauge, s["kappa"])
    out = {"linalg": {}, "solves": {}}
    with hostprog.HostFields(stub, d, mode, modes=("coherent", "lazy")) as hf:
        def arr(init=None, sites=N):
            a, p = hf.arr(V)
            if init is not None:
                a[:sites] = init
            return a, p

        # ---- the two singles by name: the worst element error in units of eps times the sum of the magnitudes of its terms
        c1, c2 = 0.7 - 0.3j, -0.45 + 1.1j
        stub.stub_set_mu(0.02)
        for sites in (N, V, 37):
            R, S, U = random_spinor(1, sites), random_spinor(2, sites), random_spinor(3, sites)
            zr, zs, zu = cplx(R), cplx(S), cplx(U)
            a, b, c = arr(R, sites), arr(S, sites), arr(U, sites)
            d.assign_add_mul_add_mul(a[1], b[1], c[1], c1.real, c1.imag, c2.real, c2.imag, sites)
            scale = np.abs(zr) + abs(c1) * np.abs(zs) + abs(c2) * np.abs(zu)
            out["linalg"]["add_mul_add_mul_%d" % sites] = float(np.max(np.abs(cplx(a[0][:sites]) - (zr + (c1 * zs + c2 * zu))) / scale) / EPS)
            a2 = arr(R, sites)
            d.assign_mul_bra_add_mul_ket_add(a2[1], b[1], c[1], c1.real, c1.imag, c2.real, c2.imag, sites)
            scale = np.abs(zu) + abs(c2) * (np.abs(zr) + abs(c1) * np.abs(zs))
            out["linalg"]["mul_bra_add_mul_ket_add_%d" % sites] = float(np.max(np.abs(cplx(a2[0][:sites]) - (zu + c2 * (zr + c1 * zs))) / scale) / EPS)
            if sites == 37:
                keep = a[0][:37].copy()
                d.assign_add_mul_add_mul(a[1], b[1], c[1], 3.0, 0.0, 1.0, 0.0, 0)
                d.assign_mul_bra_add_mul_ket_add(a[1], b[1], c[1], 3.0, 0.0, 1.0, 0.0, 0)
                out["linalg"]["N0_unchanged"] = bool(np.array_equal(a[0][:37], keep))

        # ---- the solver with operators the library knows: one entry-point call served per solve
        def solve(name, fptr, shift=0.0):
            case = s["cases"][name]
            stub.stub_set_mu(case["g_mu"])
            Q, P0 = br.case_fields(case, V)
            sites = Q.shape[0]
            q, p = arr(Q, sites), arr(P0, sites)
            before = d.tmlqcd_hip_calls()
            it = d.bicgstab_complex(p[1], q[1], case["max_iter"], case["eps_sq"], case["rel_prec"], sites, fptr)
            calls = d.tmlqcd_hip_calls() - before
            sol = p[0][:sites].copy()
            orc = br.oracle_for(shape, gauge, s["kappa"], s["c_sw"], case)
            A0 = br.operator(orc, case["op"])
            A = (lambda z: A0(z) + shift * z)
            true = float(np.sum(np.abs(cplx(Q) - A(cplx(sol))) ** 2))
            res = {"iters": it, "calls": int(calls), "true": true, "bound": br.bound_of(case, Q), "q_unchanged": bool(np.array_equal(q[0][:sites], Q))}
            if shift == 0.0:
                res["dist"] = float(np.sqrt(np.sum((sol - f[name + "_P"]) ** 2)))
                res["ref_iters"], res["sigma_min"] = case["iters"], case["sigma_min"]
            else:
                it_np, P_np, _ = br.bicgstab_complex(A, cplx(P0), cplx(Q), case["max_iter"], case["eps_sq"], case["rel_prec"])
                res["restated_iters"] = it_np
            return res

        out["solves"]["mtm_plus_sym"] = solve("mtm_plus_sym", C.cast(d.Mtm_plus_sym_psi, VP))
        out["solves"]["mtm_plus_sym_guess"] = solve("mtm_plus_sym_guess", C.cast(d.Mtm_plus_sym_psi, VP))
        out["solves"]["d_psi"] = solve("d_psi", C.cast(d.D_psi, VP))

        # ---- a foreign f: runs on host arrays, the reference's loop over the drop-in linalg in coherent mode
        def shifted(l, k):
            d.Mtm_plus_sym_psi(l, k)
            o = np.frombuffer((dbl * (N * 24)).from_address(l), dtype=np.float64)
            o += 0.1 * np.frombuffer((dbl * (N * 24)).from_address(k), dtype=np.float64)
        cb = C.CFUNCTYPE(None, VP, VP)(shifted)
        out["solves"]["foreign"] = solve("mtm_plus_sym", C.cast(cb, VP), shift=0.1)

        # ---- operators the library knows, handed to a solver that does not take them: the host loop again, many entry-point calls
        def routed(solver, fptr):
            stub.stub_set_mu(0.02)
            q, p = arr(random_spinor(4, N)), arr()
            before = d.tmlqcd_hip_calls()
            solver(p[1], q[1], 3, 1.0e-30, 0, N, fptr)
            return int(d.tmlqcd_hip_calls() - before)
        out["routing"] = {"cg_her_mtm_plus_sym": routed(d.cg_her, C.cast(d.Mtm_plus_sym_psi, VP)),
                          "bicgstab_qtm_pm": routed(d.bicgstab_complex, C.cast(d.Qtm_pm_psi, VP))}
        out["margin"] = s["margin"]
    hostprog.emit(out)


if __name__ == "__main__":
    main(sys.argv[1])
