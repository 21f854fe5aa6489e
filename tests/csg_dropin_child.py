"""Child process of tests/test_gpu_csg.py::test_dropin_symbols and ::test_dropin_refuses_a_list_of_21.

A host program in miniature (tests/hostprog.py): the stub globals of tests/host_stub/globals.c are loaded first, then
libtmlqcd_dropin.so.  In the residency mode given on the command line it calls, by name and with host arrays,
  - scalar_prod / assign_diff_mul / mul on VOLUME/2, VOLUME, 37 and 0 sites,
  - chrono_add_solution seven times into a list of three (the index sequence of the fixture),
  - chrono_guess with f = &Qtm_pm_psi on the n = 5 inputs of tests/golden/ref_csg_4x4.npz, and with an empty list and a list of length 0,
  - chrono_guess; cg_her; chrono_add_solution three times running with f = &Qsw_pm_psi (the statements of cloverdetratio_derivative),
    against the same sequence through the core library,
  - chrono_guess with a foreign f (a callback: the drop-in's Qtm_pm_psi plus 0.1 times the input) against tests/csg_restate.py,
and prints the results as one JSON line.  Mode "too_long" calls chrono_guess with a list of 21 and must not return."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.nd_restate import cplx, real  # noqa: E402
from tests import csg_restate  # noqa: E402
from tests import hostprog  # noqa: E402
from tests.util import TOL, random_spinor, rel_err  # noqa: E402

VP, dbl, INT = C.c_void_p, C.c_double, C.c_int
GOLD = os.path.join(ROOT, "tests", "golden")
C_SW = 1.2
SOLVE = (2000, 1e-14, 1)


def main(mode):
    f = np.load(os.path.join(GOLD, "ref_csg_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_csg_scalars_4x4.json")))
    gauge = np.ascontiguousarray(np.load(os.path.join(GOLD, s["gauge_from"]))["gauge"])
    stub, _, d = hostprog.load()
    shape = (s["T"], s["L"], s["L"], s["L"])
    V = int(np.prod(shape))
    N = V // 2
    kappa, mu = s["kappa"], s["mu"]
    hostprog.init_lattice(stub, *shape, gauge, kappa)
    stub.stub_set_mu(mu)
    stub.stub_init_clover(1)
    # "too_long" runs in coherent mode
    with hostprog.HostFields(stub, d, "coherent" if mode == "too_long" else mode, modes=("coherent", "resident")) as hf:
        def arr(init=None, sites=N):
            a, p = hf.arr(V)
            if init is not None:
                a[:sites] = init
            return a, p

        def host_copy(a, sites=N):
            return hf.copy(a)[:sites]

        def ptrs(fields):
            return (VP * max(len(fields), 1))(*[x[1] for x in fields])

        if mode == "too_long":
            vs = [arr(random_spinor(k, N)) for k in range(2)]
            idx = (INT * 21)(*range(21))
            d.chrono_guess(vs[0][1], vs[1][1], ptrs([vs[0]] * 21), idx, 21, 2, N, C.cast(d.Qtm_pm_psi, VP))
            print("chrono_guess returned from a list of 21")
            return

        errs = {}
        # ---- the complex linalg by name
        for sites in (N, V, 37):
            S, R = random_spinor(1, sites), random_spinor(2, sites)
            a, b = arr(S, sites), arr(R, sites)
            zs, zr = cplx(S), cplx(R)
            z = d.scalar_prod(a[1], b[1], sites, 1)
            errs["linalg_scalar_prod_%d" % sites] = abs(complex(z.re, z.im) - np.vdot(zs, zr)) / np.sum(np.abs(zs) * np.abs(zr))
            c = 0.4 - 0.9j
            d.assign_diff_mul(a[1], b[1], c.real, c.imag, sites)
            errs["linalg_assign_diff_mul_%d" % sites] = rel_err(host_copy(a, sites), real(zs - c * zr))
            d.mul(a[1], c.real, c.imag, b[1], sites)
            errs["linalg_mul_%d" % sites] = rel_err(host_copy(a, sites), real(c * zr))
            d.mul(b[1], c.real, c.imag, b[1], sites)                   # in place
            errs["linalg_mul_in_place_%d" % sites] = rel_err(host_copy(b, sites), real(c * zr))
        keep = host_copy(a, 37)
        d.mul(a[1], 3.0, 0.0, b[1], 0)
        d.assign_diff_mul(a[1], b[1], 3.0, 0.0, 0)
        z = d.scalar_prod(a[1], b[1], 0, 1)
        errs["linalg_N0"] = float(np.abs(host_copy(a, 37) - keep).max() + abs(z.re) + abs(z.im))

        # ---- the rotation of the list
        v3 = [arr() for _ in range(3)]
        idx3, n3 = (INT * 3)(-1, -1, -1), INT(0)
        seq_ok, norm_err = True, 0.0
        for k, want in enumerate(s["add_sequence_N3"]):
            x = arr(random_spinor(40 + k, N))
            d.chrono_add_solution(x[1], ptrs(v3), idx3, 3, C.byref(n3), N)
            seq_ok = seq_ok and [idx3[j] for j in range(3)] == want["index_array"] and n3.value == want["n"]
            stored = host_copy(v3[idx3[n3.value - 1]])
            norm_err = max(norm_err, abs(np.sum(stored ** 2) - 1.0), rel_err(stored, x[0][:N] / np.sqrt(np.sum(x[0][:N] ** 2))))
        n0 = INT(0)
        d.chrono_add_solution(x[1], ptrs(v3), idx3, 0, C.byref(n0), N)   # a list of length 0: nothing happens
        seq_ok = seq_ok and n0.value == 0
        errs["linalg_add_solution_norm"] = norm_err

        # ---- chrono_guess on the reference's inputs, f known to the library
        case = s["cases"]["5"]
        bound = case["cond"] * TOL
        vs = [arr(v) for v in f["n5_before"]]
        order = [3, 4, 0, 1, 2]                                         # the list as a rotated one: v[index_array[i]] is the i-th oldest
        slots = [None] * 5
        for i, sl in enumerate(order):
            slots[sl] = vs[i]
        idx = (INT * 5)(*order)
        phi, trial = arr(f["n5_phi"]), arr(random_spinor(9, N))
        fq = C.cast(d.Qtm_pm_psi, VP)
        d.chrono_guess(trial[1], phi[1], ptrs(slots), idx, 5, 5, N, fq)
        errs["guess_trial"] = rel_err(host_copy(trial), f["n5_trial"])
        errs["guess_history"] = max(rel_err(host_copy(vs[i]), f["n5_after"][i]) for i in range(5))
        zero_ok = True
        for (NN, nn, sites) in ((5, 0, N), (0, 0, N), (-1, 3, N)):
            trial[0][:] = 1.0
            d.tmlqcd_hip_host_modified(trial[1])
            d.chrono_guess(trial[1], phi[1], ptrs(slots), idx, NN, nn, sites, fq)
            zero_ok = zero_ok and not host_copy(trial).any()

        # ---- chrono_guess; cg_her; chrono_add_solution with f = &Qsw_pm_psi three times running, and the same through the core library
        d.tmlqcd_hip_sw_term(kappa, C_SW)
        d.tmlqcd_hip_sw_invert(0, mu)
        b = csg_restate.rhs_fields(N)
        fsw = C.cast(d.Qsw_pm_psi, VP)
        lst = [arr() for _ in range(2)]
        idx2, n2 = (INT * 2)(-1, -1), INT(0)
        x = arr()
        iters, sols = [], []
        for k in range(3):
            rhs = arr(b[k])
            d.chrono_guess(x[1], rhs[1], ptrs(lst), idx2, 2, n2.value, N, fsw)
            iters.append(d.cg_her(x[1], rhs[1], *SOLVE, N, fsw))
            d.chrono_add_solution(x[1], ptrs(lst), idx2, 2, C.byref(n2), N)
            sols.append(host_copy(x))
        from tmlqcd_amd import Lattice
        lat = Lattice(*shape, kappa=kappa, mu=mu)
        lat.set_gauge(gauge)
        lat.sw_term(gauge, kappa, C_SW)
        lat.sw_invert(0, mu)
        cl = [lat.field(b[0]) for _ in range(2)]
        cidx, cn = [-1, -1], 0
        cx = lat.field(b[0])
        iters_core = []
        for k in range(3):
            rhs = lat.field(b[k])
            lat.chrono_guess(cx, rhs, [cl[j] for j in cidx[:cn]], "Qsw_pm_psi")
            iters_core.append(lat.cg_her(cx, rhs, *SOLVE, N, "Qsw_pm_psi")[0])
            slot, cn = csg_restate.add_solution(cidx, cn, 2)
            lat.chrono_add_solution(cl[slot], cx)
            errs["linalg_clover_solution_%d" % k] = rel_err(sols[k], cx.download())
        lat.close()

        # ---- a foreign f: runs on host arrays, the plain path in coherent mode
        def shifted(l, k):
            d.Qtm_pm_psi(l, k)
            out = np.frombuffer((dbl * (N * 24)).from_address(l), dtype=np.float64)
            out += 0.1 * np.frombuffer((dbl * (N * 24)).from_address(k), dtype=np.float64)
        cb = C.CFUNCTYPE(None, VP, VP)(shifted)
        from oracle.oraclebind import Oracle
        orc = Oracle(*shape, kappa=kappa, mu=mu)
        orc.set_gauge(gauge)

        def A(z):
            l = np.zeros((N, 4, 3, 2))
            orc.op("Qtm_pm_psi", l, real(z))
            return cplx(l) + 0.1 * z
        want_vs = [cplx(v) for v in f["n5_before"]]
        want_trial, Gr, _, _ = csg_restate.chrono_guess(A, want_vs, cplx(f["n5_phi"]))
        fbound = float(np.linalg.cond(Gr)) * TOL
        vs = [arr(v) for v in f["n5_before"]]
        for i, sl in enumerate(order):
            slots[sl] = vs[i]
        trial = arr()
        d.chrono_guess(trial[1], phi[1], ptrs(slots), idx, 5, 5, N, C.cast(cb, VP))
        errs["foreign_trial"] = rel_err(host_copy(trial), real(want_trial))
        errs["foreign_history"] = max(rel_err(host_copy(vs[i]), real(want_vs[i])) for i in range(5))
    hostprog.emit({"errs": errs, "bounds": {"linalg": TOL, "guess": bound, "foreign": fbound}, "index_sequence_ok": bool(seq_ok), "zero_trials_ok": bool(zero_ok),
                   "clover_iters": iters, "clover_iters_core": iters_core})


if __name__ == "__main__":
    main(sys.argv[1])
