"""Child process of tests/test_gpu_nd.py::test_dropin_symbols_in_every_residency_mode.

A host program in miniature: the stub globals of tests/host_stub/globals.c plus the doublet's globals (g_mubar, g_epsbar,
phmc_invmaxev) are loaded first, then libtmlqcd_dropin.so, so that its weak references bind to them -- which needs a
fresh process.  Calls the reference-named doublet symbols with host arrays in the residency mode given on the command
line and prints the relative errors against tests/golden/ref_nd_4x4.npz as one JSON line.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = C.c_void_p
ND_GLOBALS = """
double g_mubar = 0.0, g_epsbar = 0.0, phmc_invmaxev = 1.0;
void nd_set(double a, double b, double c) { g_mubar = a; g_epsbar = b; phmc_invmaxev = c; }
"""


class SolverParams(C.Structure):   # include/tmlqcd_dropin.h: tmlqcd_solver_params (solver/solver_params.h:46-109)
    _fields_ = [("eigcg_i", C.c_int * 5), ("eigcg_d", C.c_double * 3), ("eigcg_rand_guess_opt", C.c_int), ("mcg_delta", C.c_float),
                ("type", C.c_int), ("max_iter", C.c_int), ("rel_prec", C.c_int), ("no_shifts", C.c_int), ("sdim", C.c_int),
                ("squared_solver_prec", C.c_double), ("M_psi", VP), ("M_psi32", VP), ("M_ndpsi", VP), ("M_ndpsi32", VP),
                ("shifts", C.POINTER(C.c_double)), ("solution_type", C.c_int), ("compression_type", C.c_int),
                ("sloppy_precision", C.c_int), ("external_inverter", C.c_int)]


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


def main(mode):
    tmp = tempfile.mkdtemp()
    host = os.path.join(tmp, "libhost.so")
    nd = os.path.join(tmp, "libndglobals.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-o", host, os.path.join(ROOT, "tests", "host_stub", "globals.c"), "-lm"])
    src = os.path.join(tmp, "nd.c")
    open(src, "w").write(ND_GLOBALS)
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-o", nd, src])
    stub = C.CDLL(host, mode=C.RTLD_GLOBAL)
    ndg = C.CDLL(nd, mode=C.RTLD_GLOBAL)
    d = C.CDLL(os.path.join(ROOT, "tmlqcd_amd", "lib", "libtmlqcd_dropin.so"), mode=C.RTLD_GLOBAL)
    stub.stub_init.restype = VP
    stub.stub_init.argtypes = [C.c_int] * 4
    stub.stub_boundary.argtypes = [C.c_double] * 5
    stub.stub_calloc.restype = VP
    stub.stub_calloc.argtypes = [C.c_size_t]
    ndg.nd_set.argtypes = [C.c_double] * 3
    for n in ("Qtm_ndpsi", "Qtm_dagger_ndpsi", "Qtm_pm_ndpsi"):
        getattr(d, n).argtypes = [VP] * 4
    d.M_ee_inv_ndpsi.argtypes = [VP] * 4 + [C.c_double] * 2
    d.H_eo_tm_ndpsi.argtypes = [VP] * 4 + [C.c_int]
    d.mul_one_pm_itau2.argtypes = [VP] * 4 + [C.c_double, C.c_int]
    d.cg_her_nd.restype = C.c_int
    d.cg_her_nd.argtypes = [VP] * 4 + [C.c_int, C.c_double, C.c_int, C.c_int, VP]
    d.cg_mms_tm_nd.restype = C.c_int
    d.cg_mms_tm_nd.argtypes = [C.POINTER(VP), C.POINTER(VP), VP, VP, C.POINTER(SolverParams)]
    d.tmlqcd_hip_set_residency.argtypes = [C.c_int]
    d.tmlqcd_hip_sync_to_host.argtypes = [VP]

    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_nd_4x4.npz"))
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_nd_scalars_4x4.json")))
    T = L = 4
    V = T * L ** 3
    N = V // 2
    g = stub.stub_init(T, L, L, L)
    gauge = np.ascontiguousarray(f["gauge"])
    C.memmove(g, gauge.ctypes.data, gauge.nbytes)
    stub.stub_boundary(s["kappa"], 0.0, 0.0, 0.0, 0.0)
    ndg.nd_set(s["mubar"], s["epsbar"], s["invmaxev"])
    d.tmlqcd_hip_set_residency({"coherent": 0, "resident": 1, "lazy": 2}[mode])

    def arr(init=None):   # page-aligned host arrays (watchable in lazy mode), as a host program's own fields
        p = stub.stub_calloc(N * 24 * 8)
        a = np.frombuffer((C.c_double * (N * 24)).from_address(p), dtype=np.float64).reshape(N, 4, 3, 2)
        if init is not None:
            a[:] = init
        return a, p

    def host(a):
        if mode == "resident":
            d.tmlqcd_hip_sync_to_host(a[1])
        return a[0].copy()

    errs = {}
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
    d.tmlqcd_hip_set_residency(0)
    print(json.dumps(errs))
    sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1])
