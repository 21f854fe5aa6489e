"""Child process of tests/test_gpu_mms_dropin.py.

A host program in miniature: the stub globals of tests/host_stub/globals.c plus g_sloppy_precision are loaded first, then
libtmlqcd_dropin.so, so that its weak references bind to them -- which needs a fresh process.  Calls cg_mms_tm with a
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
import subprocess
import sys
import tempfile

import numpy as np

from nd_dropin_child import SolverParams, VP, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = """
int g_sloppy_precision = 0;
void set_sloppy(int v) { g_sloppy_precision = v; }
int get_sloppy(void) { return g_sloppy_precision; }
extern void Qtm_pm_psi(void *, void *);
void wrapped_Qtm_pm_psi(void *l, void *k) { Qtm_pm_psi(l, k); }
"""


def main(mode):
    tmp = tempfile.mkdtemp()
    host = os.path.join(tmp, "libhost.so")
    extra = os.path.join(tmp, "libextra.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-o", host, os.path.join(ROOT, "tests", "host_stub", "globals.c"), "-lm"])
    src = os.path.join(tmp, "extra.c")
    open(src, "w").write(EXTRA)
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-o", extra, src])
    stub = C.CDLL(host, mode=C.RTLD_GLOBAL)
    ex = C.CDLL(extra, mode=C.RTLD_GLOBAL | getattr(os, "RTLD_LAZY", 1))
    d = C.CDLL(os.path.join(ROOT, "tmlqcd_amd", "lib", "libtmlqcd_dropin.so"), mode=C.RTLD_GLOBAL)
    stub.stub_init.restype = VP
    stub.stub_init.argtypes = [C.c_int] * 4
    stub.stub_boundary.argtypes = [C.c_double] * 5
    stub.stub_set_mu.argtypes = [C.c_double]
    stub.stub_calloc.restype = VP
    stub.stub_calloc.argtypes = [C.c_size_t]
    ex.set_sloppy.argtypes = [C.c_int]
    d.cg_mms_tm.restype = C.c_int
    d.cg_mms_tm.argtypes = [C.POINTER(VP), VP, C.POINTER(SolverParams), C.POINTER(C.c_double)]
    d.tmlqcd_hip_set_residency.argtypes = [C.c_int]
    d.tmlqcd_hip_sync_to_host.argtypes = [VP]

    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_mms_4x4.npz"))
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_mms_scalars_4x4.json")))
    T = L = 4
    V = T * L ** 3
    g = stub.stub_init(T, L, L, L)
    gauge = np.ascontiguousarray(f["gauge"])
    C.memmove(g, gauge.ctypes.data, gauge.nbytes)
    stub.stub_boundary(s["kappa"], 0.0, 0.0, 0.0, 0.0)
    d.tmlqcd_hip_set_residency({"coherent": 0, "resident": 1, "lazy": 2}[mode])

    def arr(n, init=None):   # page-aligned host arrays (watchable in lazy mode), as a host program's own fields
        p = stub.stub_calloc(n * 24 * 8)
        a = np.frombuffer((C.c_double * (n * 24)).from_address(p), dtype=np.float64).reshape(n, 4, 3, 2)
        if init is not None:
            a[:] = init
        return a, p

    def host(a):
        if mode == "resident":
            d.tmlqcd_hip_sync_to_host(a[1])
        return a[0].copy()

    out = {}
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
    d.cg_her.restype = C.c_int
    d.cg_her.argtypes = [VP, VP, C.c_int, C.c_double, C.c_int, C.c_int, VP]
    d.Qtm_pm_psi.argtypes = [VP, VP]

    def max_rel(a, b):   # max |a-b| / max |b|, the measure of tests/util.py
        return float(np.abs(a - b).max() / np.abs(b).max())

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
    d.tmlqcd_hip_set_residency(0)
    print(json.dumps(out))
    sys.stdout.flush()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main(sys.argv[1])
