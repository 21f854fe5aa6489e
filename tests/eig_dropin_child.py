"""Child process of tests/test_gpu_eig_dropin.py.

A host program in miniature, as tests/poly_dropin_child.py: the stub globals of tests/host_stub/globals.c plus the doublet's
globals, even_odd_flag and a Qtm_pm_ndbipsi that aborts when called (the drop-in may only take its address) are loaded first,
then libtmlqcd_dropin.so, so that its weak references bind to them -- which needs a fresh process.  In the residency mode given
on the command line ("lazy" or "resident") it calls, on 4x2x6x2, eigenvalues_bi with &Qtm_pm_ndbipsi for both ends,
tmlqcd_hip_phmc_compute_ev twice (inside its bounds, then with EVMin above the minimum and phmc_invmaxev so large that the
maximum exceeds 1) and tmlqcd_hip_eigenvalues with host vectors, and prints one JSON line: the values, the dense spectrum of
the CPU oracle's operators they are held against, the lines of monomial-03.data and the residuals of the returned vectors
through the oracle's Qtm_pm_psi.  Markers on stderr separate the two phmc_compute_ev calls for the parent."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import nd_restate as nd  # noqa: E402
from tests import hostprog  # noqa: E402
from tests.util import random_gauge  # noqa: E402

VP, dbl, INT = C.c_void_p, C.c_double, C.c_int
GLOBALS = """
#include <stdlib.h>
double g_mubar = 0.0, g_epsbar = 0.0, phmc_invmaxev = 1.0;
int even_odd_flag = 1;
void eig_set(double a, double b, double c) { g_mubar = a; g_epsbar = b; phmc_invmaxev = c; }
void Qtm_pm_ndbipsi(void *l, void *k) { (void)l; (void)k; abort(); }
void some_other_operator(void *l, void *k) { (void)l; (void)k; abort(); }
"""
SHAPE = (4, 2, 6, 2)
KAPPA, MU = 0.13, 0.01
THETA = (1.0, 0.3, -0.2, 0.5)
MUBAR, EPSBAR = 0.1375, 0.1175
PREC = 1e-9


def _dense(A, dim):
    M = np.zeros((dim, dim), dtype=np.complex128)
    e = np.zeros(dim, dtype=np.complex128)
    for j in range(dim):
        e[j] = 1.0
        M[:, j] = A(e)
        e[j] = 0.0
    return np.linalg.eigvalsh(0.5 * (M + M.conj().T))


def main(mode):
    stub, eg, d = hostprog.load(extra_c=GLOBALS, extra_prototypes={"eig_set": (None, [dbl] * 3)})
    pd_ = C.POINTER(dbl)

    if mode == "other_pointer":
        T, LX, LY, LZ = SHAPE
        stub.stub_init(T, LX, LY, LZ)
        nev = INT(1)
        d.eigenvalues_bi(C.byref(nev), 10, PREC, 0, C.cast(eg.some_other_operator, VP))
        print("eigenvalues_bi returned for a pointer it does not know")
        return

    from oracle.oraclebind import Oracle
    T, LX, LY, LZ = SHAPE
    V = T * LX * LY * LZ
    N = V // 2
    orc = Oracle(T, LX, LY, LZ, kappa=KAPPA, mu=MU, theta=THETA, threads=1)
    gauge = random_gauge(97, orc.VPR)
    orc.set_gauge(gauge)
    hostprog.init_lattice(stub, T, LX, LY, LZ, gauge, KAPPA, THETA)
    stub.stub_set_mu(MU)
    d.tmlqcd_hip_set_residency(hostprog.MODES[mode])   # (no way back at the end: tmlqcd_hip_finalize() ends this program)

    # the dense spectra: the doublet at invmaxev = 1 (its eigenvalues scale with invmaxev^2) and Qtm_pm_psi
    H = nd.hop_over(orc.Hopping_Matrix, N)
    n = 12 * N

    def A_nd(x):
        u, dn = nd.Qtm_pm_ndpsi(H, x[:n].reshape(N, 4, 3), x[n:].reshape(N, 4, 3), MUBAR, EPSBAR, 1.0)
        return np.concatenate([u.reshape(-1), dn.reshape(-1)])

    def A_one(x):
        out = orc.new_field()
        orc.op("Qtm_pm_psi", out, nd.real(x.reshape(N, 4, 3)))
        return nd.cplx(out[:N]).reshape(-1)
    lam_nd, lam_one = _dense(A_nd, 2 * n), _dense(A_one, n)
    c_in = float(np.sqrt(0.9 / lam_nd[-1]))           # the spectrum inside [.., 0.9]
    c_out = float(np.sqrt(1.2 / lam_nd[-1]))          # the maximum at 1.2
    out = {"lam_nd_min": lam_nd[0] * c_in ** 2, "lam_nd_max": lam_nd[-1] * c_in ** 2, "lam_nd_min_out": lam_nd[0] * c_out ** 2,
           "lam_nd_max_out": lam_nd[-1] * c_out ** 2, "lam_one": list(lam_one[:2]), "lam_one_max": lam_one[-1]}

    eg.eig_set(MUBAR, EPSBAR, c_in)
    fn = C.cast(eg.Qtm_pm_ndbipsi, VP)
    nev = INT(1)
    out["bi_min"] = d.eigenvalues_bi(C.byref(nev), 1000, PREC, 0, fn)
    out["bi_min_nev"] = nev.value
    nev = INT(1)
    out["bi_max"] = d.eigenvalues_bi(C.byref(nev), 1000, PREC, 1, fn)
    out["bi_max_nev"] = nev.value
    nev = INT(1)
    d.eigenvalues_bi(C.byref(nev), 1, PREC, 0, fn)    # one restart cannot converge: *nev reports it
    out["bi_capped_nev"] = nev.value

    evmin_in = 0.5 * out["lam_nd_min"]
    lo, hi = dbl(), dbl()
    sys.stderr.write("--- inside\n"); sys.stderr.flush()
    assert d.tmlqcd_hip_phmc_compute_ev(7, 3, b"ndpoly_heavy", evmin_in, 0, PREC, C.byref(lo), C.byref(hi)) == 0
    out["ev_in"] = [lo.value, hi.value, evmin_in]
    eg.eig_set(MUBAR, EPSBAR, c_out)
    evmin_out = 2.0 * out["lam_nd_min_out"]
    sys.stderr.write("--- outside\n"); sys.stderr.flush()
    assert d.tmlqcd_hip_phmc_compute_ev(8, 3, b"ndpoly_heavy", evmin_out, 0, PREC, C.byref(lo), C.byref(hi)) == 0
    sys.stderr.write("--- end\n"); sys.stderr.flush()
    out["ev_out"] = [lo.value, hi.value, evmin_out]
    out["file"] = open("monomial-03.data").read().splitlines()

    # the single-flavour call with host vectors
    want = 2
    p = stub.stub_calloc(want * N * 24 * 8)
    vecs = np.frombuffer((dbl * (want * N * 24)).from_address(p), dtype=np.float64).reshape(want, N, 4, 3, 2)
    evals = np.zeros(want)
    nev = INT(want)
    first = d.tmlqcd_hip_eigenvalues(C.byref(nev), 1000, PREC, 0, p, evals.ctypes.data_as(pd_))
    if mode == "resident":
        for i in range(want):
            d.tmlqcd_hip_sync_to_host(p + i * N * 24 * 8)
    res, norms = [], []
    for i in range(want):
        v = nd.cplx(vecs[i]).reshape(-1)
        res.append(float(np.linalg.norm(A_one(v) - evals[i] * v)))
        norms.append(float(np.linalg.norm(v)))
    out.update({"one_first": first, "one_evals": list(evals), "one_nev": nev.value, "one_resid": res, "one_norms": norms})
    d.tmlqcd_hip_finalize()
    hostprog.emit(out)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp_dir:
        os.chdir(tmp_dir)                             # monomial-03.data lands here
        try:
            main(sys.argv[1])
        finally:
            os.chdir(ROOT)
