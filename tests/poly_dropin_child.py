"""Child process of tests/test_gpu_poly.py::test_drop_in_symbols_equal_the_core_results and
::test_drop_in_ends_with_a_message_when_phmc_exact_poly_is_set.

A host program in miniature, as tests/nd_dropin_child.py: the stub globals of tests/host_stub/globals.c plus the doublet's and the
polynomial's globals (g_mubar, g_epsbar, phmc_invmaxev, phmc_cheb_evmin, phmc_cheb_evmax, phmc_exact_poly) are loaded first, then
libtmlqcd_dropin.so, so that its weak references bind to them -- which needs a fresh process.  In coherent mode it calls, by name and
with host arrays, assign_mul_add_mul_add_mul_add_mul_r, Ptilde_ndpsi with Qsq = &Qtm_pm_ndpsi and the three tmlqcd_hip_ndpoly_* bodies,
runs the same calls through the core library and prints the largest absolute differences as one JSON line (they must be 0).
Mode "exact_poly" sets phmc_exact_poly = 1 and calls tmlqcd_hip_ndpoly_acc, which must not return."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import HF  # noqa: E402
from tests.util import random_gauge, random_spinor  # noqa: E402

VP, dbl = C.c_void_p, C.c_double
GLOBALS = """
double g_mubar = 0.0, g_epsbar = 0.0, phmc_invmaxev = 1.0, phmc_cheb_evmin = 0.0, phmc_cheb_evmax = 1.0;
int phmc_exact_poly = 0;
void poly_set(double a, double b, double c, double lo, double hi) { g_mubar = a; g_epsbar = b; phmc_invmaxev = c; phmc_cheb_evmin = lo; phmc_cheb_evmax = hi; }
void poly_set_exact(int e) { phmc_exact_poly = e; }
"""
MUBAR, EPSBAR, INVMAXEV, LOCNORM, EVMIN = 0.11, 0.09, 0.71, 1.3, 0.02
KAPPA = 0.125
N_POLY = 5


def main(mode):
    stub, pg, d = hostprog.load(extra_c=GLOBALS, extra_prototypes={"poly_set": (None, [dbl] * 5), "poly_set_exact": (None, [C.c_int])})
    pd_ = C.POINTER(dbl)
    T = L = 4
    V = T * L ** 3
    N = V // 2
    gauge = random_gauge(97, V)
    hostprog.init_lattice(stub, T, L, L, L, gauge, KAPPA)
    stub.stub_set_mu(0.0)
    pg.poly_set(MUBAR, EPSBAR, INVMAXEV, EVMIN, 1.0)
    d.tmlqcd_hip_set_residency(0)                     # coherent only, and tmlqcd_hip_finalize() ends this program
    fields = hostprog.HostFields(stub, d, "coherent")
    arr = lambda init=None: fields.arr(N, init)

    th = np.pi * (np.arange(N_POLY - 1) + 0.5) / (N_POLY - 1)
    roots = np.concatenate([0.8 * np.exp(1j * th), 0.8 * np.exp(-1j * th[::-1])])   # z[2n-3-k] = conj(z[k]), as in the reference's root files
    rflat = np.ascontiguousarray(roots).view(np.float64)
    rp = rflat.ctypes.data_as(pd_)
    rng = np.random.default_rng(4)
    md = np.array([1.9] + list(0.05 * rng.standard_normal(N_POLY - 1)))
    pt = np.array([2.1] + list(0.04 * rng.standard_normal(6)))
    mdp, ptp = md.ctypes.data_as(pd_), pt.ctypes.data_as(pd_)
    hu, hd = random_spinor(11, N), random_spinor(12, N)

    if mode == "exact_poly":
        pg.poly_set_exact(1)
        a, b = arr(hu), arr(hd)
        e1 = dbl()
        d.tmlqcd_hip_ndpoly_acc(a[1], b[1], rp, N_POLY, LOCNORM, INVMAXEV, mdp, ptp, len(pt), EVMIN, 0.0, C.byref(e1))
        print("tmlqcd_hip_ndpoly_acc returned with phmc_exact_poly = 1")
        return

    from tmlqcd_amd import Lattice
    lat = Lattice(T, L, L, L, kappa=KAPPA, mu=0.0)
    lat.set_gauge(gauge)
    lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
    Cpol = float(np.sqrt(LOCNORM))
    errs = {}
    dmax = lambda x, y: float(np.abs(x - y).max())
    # the four-term combination, in place on R
    h = [random_spinor(20 + k, N) for k in range(4)]
    ha = [arr(x) for x in h]
    d.assign_mul_add_mul_add_mul_add_mul_r(ha[0][1], ha[1][1], ha[2][1], ha[3][1], 0.7, -1.3, 0.0, 2.1, N)
    f = [lat.field(x) for x in h]
    lat.assign_mul_add_mul_add_mul_add_mul_r(f[0], f[1], f[2], f[3], 0.7, -1.3, 0.0, 2.1)
    errs["assign_mul_add_mul_add_mul_add_mul_r"] = dmax(ha[0][0], f[0].download())
    # Ptilde_ndpsi
    su, sd, ru, rd = arr(hu), arr(hd), arr(), arr()
    d.Ptilde_ndpsi(ru[1], rd[1], ptp, len(pt), su[1], sd[1], C.cast(d.Qtm_pm_ndpsi, VP))
    fsu, fsd, fru, frd = lat.field(hu), lat.field(hd), lat.field(), lat.field()
    lat.Ptilde_ndpsi(fru, frd, list(pt), fsu, fsd, EVMIN, 1.0)
    errs["Ptilde_ndpsi"] = max(dmax(ru[0], fru.download()), dmax(rd[0], frd.download()))
    # the derivative, into a zeroed hf->derivative
    df_host = np.zeros((V, 4, 8))
    rows = (VP * V)(*[df_host.ctypes.data + 4 * 8 * 8 * i for i in range(V)])      # su3adj **derivative
    hf = HF(None, None, C.cast(rows, VP), 0, 0)
    pu, pd = arr(hu), arr(hd)
    d.tmlqcd_hip_ndpoly_derivative(C.byref(hf), pu[1], pd[1], rp, N_POLY, LOCNORM, INVMAXEV)
    fpu, fpd = lat.field(hu), lat.field(hd)
    lat.derivative_zero()
    lat.ndpoly_derivative(fpu, fpd, roots, Cpol, INVMAXEV)
    errs["ndpoly_derivative"] = dmax(df_host, lat.derivative())
    # the heatbath
    e0 = dbl()
    d.tmlqcd_hip_ndpoly_heatbath(pu[1], pd[1], rp, N_POLY, LOCNORM, INVMAXEV, ptp, len(pt), EVMIN, C.byref(e0))
    e0c = lat.ndpoly_heatbath(fpu, fpd, roots, Cpol, INVMAXEV, list(pt), EVMIN, 1.0)
    errs["ndpoly_heatbath_pf"] = max(dmax(pu[0], fpu.download()), dmax(pd[0], fpd.download()))
    errs["ndpoly_heatbath_energy0"] = abs(e0.value - e0c)
    # the acceptance step on that pf
    e1 = dbl()
    steps = d.tmlqcd_hip_ndpoly_acc(pu[1], pd[1], rp, N_POLY, LOCNORM, INVMAXEV, mdp, ptp, len(pt), EVMIN, 0.0, C.byref(e1))
    e1c, steps_c, _ = lat.ndpoly_acc(fpu, fpd, roots, Cpol, INVMAXEV, list(md), list(pt), EVMIN, 1.0, 0.0)
    errs["ndpoly_acc_energy1"] = abs(e1.value - e1c)
    lat.close()
    d.tmlqcd_hip_finalize()
    hostprog.emit({"errs": errs, "corrections": steps, "corrections_core": steps_c})


if __name__ == "__main__":
    main(sys.argv[1])
