"""Child process of tests/test_gpu_cloverrat.py::test_dropin_symbols.

A host program in miniature (tests/hostprog.py): the stub globals of tests/host_stub/globals.c (with its sw / sw_inv arrays)
are loaded first, then libtmlqcd_dropin.so.  Calls tmlqcd_hip_sw_term, tmlqcd_hip_sw_invert(EE, 0.) and the three CLOVERRAT bodies
tmlqcd_hip_cloverrat_derivative / _acc / _heatbath with host arrays in the residency mode given on the command line, with g_mu != 0
(the bodies run at twisted mass 0 and leave g_mu alone), and prints the errors against the core library's results on the same inputs
as one JSON line.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests import ndsw_restate as sw  # noqa: E402
from tests.hostprog import HF, rel_max  # noqa: E402
from tests.util import random_gauge, random_spinor  # noqa: E402

VP, dbl = C.c_void_p, C.c_double
MU3, RMU3 = [0.21, 0.6, 1.7], [0.05, 0.4, 1.3]
NU3, RNU3 = [0.15, 0.5, 1.4], [0.04, 0.3, 0.9]
SOLVE = (2000, 1e-24, 1)
G_MU = 0.17


def main(mode):
    stub, _, d = hostprog.load()
    shape = (4, 4, 4, 4)
    V = int(np.prod(shape))
    N = V // 2
    kappa, c_sw = sw.KAPPA, sw.C_SW
    gauge = random_gauge(sw.shape_seed(shape), V)
    hostprog.init_lattice(stub, *shape, gauge, kappa, sw.THETA)
    stub.stub_set_mu(G_MU)
    stub.stub_init_clover(1)                                            # the host program's sw / sw_inv (init_sw_fields)
    errs = {}
    with hostprog.HostFields(stub, d, mode, modes=("coherent", "resident")) as hf:
        # the core library on the same inputs
        from tmlqcd_amd import Lattice
        h = random_spinor(21, N)
        lat = Lattice(*shape, kappa=kappa, mu=G_MU, theta=sw.THETA)
        lat.set_gauge(gauge)
        lat.sw_term(gauge, kappa, c_sw)
        lat.sw_invert(0, 0.0)
        lat.derivative_zero()
        it_d = lat.cloverrat_derivative(lat.field(h), MU3, RMU3, kappa, c_sw, 1, *SOLVE)
        ref = lat.derivative()
        e1_ref, it_a = lat.cloverrat_acc(lat.field(h), MU3, RMU3, *SOLVE)
        fh = lat.field(h)
        e0_ref, it_h = lat.cloverrat_heatbath(fh, NU3, RNU3, *SOLVE)
        pf_ref = fh.download()
        lat.close()

        d.tmlqcd_hip_sw_term(kappa, c_sw)
        d.tmlqcd_hip_sw_invert(0, 0.0)
        errs["sw_invert_failures"] = float(d.tmlqcd_hip_sw_invert_failures())
        pf = hf.arr(N, h)
        df_host = np.random.default_rng(96).standard_normal((V, 4, 8))
        start = df_host.copy()
        rows = (VP * V)(*[df_host.ctypes.data + 4 * 8 * 8 * i for i in range(V)])      # su3adj **derivative
        hfield = HF(None, None, C.cast(rows, VP), 0, 0)
        mu, rmu = (dbl * 3)(*MU3), (dbl * 3)(*RMU3)
        nu, rnu = (dbl * 3)(*NU3), (dbl * 3)(*RNU3)
        it = d.tmlqcd_hip_cloverrat_derivative(C.byref(hfield), pf[1], mu, rmu, 3, kappa, c_sw, 1, *SOLVE)
        errs["cloverrat_derivative_iters"] = abs(it - it_d)
        if mode == "resident":
            errs["cloverrat_derivative_held_back"] = float(np.abs(df_host - start).max())
            d.tmlqcd_hip_flush_derivative(C.byref(hfield))
        errs["cloverrat_derivative"] = rel_max(df_host, start + ref)
        e = dbl()
        it = d.tmlqcd_hip_cloverrat_acc(pf[1], mu, rmu, 3, *SOLVE, C.byref(e))
        errs["cloverrat_acc_iters"] = abs(it - it_a)
        errs["cloverrat_acc"] = abs(e.value - e1_ref) / abs(e1_ref)
        it = d.tmlqcd_hip_cloverrat_heatbath(pf[1], nu, rnu, 3, *SOLVE, C.byref(e))
        errs["cloverrat_heatbath_iters"] = abs(it - it_h)
        errs["cloverrat_heatbath_energy"] = abs(e.value - e0_ref) / abs(e0_ref)
        errs["cloverrat_heatbath"] = rel_max(hf.copy(pf), pf_ref)
        errs["g_mu_moved"] = abs(stub.stub_get_mu() - G_MU)
    hostprog.emit(errs)


if __name__ == "__main__":
    main(sys.argv[1])
