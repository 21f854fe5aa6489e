"""Child process of tests/test_gpu_cloverrat.py::test_dropin_symbols.

A host program in miniature, as tests/ndsw_dropin_child.py: the stub globals of tests/host_stub/globals.c (with its sw / sw_inv arrays)
are loaded first, then libtmlqcd_dropin.so.  Calls tmlqcd_hip_sw_term, tmlqcd_hip_sw_invert(EE, 0.) and the three CLOVERRAT bodies
tmlqcd_hip_cloverrat_derivative / _acc / _heatbath with host arrays in the residency mode given on the command line, with g_mu != 0
(the bodies run at twisted mass 0 and leave g_mu alone), and prints the errors against the core library's results on the same inputs
as one JSON line.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ndsw_restate as sw  # noqa: E402
from tests.util import random_gauge, random_spinor  # noqa: E402

VP, dbl = C.c_void_p, C.c_double
MU3, RMU3 = [0.21, 0.6, 1.7], [0.05, 0.4, 1.3]
NU3, RNU3 = [0.15, 0.5, 1.4], [0.04, 0.3, 0.9]
SOLVE = (2000, 1e-24, 1)
G_MU = 0.17


class HF(C.Structure):        # hamiltonian_field.h:26-32
    _fields_ = [("gaugefield", VP), ("momenta", VP), ("derivative", VP), ("update_gauge_copy", C.c_int), ("traj_counter", C.c_int)]


def main(mode):
    tmp = tempfile.mkdtemp()
    host = os.path.join(tmp, "libhost.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-o", host, os.path.join(ROOT, "tests", "host_stub", "globals.c"), "-lm"])
    stub = C.CDLL(host, mode=C.RTLD_GLOBAL)
    d = C.CDLL(os.path.join(ROOT, "tmlqcd_amd", "lib", "libtmlqcd_dropin.so"), mode=C.RTLD_GLOBAL)
    stub.stub_init.restype = VP
    stub.stub_init.argtypes = [C.c_int] * 4
    stub.stub_boundary.argtypes = [dbl] * 5
    stub.stub_set_mu.argtypes = [dbl]
    stub.stub_get_mu.restype = dbl
    stub.stub_calloc.restype = VP
    stub.stub_calloc.argtypes = [C.c_size_t]
    stub.stub_init_clover.restype = VP
    stub.stub_init_clover.argtypes = [C.c_int]
    pd_ = C.POINTER(dbl)
    d.tmlqcd_hip_sw_term.argtypes = [dbl, dbl]
    d.tmlqcd_hip_sw_invert.argtypes = [C.c_int, dbl]
    d.tmlqcd_hip_set_residency.argtypes = [C.c_int]
    d.tmlqcd_hip_sync_to_host.argtypes = [VP]
    d.tmlqcd_hip_flush_derivative.argtypes = [C.POINTER(HF)]
    d.tmlqcd_hip_sw_invert_failures.restype = C.c_int
    d.tmlqcd_hip_cloverrat_derivative.restype = C.c_int
    d.tmlqcd_hip_cloverrat_derivative.argtypes = [C.POINTER(HF), VP, pd_, pd_, C.c_int, dbl, dbl, C.c_int, C.c_int, dbl, C.c_int]
    d.tmlqcd_hip_cloverrat_heatbath.restype = C.c_int
    d.tmlqcd_hip_cloverrat_heatbath.argtypes = [VP, pd_, pd_, C.c_int, C.c_int, dbl, C.c_int, pd_]
    d.tmlqcd_hip_cloverrat_acc.restype = C.c_int
    d.tmlqcd_hip_cloverrat_acc.argtypes = [VP, pd_, pd_, C.c_int, C.c_int, dbl, C.c_int, pd_]

    shape = (4, 4, 4, 4)
    V = int(np.prod(shape))
    N = V // 2
    kappa, c_sw = sw.KAPPA, sw.C_SW
    gauge = random_gauge(sw.shape_seed(shape), V)
    g = stub.stub_init(*shape)
    C.memmove(g, gauge.ctypes.data, gauge.nbytes)
    stub.stub_boundary(kappa, *sw.THETA)
    stub.stub_set_mu(G_MU)
    stub.stub_init_clover(1)                                            # the host program's sw / sw_inv (init_sw_fields)
    d.tmlqcd_hip_set_residency({"coherent": 0, "resident": 1}[mode])

    def arr(init=None):
        p = stub.stub_calloc(N * 24 * 8)
        a = np.frombuffer((dbl * (N * 24)).from_address(p), dtype=np.float64).reshape(N, 4, 3, 2)
        if init is not None:
            a[:] = init
        return a, p

    def host_copy(a):
        if mode == "resident":
            d.tmlqcd_hip_sync_to_host(a[1])
        return a[0].copy()

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

    errs = {}
    d.tmlqcd_hip_sw_term(kappa, c_sw)
    d.tmlqcd_hip_sw_invert(0, 0.0)
    errs["sw_invert_failures"] = float(d.tmlqcd_hip_sw_invert_failures())
    pf = arr(h)
    df_host = np.random.default_rng(96).standard_normal((V, 4, 8))
    start = df_host.copy()
    rows = (VP * V)(*[df_host.ctypes.data + 4 * 8 * 8 * i for i in range(V)])      # su3adj **derivative
    hf = HF(None, None, C.cast(rows, VP), 0, 0)
    mu, rmu = (dbl * 3)(*MU3), (dbl * 3)(*RMU3)
    nu, rnu = (dbl * 3)(*NU3), (dbl * 3)(*RNU3)
    it = d.tmlqcd_hip_cloverrat_derivative(C.byref(hf), pf[1], mu, rmu, 3, kappa, c_sw, 1, *SOLVE)
    errs["cloverrat_derivative_iters"] = abs(it - it_d)
    if mode == "resident":
        errs["cloverrat_derivative_held_back"] = float(np.abs(df_host - start).max())
        d.tmlqcd_hip_flush_derivative(C.byref(hf))
    errs["cloverrat_derivative"] = float(np.abs(df_host - (start + ref)).max() / np.abs(start + ref).max())
    e = dbl()
    it = d.tmlqcd_hip_cloverrat_acc(pf[1], mu, rmu, 3, *SOLVE, C.byref(e))
    errs["cloverrat_acc_iters"] = abs(it - it_a)
    errs["cloverrat_acc"] = abs(e.value - e1_ref) / abs(e1_ref)
    it = d.tmlqcd_hip_cloverrat_heatbath(pf[1], nu, rnu, 3, *SOLVE, C.byref(e))
    errs["cloverrat_heatbath_iters"] = abs(it - it_h)
    errs["cloverrat_heatbath_energy"] = abs(e.value - e0_ref) / abs(e0_ref)
    errs["cloverrat_heatbath"] = float(np.abs(host_copy(pf) - pf_ref).max() / np.abs(pf_ref).max())
    errs["g_mu_moved"] = abs(stub.stub_get_mu() - G_MU)
    d.tmlqcd_hip_set_residency(0)
    print(json.dumps(errs))
    sys.stdout.flush()


if __name__ == "__main__":
    main(sys.argv[1])
