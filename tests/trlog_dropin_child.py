"""Child process of tests/test_gpu_trlog.py::test_dropin_symbols.

A host program in miniature, as tests/ndsw_dropin_child.py: the stub globals of tests/host_stub/globals.c (with its sw / sw_inv
arrays) are loaded first, then libtmlqcd_dropin.so.  Calls sw_trace / sw_trace_nd under their reference names (a) after
tmlqcd_hip_sw_term, where they read the device's clover term, and (b) after tmlqcd_hip_update_clover with the host's sw array filled
by the CPU oracle, where they upload it first.  Prints |got - want| / sum |per-site term| against tests/cloverrat_restate.py over the
CPU oracle as one JSON line.
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
from tests import cloverrat_restate as cr  # noqa: E402
from tests import ndsw_restate as sw  # noqa: E402
from tests.util import random_gauge  # noqa: E402

VP, dbl = C.c_void_p, C.c_double


def main():
    from oracle.oraclebind import Oracle
    tmp = tempfile.mkdtemp()
    host = os.path.join(tmp, "libhost.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-o", host, os.path.join(ROOT, "tests", "host_stub", "globals.c"), "-lm"])
    stub = C.CDLL(host, mode=C.RTLD_GLOBAL)
    d = C.CDLL(os.path.join(ROOT, "tmlqcd_amd", "lib", "libtmlqcd_dropin.so"), mode=C.RTLD_GLOBAL)
    stub.stub_init.restype = VP
    stub.stub_init.argtypes = [C.c_int] * 4
    stub.stub_boundary.argtypes = [dbl] * 5
    stub.stub_init_clover.restype = VP
    stub.stub_init_clover.argtypes = [C.c_int]
    d.tmlqcd_hip_sw_term.argtypes = [dbl, dbl]
    d.sw_trace.restype = dbl; d.sw_trace.argtypes = [C.c_int, dbl]
    d.sw_trace_nd.restype = dbl; d.sw_trace_nd.argtypes = [C.c_int, dbl, dbl]
    d.tmlqcd_hip_sw_trace_failures.restype = C.c_int

    shape = (4, 4, 4, 4)
    V = int(np.prod(shape))
    orc = Oracle(*shape, kappa=sw.KAPPA, mu=0.0)
    gauge = random_gauge(sw.shape_seed(shape), orc.VPR)
    orc.set_gauge(gauge)
    cl = cr.clover_of(orc, sw.KAPPA, sw.C_SW)
    g = stub.stub_init(*shape)
    C.memmove(g, gauge.ctypes.data, gauge.nbytes)
    stub.stub_boundary(sw.KAPPA, 0.0, 0.0, 0.0, 0.0)
    swh = stub.stub_init_clover(0)                                      # the host program's sw / sw_inv (init_sw_fields)
    sw_host = np.frombuffer((dbl * (V * 6 * 18)).from_address(swh), dtype=np.float64).reshape(V, 3, 2, 3, 3, 2)
    mub, epsb, _ = sw.FIXTURE

    def cases(tag, errs):
        for ieo in (0, 1):
            for mu in cr.TRACE_MU:
                want, scale = cr.sw_trace(cl, ieo, mu)
                errs["%s_sw_trace_%d_%g" % (tag, ieo, mu)] = abs(d.sw_trace(ieo, mu) - want) / scale
            want, scale = cr.sw_trace_nd(cl, ieo, mub, epsb)
            errs["%s_sw_trace_nd_%d" % (tag, ieo)] = abs(d.sw_trace_nd(ieo, mub, epsb) - want) / scale
        errs["%s_failures" % tag] = float(d.tmlqcd_hip_sw_trace_failures())

    errs = {}
    d.tmlqcd_hip_sw_term(sw.KAPPA, sw.C_SW)                            # (a) the device's clover term is current
    errs["sw_term_host_copy"] = float(np.abs(sw_host - orc.sw_term(sw.KAPPA, sw.C_SW)).max())
    cases("device", errs)
    d.tmlqcd_hip_update_clover()                                       # (b) the host computed sw itself: uploaded on the next call
    sw_host[:] = 0.5 * orc.sw_term(sw.KAPPA, sw.C_SW)                  # half the term: told apart from (a)
    half = cr.Clover(sw_host.copy(), orc.eo2lexic(), orc.Vh, orc.VPR // 2)
    want, scale = cr.sw_trace(half, 0, 0.23)
    errs["upload_sw_trace"] = abs(d.sw_trace(0, 0.23) - want) / scale
    errs["upload_differs"] = abs(want - cr.sw_trace(cl, 0, 0.23)[0]) / scale
    d.tmlqcd_hip_finalize()
    print(json.dumps(errs))
    sys.stdout.flush()


if __name__ == "__main__":
    main()
