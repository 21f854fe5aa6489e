"""Child process of tests/test_gpu_trlog.py::test_dropin_symbols.

A host program in miniature, as tests/ndsw_dropin_child.py: the stub globals of tests/host_stub/globals.c (with its sw / sw_inv
arrays) are loaded first, then libtmlqcd_dropin.so.  Calls sw_trace / sw_trace_nd under their reference names (a) after
tmlqcd_hip_sw_term, where they read the device's clover term, and (b) after tmlqcd_hip_update_clover with the host's sw array filled
by the CPU oracle, where they upload it first.  Prints |got - want| / sum |per-site term| against tests/cloverrat_restate.py over the
CPU oracle as one JSON line.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import cloverrat_restate as cr  # noqa: E402
from tests import hostprog  # noqa: E402
from tests import ndsw_restate as sw  # noqa: E402
from tests.util import random_gauge  # noqa: E402

dbl = C.c_double


def main():
    from oracle.oraclebind import Oracle
    stub, _, d = hostprog.load()
    shape = (4, 4, 4, 4)
    V = int(np.prod(shape))
    orc = Oracle(*shape, kappa=sw.KAPPA, mu=0.0)
    gauge = random_gauge(sw.shape_seed(shape), orc.VPR)
    orc.set_gauge(gauge)
    cl = cr.clover_of(orc, sw.KAPPA, sw.C_SW)
    hostprog.init_lattice(stub, *shape, gauge, sw.KAPPA)
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
    hostprog.emit(errs)


if __name__ == "__main__":
    main()
