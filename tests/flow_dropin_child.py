"""Child process of tests/test_gpu_flow.py::test_through_the_drop_in and ::test_drop_in_ends_the_program_on_an_unopenable_file.

A host program in miniature, as tests/csg_dropin_child.py: the stub globals of tests/host_stub/globals.c are loaded first, then
libtmlqcd_dropin.so.  With the 4^4 RANLUX links of tests/golden/ref_fields_4x4.npz in g_gauge_field and in the residency mode given
on the command line it calls, by name,
  - measure_clover_field_strength_observables(g_gauge_field, &fso),
  - tmlqcd_hip_gradient_flow_measurement(7, 0.02, 0.1), which writes gradflow.000007 into the working directory,
  - in resident mode tmlqcd_hip_update_gauge and the measurement again: the device's moved links are measured, the host's stay behind;
    the moved links are then brought to the host and measured by tests/flow_restate.py,
and prints the results as one JSON line.  Mode "unopenable" finds a directory under the name of the output file and must not return."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import flow_restate as fr  # noqa: E402
from tests import hostprog  # noqa: E402
from tests.hostprog import FSO, HF  # noqa: E402

VP, dbl = C.c_void_p, C.c_double
GOLD = os.path.join(ROOT, "tests", "golden")


def main(mode):
    s = json.load(open(os.path.join(GOLD, "ref_flow_scalars_4x4.json")))
    dims = (4, 4, 4, 4)
    V = 256
    gauge = np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"][:V])
    stub, _, d = hostprog.load()
    gptr = hostprog.init_lattice(stub, *dims, gauge, 0.125)
    stub.stub_set_mu(0.01)
    grows = (VP * V)(*[gptr + 4 * 144 * i for i in range(V)])
    gf = C.cast(grows, VP)
    host_links = np.frombuffer((dbl * (V * 72)).from_address(gptr), dtype=np.float64).reshape(V, 4, 3, 3, 2)

    if mode == "unopenable":
        os.mkdir("gradflow.%06d" % 9)
        d.tmlqcd_hip_gradient_flow_measurement(9, s["eps"], s["tmax"])
        print("tmlqcd_hip_gradient_flow_measurement returned without an output file")
        return

    d.tmlqcd_hip_set_residency(1 if mode == "resident" else 0)
    out = {}
    n0 = d.tmlqcd_hip_calls()
    fso = FSO(0.0, 0.0)
    d.measure_clover_field_strength_observables(gf, C.byref(fso))
    out["E"], out["Q"] = fso.E, fso.Q
    d.tmlqcd_hip_gradient_flow_measurement(s["traj"], s["eps"], s["tmax"])
    out["calls_served"] = int(d.tmlqcd_hip_calls() - n0)
    d.measure_clover_field_strength_observables(gf, C.byref(fso))              # the flow left the links alone
    out["host_links_unchanged"] = bool(np.array_equal(host_links, gauge) and (fso.E, fso.Q) == (out["E"], out["Q"]))
    if mode == "resident":
        mom = np.random.default_rng(296).standard_normal((V, 4, 8))
        df = np.zeros((V, 4, 8))
        mrows = (VP * V)(*[mom.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
        drows = (VP * V)(*[df.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
        hf = HF(gf, C.cast(mrows, VP), C.cast(drows, VP), 0, 0)
        d.tmlqcd_hip_update_gauge(0.04, C.byref(hf))
        n1 = d.tmlqcd_hip_calls()
        d.measure_clover_field_strength_observables(gf, C.byref(fso))
        out["moved_calls"] = int(d.tmlqcd_hip_calls() - n1)
        out["moved_E"], out["moved_Q"] = fso.E, fso.Q
        out["host_links_unchanged"] = bool(out["host_links_unchanged"] and np.array_equal(host_links, gauge))
        d.tmlqcd_hip_set_residency(0)
        d.tmlqcd_hip_sync_gauge_to_host(C.byref(hf))                           # now the host holds the moved links
        moved = np.array(host_links)
        out["moved_want_E"], out["moved_want_Q"] = fr.field_strength(moved, dims)
        out["moved_sum_abs_q"] = fr.sum_abs_q(moved, dims)
    d.tmlqcd_hip_finalize()
    hostprog.emit(out)


if __name__ == "__main__":
    main(sys.argv[1])
