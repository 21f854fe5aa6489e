"""Child process of tests/test_gpu_meas.py::test_through_the_drop_in and ::test_drop_in_on_unopenable_files.

A host program in miniature, as tests/flow_dropin_child.py: the stub globals of tests/host_stub/globals.c are loaded first, then
libtmlqcd_dropin.so.  With the 4^4 RANLUX links of tests/golden/ref_fields_4x4.npz in g_gauge_field, the propagator of
tests/golden/ref_meas_scalars_4x4.json in two host arrays and the residency mode given on the command line it calls, by name,
  - tmlqcd_hip_slice_correlators(even, odd, 0, pp, pa, p4) and (even, odd, 3, pz, NULL, NULL), each twice,
  - oriented_plaquettes_measurement(7, 0, 0) twice and measure_oriented_plaquettes(g_gauge_field, plaq),
  - tmlqcd_hip_polyakov_loop_dir(0, 0), (1, 0), (0, 3) and (0, 1), and tmlqcd_hip_polyakov_loop(pl, dir) for the four directions,
and prints the results as one JSON line; the files are left in the working directory.  Modes "unopenable_oriented" and
"unopenable_polyakov" find a directory under the name of the output file: the first must not return, the second returns -1."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import PD, VP  # noqa: E402
from tests.util import random_spinor  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main(mode):
    s = json.load(open(os.path.join(GOLD, "ref_meas_scalars_4x4.json")))
    dims = (4, 4, 4, 4)
    V = 256
    gauge = np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"][:V])
    even, odd = random_spinor(s["prop_seeds"][0], V // 2), random_spinor(s["prop_seeds"][1], V // 2)
    stub, _, d = hostprog.load()
    gptr = hostprog.init_lattice(stub, *dims, gauge, s["kappa"])
    stub.stub_set_mu(s["mu"])
    grows = (VP * V)(*[gptr + 4 * 144 * i for i in range(V)])
    gf = C.cast(grows, VP)

    if mode == "unopenable_oriented":
        os.mkdir("oriented_plaquettes.data")
        d.oriented_plaquettes_measurement(9, 3, 0)
        print("oriented_plaquettes_measurement returned without an output file")
        return
    if mode == "unopenable_polyakov":
        os.mkdir("polyakovloop_dir3")
        print(json.dumps({"rc": d.tmlqcd_hip_polyakov_loop_dir(0, 3)}))
        d.tmlqcd_hip_finalize()
        return

    d.tmlqcd_hip_set_residency(1 if mode == "resident" else 0)
    out = {}
    n0 = d.tmlqcd_hip_calls()
    runs = []
    for _ in range(2):
        pp, pa, p4, pz = np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4)
        d.tmlqcd_hip_slice_correlators(even.ctypes.data, odd.ctypes.data, 0, pp.ctypes.data_as(PD), pa.ctypes.data_as(PD), p4.ctypes.data_as(PD))
        d.tmlqcd_hip_slice_correlators(even.ctypes.data, odd.ctypes.data, 3, pz.ctypes.data_as(PD), None, None)
        runs.append((pp.tolist(), pa.tolist(), p4.tolist(), pz.tolist()))
    out["pp"], out["pa"], out["p4"], out["pz"] = runs[0]
    out["slices_repeat"] = runs[0] == runs[1]
    d.oriented_plaquettes_measurement(s["traj"], 0, 0)
    d.oriented_plaquettes_measurement(s["traj"] + 1, 0, 0)
    pq = np.zeros(6)
    d.measure_oriented_plaquettes(gf, pq.ctypes.data_as(PD))
    out["oriented"] = pq.tolist()
    out["rc"] = [d.tmlqcd_hip_polyakov_loop_dir(0, 0), d.tmlqcd_hip_polyakov_loop_dir(1, 0), d.tmlqcd_hip_polyakov_loop_dir(0, 3),
                 d.tmlqcd_hip_polyakov_loop_dir(0, 1)]
    out["polyakov"] = []
    for dir_ in range(4):
        pl = np.zeros(2)
        d.tmlqcd_hip_polyakov_loop(pl.ctypes.data_as(PD), dir_)
        out["polyakov"].append(pl.tolist())
    out["calls_served"] = int(d.tmlqcd_hip_calls() - n0)
    d.tmlqcd_hip_finalize()
    hostprog.emit(out)


if __name__ == "__main__":
    main(sys.argv[1])
