"""One rank of tests/test_gpu_gauge.py::test_drop_in_measures_are_global_on_t_split_ranks: `python mp_gauge_worker.py RANK WORLD JOB OUTDIR`.
A host program on a T-split lattice the way an MPI tmLQCD run is one (g_nproc_t, g_proc_coords, RAND = the two halo slices of the gauge
field) calls the gauge monomial through libtmlqcd_dropin.so after tmlqcd_hip_comm_init_shm: measure_plaquette and measure_gauge_action
under their reference names (the sum over ALL ranks on every rank, as after the reference's MPI_Allreduce), and
tmlqcd_hip_gauge_derivative for its slab, before and after a tmlqcd_hip_update_gauge.  WORLD = 1: the unsplit host program."""
import ctypes as C
import faulthandler
import os
import sys

import numpy as np

faulthandler.enable()
faulthandler.dump_traceback_later(int(os.environ.get("MP_WORKER_TIMEOUT", "240")), exit=True)     # a hung rank says where, and ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import HF, GaugeInfo  # noqa: E402
from tmlqcd_amd import synthetic as syn  # noqa: E402

rank, world, job, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
VP = C.c_void_p
stub, _, d = hostprog.load(core_first=True)

Tg, L = 8, 4
T = Tg // world
V = T * L ** 3
g = syn.gauge_field(51, T, L, L, L, world, rank)                       # [VOLUMEPLUSRAND][4] su3, halo slices filled as xchange_gauge would
VPR = g.shape[0]
gptr = hostprog.init_lattice(stub, T, L, L, L, g, 0.13, (1.0, 0.0, 0.0, 0.0), rank=(world, rank))
stub.stub_set_mu(0.02)
if world > 1:
    d.tmlqcd_hip_comm_init_shm(job.encode())
mom_all = np.random.default_rng(52).standard_normal((Tg * L ** 3, 4, 8))
mom = np.ascontiguousarray(mom_all[rank * V:(rank + 1) * V])
df = np.zeros((V, 4, 8))
grows = (VP * VPR)(*[gptr + 4 * 144 * i for i in range(VPR)])
mrows = (VP * V)(*[mom.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
drows = (VP * V)(*[df.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
hf = HF(C.cast(grows, VP), C.cast(mrows, VP), C.cast(drows, VP), 0, 0)
gf = C.cast(grows, VP)

res = {}
for tag in ("start", "moved"):
    if tag == "moved":
        d.tmlqcd_hip_update_gauge(0.05, C.byref(hf))                     # coherent mode: the new links reach the neighbours' halo slabs on the device
    a = d.measure_gauge_action(gf, 0.3)
    res[tag + "_sums"] = np.array([d.measure_plaquette(gf), a, GaugeInfo.in_dll(d, "GaugeInfo").plaquetteEnergy])
    df[:] = 0.0
    d.tmlqcd_hip_gauge_derivative(C.byref(hf), 5.8, 1.0, 0.0, 0, 0.3)
    res[tag + "_force"] = df.copy()
d.tmlqcd_hip_finalize()
np.savez(os.path.join(outdir, "gauge_%d_of_%d.npz" % (rank, world)), **res)
print("rank %d of %d done" % (rank, world), flush=True)
