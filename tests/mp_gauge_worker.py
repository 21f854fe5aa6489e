"""One rank of tests/test_gpu_gauge.py::test_drop_in_measures_are_global_on_t_split_ranks: `python mp_gauge_worker.py RANK WORLD JOB OUTDIR`.
A host program on a T-split lattice the way an MPI tmLQCD run is one (g_nproc_t, g_proc_coords, RAND = the two halo slices of the gauge
field) calls the gauge monomial through libtmlqcd_dropin.so after tmlqcd_hip_comm_init_shm: measure_plaquette and measure_gauge_action
under their reference names (the sum over ALL ranks on every rank, as after the reference's MPI_Allreduce), and
tmlqcd_hip_gauge_derivative for its slab, before and after a tmlqcd_hip_update_gauge.  WORLD = 1: the unsplit host program."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys

import numpy as np

faulthandler.enable()
faulthandler.dump_traceback_later(int(os.environ.get("MP_WORKER_TIMEOUT", "240")), exit=True)     # a hung rank says where, and ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tmlqcd_amd import synthetic as syn  # noqa: E402

rank, world, job, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
VP = C.c_void_p
d0 = os.path.join(ROOT, "tests", "host_stub")
so, src = os.path.join(d0, "libtmhost.so"), os.path.join(d0, "globals.c")
if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-o", so + ".%d" % os.getpid(), src, "-lm"])
    os.replace(so + ".%d" % os.getpid(), so)          # (several ranks may get here at once)
stub = C.CDLL(so, mode=C.RTLD_GLOBAL)
import tmlqcd_amd  # noqa: E402
tmlqcd_amd.load_library()
d = C.CDLL(os.path.join(ROOT, "tmlqcd_amd", "lib", "libtmlqcd_dropin.so"), mode=C.RTLD_GLOBAL)


class HF(C.Structure):        # hamiltonian_field.h:26-32
    _fields_ = [("gaugefield", VP), ("momenta", VP), ("derivative", VP), ("update_gauge_copy", C.c_int), ("traj_counter", C.c_int)]


class GaugeInfo(C.Structure):  # io/params.h:98-104, first member
    _fields_ = [("plaquetteEnergy", C.c_double)]


stub.stub_init_rank.restype = VP; stub.stub_init_rank.argtypes = [C.c_int] * 6
stub.stub_boundary.argtypes = [C.c_double] * 5
stub.stub_set_mu.argtypes = [C.c_double]
d.measure_plaquette.restype = C.c_double; d.measure_plaquette.argtypes = [VP]
d.measure_gauge_action.restype = C.c_double; d.measure_gauge_action.argtypes = [VP, C.c_double]
d.tmlqcd_hip_gauge_derivative.restype = None
d.tmlqcd_hip_gauge_derivative.argtypes = [C.POINTER(HF)] + [C.c_double] * 3 + [C.c_int, C.c_double]
d.tmlqcd_hip_update_gauge.restype = None; d.tmlqcd_hip_update_gauge.argtypes = [C.c_double, C.POINTER(HF)]
d.tmlqcd_hip_comm_init_shm.argtypes = [C.c_char_p]

Tg, L = 8, 4
T = Tg // world
V = T * L ** 3
g = syn.gauge_field(51, T, L, L, L, world, rank)                       # [VOLUMEPLUSRAND][4] su3, halo slices filled as xchange_gauge would
VPR = g.shape[0]
gptr = stub.stub_init_rank(T, L, L, L, world, rank)
C.memmove(gptr, g.ctypes.data_as(VP), g.nbytes)
stub.stub_boundary(0.13, 1.0, 0.0, 0.0, 0.0)
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
