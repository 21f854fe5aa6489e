"""One rank of tests/test_gpu_multiprocess.py::test_drop_in_symbols_on_t_split_ranks: `python mp_dropin_worker.py RANK WORLD JOB OUTDIR`.
A host program on a T-split lattice the way an MPI tmLQCD run is one (g_nproc_t, g_proc_coords, RAND = the two halo slices of the gauge
field): it calls the REFERENCE-NAMED symbols of libtmlqcd_dropin.so -- Hopping_Matrix, Qtm_pm_psi, square_norm / scalar_prod_r with
parallel = 1, cg_her with a function pointer -- after tmlqcd_hip_comm_init_shm.  WORLD = 1: the unsplit host program."""
import ctypes as C
import os
import sys

import faulthandler

import numpy as np

faulthandler.enable()
faulthandler.dump_traceback_later(int(os.environ.get("MP_WORKER_TIMEOUT", "240")), exit=True)     # a hung rank says where, and ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tmlqcd_amd import synthetic as syn  # noqa: E402

rank, world, job, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
VP = C.c_void_p
stub, _, d = hostprog.load(core_first=True)

Tg, L = 8, 8
T = Tg // world
N = T * L ** 3 // 2
g = syn.gauge_field(41, T, L, L, L, world, rank)                       # [VOLUMEPLUSRAND][4] su3, halo slices filled as xchange_gauge would
hostprog.init_lattice(stub, T, L, L, L, g, 0.13, (1.0, 0.0, 0.0, 0.0), rank=(world, rank))
stub.stub_set_mu(0.02)
if world > 1:
    d.tmlqcd_hip_comm_init_shm(job.encode())
    if os.environ.get("MP_FACES") == "direct":
        assert d.tmlqcd_hip_comm_init_ipc() == 0


def p(a):
    return a.ctypes.data_as(VP)


res = {}
modes = [m for m in ((0, "coherent"), (2, "lazy")) if str(m[0]) in os.environ.get("MP_DROPIN_MODES", "02")]
for mode, tag in modes:
    d.tmlqcd_hip_set_residency(mode)
    sys.stderr.write("rank %d: %s\n" % (rank, tag)); sys.stderr.flush()
    k = syn.spinor_field_eo(42, 0, T, L, L, L, world, rank)
    b = syn.spinor_field_eo(43, 1, T, L, L, L, world, rank)
    l, x = np.zeros_like(k), np.zeros_like(k)
    d.Hopping_Matrix(1, p(l), p(k)); res[tag + "_hop"] = l.copy()
    d.Qtm_pm_psi(p(l), p(k)); res[tag + "_qtm"] = l.copy()
    res[tag + "_sums"] = np.array([d.square_norm(p(l), N, 1), d.scalar_prod_r(p(l), p(k), N, 1), d.square_norm(p(l), N, 0)])
    it = d.cg_her(p(x), p(b), 2000, 1e-18, 1, N, C.cast(d.Qtm_pm_psi, VP))
    res[tag + "_cg"] = x.copy(); res[tag + "_it"] = np.array([it])
d.tmlqcd_hip_set_residency(0)
d.tmlqcd_hip_finalize()
np.savez(os.path.join(outdir, "dropin_%d_of_%d.npz" % (rank, world)), **res)
print("rank %d of %d done" % (rank, world), flush=True)
