"""One rank of tests/test_gpu_trlog.py::test_drop_in_traces_are_global_on_t_split_ranks: `python mp_trlog_worker.py RANK WORLD JOB OUTDIR`.
A host program on a T-split lattice (tests/mp_gauge_worker.py) calls tmlqcd_hip_sw_term and then sw_trace / sw_trace_nd under their
reference names through libtmlqcd_dropin.so after tmlqcd_hip_comm_init_shm: every rank gets the sum over ALL ranks, as after the
reference's MPI_Allreduce (operator/clover_det.c:184,274)."""
import faulthandler
import os
import sys

import numpy as np

faulthandler.enable()
faulthandler.dump_traceback_later(int(os.environ.get("MP_WORKER_TIMEOUT", "240")), exit=True)     # a hung rank says where, and ends

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.cloverrat_restate import SPLIT_CASE  # noqa: E402
from tmlqcd_amd import synthetic as syn  # noqa: E402

rank, world, job, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
stub, _, d = hostprog.load(core_first=True)

(Tg, LX, LY, LZ), seed, kappa, c_sw, mu, (mub, epsb) = SPLIT_CASE
T = Tg // world
g = syn.gauge_field(seed, T, LX, LY, LZ, world, rank)                  # [VOLUMEPLUSRAND][4] su3, halo slices filled as xchange_gauge would
hostprog.init_lattice(stub, T, LX, LY, LZ, g, kappa, rank=(world, rank))
if world > 1:
    d.tmlqcd_hip_comm_init_shm(job.encode())
d.tmlqcd_hip_sw_term(kappa, c_sw)
res = [d.sw_trace(0, 0.0), d.sw_trace(0, mu), d.sw_trace(1, mu), d.sw_trace_nd(0, mub, epsb), d.sw_trace_nd(1, mub, epsb)]
fails = d.tmlqcd_hip_sw_trace_failures()
d.tmlqcd_hip_finalize()
np.savez(os.path.join(outdir, "trlog_%d_of_%d.npz" % (rank, world)), sums=np.array(res), fails=np.array([fails]))
print("rank %d of %d done" % (rank, world), flush=True)
