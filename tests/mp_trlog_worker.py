"""One rank of tests/test_gpu_trlog.py::test_drop_in_traces_are_global_on_t_split_ranks: `python mp_trlog_worker.py RANK WORLD JOB OUTDIR`.
A host program on a T-split lattice (tests/mp_gauge_worker.py) calls tmlqcd_hip_sw_term and then sw_trace / sw_trace_nd under their
reference names through libtmlqcd_dropin.so after tmlqcd_hip_comm_init_shm: every rank gets the sum over ALL ranks, as after the
reference's MPI_Allreduce (operator/clover_det.c:184,274)."""
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
from tests.cloverrat_restate import SPLIT_CASE  # noqa: E402
from tmlqcd_amd import synthetic as syn  # noqa: E402

rank, world, job, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
VP, dbl = C.c_void_p, C.c_double
d0 = os.path.join(ROOT, "tests", "host_stub")
so, src = os.path.join(d0, "libtmhost.so"), os.path.join(d0, "globals.c")
if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-o", so + ".%d" % os.getpid(), src, "-lm"])
    os.replace(so + ".%d" % os.getpid(), so)          # (several ranks may get here at once)
stub = C.CDLL(so, mode=C.RTLD_GLOBAL)
import tmlqcd_amd  # noqa: E402
tmlqcd_amd.load_library()
d = C.CDLL(os.path.join(ROOT, "tmlqcd_amd", "lib", "libtmlqcd_dropin.so"), mode=C.RTLD_GLOBAL)

stub.stub_init_rank.restype = VP; stub.stub_init_rank.argtypes = [C.c_int] * 6
stub.stub_boundary.argtypes = [dbl] * 5
d.tmlqcd_hip_comm_init_shm.argtypes = [C.c_char_p]
d.tmlqcd_hip_sw_term.argtypes = [dbl, dbl]
d.sw_trace.restype = dbl; d.sw_trace.argtypes = [C.c_int, dbl]
d.sw_trace_nd.restype = dbl; d.sw_trace_nd.argtypes = [C.c_int, dbl, dbl]
d.tmlqcd_hip_sw_trace_failures.restype = C.c_int

(Tg, LX, LY, LZ), seed, kappa, c_sw, mu, (mub, epsb) = SPLIT_CASE
T = Tg // world
g = syn.gauge_field(seed, T, LX, LY, LZ, world, rank)                  # [VOLUMEPLUSRAND][4] su3, halo slices filled as xchange_gauge would
gptr = stub.stub_init_rank(T, LX, LY, LZ, world, rank)
C.memmove(gptr, g.ctypes.data_as(VP), g.nbytes)
stub.stub_boundary(kappa, 0.0, 0.0, 0.0, 0.0)
if world > 1:
    d.tmlqcd_hip_comm_init_shm(job.encode())
d.tmlqcd_hip_sw_term(kappa, c_sw)
res = [d.sw_trace(0, 0.0), d.sw_trace(0, mu), d.sw_trace(1, mu), d.sw_trace_nd(0, mub, epsb), d.sw_trace_nd(1, mub, epsb)]
fails = d.tmlqcd_hip_sw_trace_failures()
d.tmlqcd_hip_finalize()
np.savez(os.path.join(outdir, "trlog_%d_of_%d.npz" % (rank, world)), sums=np.array(res), fails=np.array([fails]))
print("rank %d of %d done" % (rank, world), flush=True)
