"""One rank of tests/test_gpu_trajectory_dropin.py::test_t_split_ranks: `python mp_traj_worker.py RANK WORLD JOB OUTDIR`.
A host program on a T-split lattice the way an MPI tmLQCD run is one (tests/mp_gauge_worker.py) calls the trajectory frame through
libtmlqcd_dropin.so after tmlqcd_hip_comm_init_shm, coherent mode: snapshot, tmlqcd_hip_moment_energy, tmlqcd_hip_update_gauge,
tmlqcd_hip_gauge_snapshot_diff, the plaquette force and tmlqcd_hip_force_norms, tmlqcd_hip_accept_links on links the host has pushed off the
group; then a second snapshot, another update and tmlqcd_hip_reject_links.  What the host sees is saved per rank."""
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
from tests import traj_restate as tj  # noqa: E402

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


class HF(C.Structure):        # hamiltonian_field.h:26-32
    _fields_ = [("gaugefield", VP), ("momenta", VP), ("derivative", VP), ("update_gauge_copy", C.c_int), ("traj_counter", C.c_int)]


P = C.POINTER(HF)
stub.stub_init_rank.restype = VP; stub.stub_init_rank.argtypes = [C.c_int] * 6
stub.stub_boundary.argtypes = [dbl] * 5
stub.stub_set_mu.argtypes = [dbl]
for name, res, args in (("tmlqcd_hip_gauge_snapshot", None, [P]), ("tmlqcd_hip_moment_energy", dbl, [P]), ("tmlqcd_hip_gauge_snapshot_diff", dbl, [P]),
                        ("tmlqcd_hip_accept_links", None, [P, C.c_int]), ("tmlqcd_hip_reject_links", None, [P]),
                        ("tmlqcd_hip_force_norms", None, [P, C.POINTER(dbl), C.POINTER(dbl)]), ("tmlqcd_hip_update_gauge", None, [dbl, P]),
                        ("tmlqcd_hip_gauge_derivative", None, [P, dbl, dbl, dbl, C.c_int, dbl]), ("tmlqcd_hip_comm_init_shm", None, [C.c_char_p])):
    f = getattr(d, name)
    f.restype, f.argtypes = res, args

DIMS = (8, 4, 4, 4)
Tg, L = DIMS[0], DIMS[1]
T, XYZ = Tg // world, L ** 3
V = T * XYZ
sl = lambda a, r: a[(r % world) * V:(r % world + 1) * V]
noisy = tj.noisy_gauge(DIMS)                                         # off the group: the accept has something to do
g = np.ascontiguousarray(np.concatenate([sl(noisy, rank), sl(noisy, rank + 1)[:XYZ], sl(noisy, rank - 1)[V - XYZ:]])) if world > 1 else noisy
VPR = g.shape[0]
gptr = stub.stub_init_rank(T, L, L, L, world, rank)
C.memmove(gptr, g.ctypes.data_as(VP), g.nbytes)
stub.stub_boundary(0.13, 1.0, 0.0, 0.0, 0.0)
stub.stub_set_mu(0.02)
if world > 1:
    d.tmlqcd_hip_comm_init_shm(job.encode())
mom = np.ascontiguousarray(sl(tj.momenta(DIMS), rank))
df = np.zeros((V, 4, 8))
grows = (VP * VPR)(*[gptr + 4 * 144 * i for i in range(VPR)])
mrows = (VP * V)(*[mom.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
drows = (VP * V)(*[df.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
hf = HF(C.cast(grows, VP), C.cast(mrows, VP), C.cast(drows, VP), 0, 0)
host_links = np.frombuffer((dbl * (VPR * 72)).from_address(gptr), dtype=np.float64).reshape(VPR, 4, 3, 3, 2)

res = {}
d.tmlqcd_hip_gauge_snapshot(C.byref(hf))
energy = d.tmlqcd_hip_moment_energy(C.byref(hf))
d.tmlqcd_hip_update_gauge(0.05, C.byref(hf))                         # coherent mode: hf->gaugefield follows
res["moved"] = np.array(host_links)
ddu = d.tmlqcd_hip_gauge_snapshot_diff(C.byref(hf))
d.tmlqcd_hip_gauge_derivative(C.byref(hf), 5.8, 1.0, 0.0, 0, 0.0)    # one contribution: the accumulator holds what hf->derivative received
s, m = dbl(), dbl()
d.tmlqcd_hip_force_norms(C.byref(hf), C.byref(s), C.byref(m))
res["force"] = df.copy()
res["sums"] = np.array([energy, ddu, s.value, m.value])
d.tmlqcd_hip_accept_links(C.byref(hf), 1)
res["accepted"] = np.array(host_links)
d.tmlqcd_hip_gauge_snapshot(C.byref(hf))
d.tmlqcd_hip_update_gauge(-0.03, C.byref(hf))
res["moved_again"] = np.array(host_links)
d.tmlqcd_hip_reject_links(C.byref(hf))
res["rejected"] = np.array(host_links)
res["ddu_after_reject"] = np.array([d.tmlqcd_hip_gauge_snapshot_diff(C.byref(hf))])
d.tmlqcd_hip_finalize()
np.savez(os.path.join(outdir, "traj_%d_of_%d.npz" % (rank, world)), **res)
print("rank %d of %d done" % (rank, world), flush=True)
