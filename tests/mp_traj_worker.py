"""One rank of tests/test_gpu_trajectory_dropin.py::test_t_split_ranks: `python mp_traj_worker.py RANK WORLD JOB OUTDIR`.
A host program on a T-split lattice the way an MPI tmLQCD run is one (tests/mp_gauge_worker.py) calls the trajectory frame through
libtmlqcd_dropin.so after tmlqcd_hip_comm_init_shm, coherent mode: snapshot, tmlqcd_hip_moment_energy, tmlqcd_hip_update_gauge,
tmlqcd_hip_gauge_snapshot_diff, the plaquette force and tmlqcd_hip_force_norms, tmlqcd_hip_accept_links on links the host has pushed off the
group; then a second snapshot, another update and tmlqcd_hip_reject_links.  What the host sees is saved per rank."""
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
from tests import traj_restate as tj  # noqa: E402
from tests.hostprog import HF  # noqa: E402

rank, world, job, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
VP, dbl = C.c_void_p, C.c_double
stub, _, d = hostprog.load(core_first=True)

DIMS = (8, 4, 4, 4)
Tg, L = DIMS[0], DIMS[1]
T, XYZ = Tg // world, L ** 3
V = T * XYZ
sl = lambda a, r: a[(r % world) * V:(r % world + 1) * V]
noisy = tj.noisy_gauge(DIMS)                                         # off the group: the accept has something to do
g = np.ascontiguousarray(np.concatenate([sl(noisy, rank), sl(noisy, rank + 1)[:XYZ], sl(noisy, rank - 1)[V - XYZ:]])) if world > 1 else noisy
VPR = g.shape[0]
gptr = hostprog.init_lattice(stub, T, L, L, L, g, 0.13, (1.0, 0.0, 0.0, 0.0), rank=(world, rank))
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
