"""Child process of tests/test_gpu_lazy.py::test_faults_of_the_host_program_reach_its_own_handler: a host program whose own SIGSEGV
handler is installed BEFORE the library's.  Prints one line, "OK ..." or the reason it is not."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.util import TOL, random_gauge, random_spinor, rel_err  # noqa: E402

VP = C.c_void_p
stub, _, d = hostprog.load(core_first=True)

T = L = 8
V = T * L ** 3
N = V // 2
g = random_gauge(5, V)
hostprog.init_lattice(stub, T, L, L, L, g, 0.13)
stub.stub_set_mu(0.01)
assert stub.stub_install_segv_probe() == 0                    # the program's handler first ...
assert stub.stub_touch_guard() == 1                           # ... and it works on its own
blk = np.zeros(3 * N * 24 + 64)                               # (an mmap of its own: 3 fields back to back)
f = [blk[8 + i * N * 24: 8 + (i + 1) * N * 24].reshape(N, 4, 3, 2) for i in range(3)]
f[0][:] = random_spinor(6, N)


def p(a):
    return a.ctypes.data_as(VP)


d.tmlqcd_hip_set_residency(0)
d.Hopping_Matrix(0, p(f[2]), p(f[0]))                         # coherent mode: the reference
want = f[2].copy()
d.tmlqcd_hip_set_residency(2)                                 # lazy: the library's handler goes on top, chaining to the program's
d.Hopping_Matrix(0, p(f[1]), p(f[0]))
if stub.stub_touch_guard() != 2:
    print("the program's handler did not see its fault while fields were stale"); sys.exit(1)
if not np.array_equal(f[1], want):                            # the library's faults, served as before
    print("lazy result differs", rel_err(f[1], want)); sys.exit(1)
f[0][3] *= 2.0                                                # a store into the write-protected input
d.Hopping_Matrix(0, p(f[1]), p(f[0]))
d.tmlqcd_hip_set_residency(0)
d.Hopping_Matrix(0, p(f[2]), p(f[0]))
if stub.stub_touch_guard() != 3 or not np.array_equal(f[1], f[2]):
    print("second round failed"); sys.exit(1)
st = (C.c_ulong * 4)(); d.tmlqcd_hip_lazy_stats(st)
d.tmlqcd_hip_finalize()
print("OK program faults 3, library faults %d stores %d" % (st[0], st[3]))
