"""Child process of tests/test_gpu_lazy.py::test_arrays_that_cannot_be_watched: a host program whose spinor arrays live where the lazy
mode must not take pages away -- inside the malloc heap, inside a thread's malloc arena, in a shared mapping.  `python
lazy_unwatchable_child.py heap|arena|shared`: the arrays are recognised (TMLQCD_HIP_LAZY_DEBUG says why), left unwatched, copied per
call, and the results are the coherent mode's.  With TMLQCD_HIP_LAZY_FORCE_WATCH=1 (test hook) they ARE watched: the first fault on one
of them must end the process with a message -- not hang it, which is what a fault taken inside malloc did in round 3."""
import ctypes as C
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.util import random_gauge, random_spinor  # noqa: E402

where = sys.argv[1]
VP = C.c_void_p
stub, _, d = hostprog.load(core_first=True)
libc = C.CDLL(None, use_errno=True)
hostprog.set_prototypes(libc, {"malloc": (VP, [C.c_size_t]), "mmap": (VP, [VP, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long]),
                               "mallopt": (C.c_int, [C.c_int, C.c_int])})

T = L = 8
V = T * L ** 3
N = V // 2
g = random_gauge(5, V)
hostprog.init_lattice(stub, T, L, L, L, g, 0.13)
stub.stub_set_mu(0.01)
nb = 3 * N * 192 + 64
if where == "shared":
    base = libc.mmap(None, (nb + 4095) // 4096 * 4096, 3, 0x21, -1, 0)          # MAP_SHARED | MAP_ANONYMOUS
elif where == "heap":
    libc.mallopt(-3, 1 << 30)                                                    # M_MMAP_THRESHOLD: the PROGRAM keeps big blocks in its heap
    junk = [libc.malloc(1 << 20) for _ in range(4)]
    base = libc.malloc(nb)
else:                                                                            # a thread's arena
    libc.mallopt(-3, 1 << 30)
    box = {}
    th = threading.Thread(target=lambda: box.update(p=libc.malloc(nb)))
    th.start(); th.join()
    base = box["p"]
assert base not in (None, 0, C.c_void_p(-1).value)
blk = np.ctypeslib.as_array(C.cast(base, C.POINTER(C.c_double)), shape=(nb // 8,))
f = [blk[8 + i * N * 24: 8 + (i + 1) * N * 24].reshape(N, 4, 3, 2) for i in range(3)]
f[0][:] = random_spinor(6, N)


def p(a):
    return a.ctypes.data_as(VP)


d.tmlqcd_hip_set_residency(0)
d.Hopping_Matrix(0, p(f[2]), p(f[0]))                         # coherent mode: the reference
want = f[2].copy()
d.tmlqcd_hip_set_residency(2)                                 # lazy
d.Hopping_Matrix(0, p(f[1]), p(f[0]))
got = f[1].copy()                                             # FORCE_WATCH: this load faults on a page that must not be watched -> message + exit
f[0][3] *= 2.0
d.Hopping_Matrix(0, p(f[1]), p(f[0]))
d.tmlqcd_hip_set_residency(0)
d.Hopping_Matrix(0, p(f[2]), p(f[0]))
if not np.array_equal(got, want) or not np.array_equal(f[1], f[2]):
    print("results differ from the coherent mode's"); sys.exit(2)
st = (C.c_ulong * 4)(); d.tmlqcd_hip_lazy_stats(st)
d.tmlqcd_hip_finalize()
print("OK %s: faults served %d" % (where, st[0]))
