"""Child process of tests/test_gpu_laph_dropin.py.

A host program in miniature (tests/hostprog.py): the stub globals, then libtmlqcd_dropin.so, in a fresh process.  On 4x2x6x2 it
calls Jacobi on host vectors for every time-slice and tmlqcd_hip_laph_eigensystem, which writes its files into the working
directory (a temporary one), and repeats both through the core library on a lattice of its own with the same links.  It prints one
JSON line: the differences between the two paths and to the NumPy statement, and what the files hold against the Python packing
of the vectors the core library returned."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests import laph_restate as lr  # noqa: E402
from tests.util import random_gauge, rel_err  # noqa: E402

SHAPE = (4, 2, 6, 2)
NEV, PREC, MAX_APPS, NSTORE = 3, 1e-8, 20000, 17


def main():
    stub, _, d = hostprog.load()
    VP, INT, DBL = C.c_void_p, C.c_int, C.c_double
    hostprog.set_prototypes(d, {"Jacobi": (None, [VP, VP, INT]), "tmlqcd_hip_laph_eigensystem": (INT, [INT, DBL, INT, INT])})
    T, LX, LY, LZ = SHAPE
    V, S3 = T * LX * LY * LZ, LX * LY * LZ
    gauge = random_gauge(41, V)
    hostprog.init_lattice(stub, T, LX, LY, LZ, gauge, 0.125)
    rng = np.random.default_rng(6)
    kh = rng.standard_normal((T, S3, 3, 2))
    lh = np.zeros_like(kh)
    for t in range(T):
        kt, lt = np.ascontiguousarray(kh[t]), np.zeros((S3, 3, 2))
        d.Jacobi(lt.ctypes.data_as(VP), kt.ctypes.data_as(VP), t)
        lh[t] = lt
    slices_done = d.tmlqcd_hip_laph_eigensystem(NEV, PREC, MAX_APPS, NSTORE)

    from tmlqcd_amd import Lattice
    lat = Lattice(*SHAPE)
    lat.set_gauge(gauge)
    k, l = lat.cvfield(kh), lat.cvfield()
    lat.laph_apply(l, k)
    core = l.download()
    r = lat.laph_eigensystem(NEV, prec=PREC, max_apps=MAX_APPS, vectors=True)
    vecs = [f.download() for f in r["vectors"]]
    out = {"jacobi_vs_core": float(np.abs(lh - core).max()), "jacobi_vs_numpy": rel_err(lh, lr.apply_field(gauge, SHAPE, kh)),
           "slices_done": slices_done, "core_converged": [int(c) for c in r["converged"]], "files": sorted(os.listdir(".")),
           "vector_bytes_equal": True, "lines_equal": True, "parsed": [], "evals": r["evals"].tolist()}
    for t in range(T):
        lines = open("eigenvalues.%.3d.%.4d" % (t, NSTORE)).read().splitlines()
        out["lines_equal"] = out["lines_equal"] and lines == ["%e" % e for e in r["evals"][t]]
        out["parsed"].append([float(x) for x in lines])
        for i in range(NEV):
            data = open("eigenvector.%.3d.%.3d.%.4d" % (i, t, NSTORE), "rb").read()
            out["vector_bytes_equal"] = out["vector_bytes_equal"] and data == np.ascontiguousarray(vecs[i][t]).tobytes()
    lat.close()
    d.tmlqcd_hip_finalize()
    hostprog.emit(out)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp_dir:
        os.chdir(tmp_dir)
        main()
