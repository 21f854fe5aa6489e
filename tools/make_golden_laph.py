"""TEST INFRASTRUCTURE ONLY: fixtures of the LapH operator (tests/golden/ref_laph_4x4.npz, ref_laph_8x6x4x12.npz).

Run once on a CPU machine:

    python tools/make_golden_laph.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

jacobi.c, geometry_eo.c and init/init_geometry_indices.c are compiled here, in place from the reference tree, with -DWITHLAPH and the
DEFS of oracle/Makefile into a temporary directory (nothing is copied into this repository) and linked with tools/laph_harness.c.  The
reference's own geometry() fills g_iup3d / g_idn3d and the reference's Jacobi() runs on every time-slice of one colour-vector field.
4^4: the gauge field of ref_mms_4x4.npz (not stored again).  8x6x4x12: tests.util.random_gauge(123456, VOLUME) (made again by the test).
The input vector is numpy.random.default_rng(LAPH_SEED).standard_normal and is stored with the outputs, 48 bytes per site each.

The reference's eigen-driver (solver/eigenvalues_Jacobi.c, LapH_ev.c) cannot be built -- it is empty without LAPACK, needs lime.h
and init/init_jacobi_field.c does not compile with a current gcc -- so eigenvalues are pinned to numpy.linalg.eigvalsh of the dense
matrix of tests/laph_restate.py, which the outputs stored here pin to the reference's object code.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRCS = ["jacobi.c", "geometry_eo.c", "init/init_geometry_indices.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1", "-DWITHLAPH"]
SHAPES = {"4x4": (4, 4, 4, 4), "8x6x4x12": (8, 6, 4, 12)}
LAPH_SEED = 20261


def build_lib(ref, tmp):
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "laph_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmlaph.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-Wl,--no-undefined", "-lm"])
    return so


def gen(tag, so):
    import numpy as np
    sys.path.insert(0, ROOT)
    from tests.util import random_gauge
    dims = SHAPES[tag]
    T, LX, LY, LZ = dims
    V, S3 = T * LX * LY * LZ, LX * LY * LZ
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    lib.tmlaph_init.argtypes = [i, i, i, i]
    lib.tmlaph_set_gauge.argtypes = [vp]
    lib.tmlaph_jacobi.argtypes = [vp, vp, i]
    lib.tmlaph_neighbours.argtypes = [vp, vp]
    assert lib.tmlaph_init(*dims) == 0 and lib.tmlaph_spacevolume() == S3
    gauge_from = "ref_mms_4x4.npz" if tag == "4x4" else "tests.util.random_gauge(123456, VOLUME)"
    gauge = np.load(os.path.join(GOLD, "ref_mms_4x4.npz"))["gauge"] if tag == "4x4" else random_gauge(123456, V)
    gauge = np.ascontiguousarray(gauge[:V], dtype=np.float64)
    lib.tmlaph_set_gauge(gauge.ctypes.data_as(vp))
    k = np.random.default_rng(LAPH_SEED).standard_normal((T, S3, 3, 2))
    l = np.zeros_like(k)
    for t in range(T):
        kt, lt = np.ascontiguousarray(k[t]), np.zeros((S3, 3, 2))
        lib.tmlaph_jacobi(lt.ctypes.data_as(vp), kt.ctypes.data_as(vp), t)
        l[t] = lt
    up, dn = np.zeros((S3, 4), dtype=np.int32), np.zeros((S3, 4), dtype=np.int32)
    lib.tmlaph_neighbours(up.ctypes.data_as(vp), dn.ctypes.data_as(vp))
    np.savez_compressed(os.path.join(GOLD, "ref_laph_%s.npz" % tag), dims=np.array(dims), k=k, l=l, iup3d=up, idn3d=dn,
                        seed=np.array(LAPH_SEED), gauge_from=np.array(gauge_from),
                        run=np.array("Jacobi(l[t], k[t], t) of jacobi.c for every t; geometry() of geometry_eo.c filled g_iup3d / g_idn3d; -DWITHLAPH, gcc -O2"))
    print("%s: |k|^2 %.6e |l|^2 %.6e" % (tag, float((k ** 2).sum()), float((l ** 2).sum())), file=sys.stderr)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "SO"))
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        gen(a.child[0], a.child[1])
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_laph.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for tag in SHAPES:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", tag, so])
