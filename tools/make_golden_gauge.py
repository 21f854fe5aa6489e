"""TEST INFRASTRUCTURE ONLY: fixtures of the gauge monomial (tests/golden/ref_gauge_*).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_gauge.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

oracle/Makefile builds none of monomial/gauge_monomial.c, get_staples.c, get_rectangle_staples.c, measure_gauge_action.c and
measure_rectangles.c.  They are compiled here, in place from the reference tree, into a temporary directory (nothing is copied into
this repository), linked with tools/gauge_harness.c against libtmref.so, and run
  4^4        on the seed-123456 RANLUX gauge field (the `gauge` of ref_fields_4x4.npz): full derivative fields and scalars
  T=6, L=4   on tests.util.random_gauge(SEED_6x4, V): scalars and checksums of the derivative fields only
Every derivative starts from the seeded non-zero field tests.gauge_restate.seed_derivative(V), as a force that accumulates must.
Cases: wilson (beta 6, plaquette only), iwasaki (c1 = -0.331, c0 = 1 - 8 c1), and both through gauge_EMderivative with lambda 0.3.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRCS = ["monomial/gauge_monomial.c", "get_staples.c", "get_rectangle_staples.c", "measure_gauge_action.c", "measure_rectangles.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
BETA, C1, LAMBDA = 6.0, -0.331, 0.3
SEED_6x4 = 64
# name: (use_rectangles, glambda, through gauge_EMderivative)
CASES = {"wilson": (0, 0.0, 0), "iwasaki": (1, 0.0, 0), "em_wilson": (0, LAMBDA, 1), "em_iwasaki": (1, LAMBDA, 1)}


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "gauge_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmgauge.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def gen(T, L, so, full):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    from tests.gauge_restate import checksums, seed_derivative
    from tests.util import random_gauge
    r = RefLattice(T, L, L, L, kappa=0.125, mu=0.0)
    gl = C.CDLL(so)
    d, i = C.c_double, C.c_int
    gl.tmgauge_setup.argtypes = [d, d, d, i, d]
    gl.tmgauge_derivative.argtypes = [i, C.c_void_p]
    gl.tmgauge_action.argtypes = [d]
    for n in ("tmgauge_heatbath", "tmgauge_c0", "tmgauge_plaquette", "tmgauge_action", "tmgauge_plaquette_energy", "tmgauge_rectangles"):
        getattr(gl, n).restype = d
    V = r.V
    if full:
        r.random_fields(123456)
        stored = np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"]
        assert np.array_equal(stored[:V], r.gauge()), "the RANLUX field is not the one of ref_fields_4x4.npz"
        gauge_note = "gauge of ref_fields_4x4.npz (RANLUX, seed 123456)"
    else:
        r.gauge()[:] = random_gauge(SEED_6x4, V)
        r.mark_gauge_dirty()
        gauge_note = "tests.util.random_gauge(%d, V)" % SEED_6x4
    scal = {"T": T, "L": L, "beta": BETA, "c1": C1, "lambda": LAMBDA, "gauge": gauge_note,
            "measure_plaquette": gl.tmgauge_plaquette(), "measure_gauge_action_0": gl.tmgauge_action(0.0),
            "measure_gauge_action_lambda": gl.tmgauge_action(LAMBDA)}
    scal["plaquetteEnergy_after_lambda"] = gl.tmgauge_plaquette_energy()
    scal["measure_rectangles"] = gl.tmgauge_rectangles()
    arrs = {}
    scal["cases"] = {}
    for name, (rect, lam, em) in CASES.items():
        gl.tmgauge_setup(BETA, 1.0, C1 if rect else 0.0, rect, lam)
        e0 = gl.tmgauge_heatbath()                       # sets c0 = 1 - 8 c1 with rectangles, as a run does before any force
        c0 = gl.tmgauge_c0()
        df = np.zeros((V, 4, 8))                          # VOLUMEPLUSRAND == VOLUME without MPI
        df[:] = seed_derivative(V)
        gl.tmgauge_derivative(em, df.ctypes.data_as(C.c_void_p))
        scal["cases"][name] = {"use_rectangles": rect, "glambda": lam, "em": em, "c0": c0, "c1": C1 if rect else 0.0,
                               "energy0": e0, "checksums": checksums(df)}
        if full:
            arrs[name] = df
        print("%dx%d %-10s energy0 %.15e" % (T, L, name, e0), file=sys.stderr)
    tag = "%dx%d" % (T, L)
    json.dump(scal, open(os.path.join(GOLD, "ref_gauge_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_gauge_%s.npz" % tag), **arrs)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=3, metavar=("T", "L", "SO"))
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        T, L = int(a.child[0]), int(a.child[1])
        gen(T, L, a.child[2], T == 4)
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_gauge.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for T, L in ((4, 4), (6, 4)):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(T), str(L), so])
