"""TEST INFRASTRUCTURE ONLY: fixtures of the online measurements other than the gradient flow (tests/golden/ref_meas_scalars_*).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_meas.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

oracle/Makefile builds none of meas/correlators.c, meas/pion_norm.c, meas/polyakov_loop.c, meas/oriented_plaquettes.c,
source_generation.c and linalg/convert_eo_to_lexic.c.  They are compiled here, in place from the reference tree, into a temporary
directory (nothing is copied into this repository), linked with tools/meas_harness.c against libtmref.so, and run
  4^4        on the seed-123456 RANLUX gauge field (the `gauge` of ref_fields_4x4.npz)
  T=6, L=4   on tests.util.random_gauge(SEED_6x4, V)
with the propagator tests.util.random_spinor(seed, V/2) for the even and for the odd half (seeds in the JSON).
meas/correlators.c includes operator.h, which reaches c-lime's lime.h through io/utils.h for pointer types only; c-lime is not part
of the reference tree and not installed, so three forward declarations are written into the temporary directory under that name.

Route taken for pion_norm_measurement: invert_eo CAN be stubbed at link time (the harness defines it), so both correlator
measurements run unmodified on the given propagator and their files are recorded; the source slices t0 / z0 they draw from RANLUX
are identified from the files (the one slice whose rebuilt text equals the file).  The raw per-slice sums, which the files hold to
six digits only, come from the harness's loop over the reference's own macros.
polyakov_loop keeps its Kahan accumulators in static variables it never resets, so directions 2 and 3 are taken from two loaded
copies of the harness library.

Each JSON holds scalars and file texts only, `sum_abs` per quantity (the sum over sites or lines of the absolute contribution, from
tests/meas_restate.py) and `restate_vs_ref`, the deviation of that restatement from the reference.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRCS = ["meas/correlators.c", "meas/pion_norm.c", "meas/polyakov_loop.c", "meas/oriented_plaquettes.c", "source_generation.c",
        "linalg/convert_eo_to_lexic.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
LIME_H = ("#ifndef LIME_TYPES_ONLY_H\n#define LIME_TYPES_ONLY_H\n#include <stdio.h>\n#include <stdint.h>\n"
          "typedef struct LimeWriter LimeWriter;\ntypedef struct LimeReader LimeReader;\ntypedef struct LimeRecordHeader LimeRecordHeader;\n#endif\n")
KAPPA, MU, TRAJ = 0.137, 0.01, 7
SEED_6x4 = 65
PROP_SEEDS = {4: (71, 72), 6: (73, 74)}


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    inc = os.path.join(tmp, "inc")
    os.mkdir(inc)
    open(os.path.join(inc, "lime.h"), "w").write(LIME_H)
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "meas_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-I" + ref, "-I" + inc, "-O2"] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmmeas.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:" + os.path.basename(refso),
                                                                  "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    shutil.copy(so, os.path.join(tmp, "libtmmeas_second.so"))
    return so


def bind(so):
    pd = C.POINTER(C.c_double)
    ml = C.CDLL(so)
    ml.tmmeas_set_propagator.argtypes = [C.c_void_p, C.c_void_p]
    ml.tmmeas_correlators.argtypes = [C.c_int, C.c_double, C.c_double]
    ml.tmmeas_pion_norm.argtypes = [C.c_int]
    ml.tmmeas_slice_sums.argtypes = [C.c_int, pd, pd, pd]
    ml.tmmeas_polyakov_loop_dir.argtypes = [C.c_int, C.c_int]
    ml.tmmeas_polyakov_loop.argtypes = [C.c_int, pd]
    ml.tmmeas_oriented_plaquettes.argtypes = [pd]
    ml.tmmeas_oriented_plaquettes_measurement.argtypes = [C.c_int]
    return ml


def gen(T, L, so):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    from tests import meas_restate as mr
    from tests.util import random_gauge, random_spinor
    r = RefLattice(T, L, L, L, kappa=KAPPA, mu=MU)
    ml, ml2 = bind(so), bind(os.path.join(os.path.dirname(so), "libtmmeas_second.so"))
    V, dims = r.V, (T, L, L, L)
    pd = C.POINTER(C.c_double)
    if T == 4:
        r.random_fields(123456)
        stored = np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"]
        assert np.array_equal(stored[:V], r.gauge()), "the RANLUX field is not the one of ref_fields_4x4.npz"
        gauge_note = "gauge of ref_fields_4x4.npz (RANLUX, seed 123456)"
    else:
        r.gauge()[:] = random_gauge(SEED_6x4, V)
        r.mark_gauge_dirty()
        gauge_note = "tests.util.random_gauge(%d, V)" % SEED_6x4
    g0 = np.array(r.gauge())
    se, so_ = PROP_SEEDS[T]
    even, odd = random_spinor(se, V // 2), random_spinor(so_, V // 2)
    ml.tmmeas_set_propagator(even.ctypes.data, odd.ctypes.data)
    scal = {"T": T, "L": L, "kappa": KAPPA, "mu": MU, "traj": TRAJ, "gauge": gauge_note, "prop_seeds": [se, so_],
            "prop": "tests.util.random_spinor(seed, V/2) for the even and the odd half",
            "pion_norm_route": "pion_norm_measurement run unmodified, invert_eo stubbed at link time by tools/meas_harness.c"}

    # ---- slice sums: raw values from the harness's loop over the reference's macros
    pp, pa, p4, pz = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(L)
    ml.tmmeas_slice_sums(0, pp.ctypes.data_as(pd), pa.ctypes.data_as(pd), p4.ctypes.data_as(pd))
    ml.tmmeas_slice_sums(3, pz.ctypes.data_as(pd), None, None)
    scal["slices"] = {"dir0": {"pp": pp.tolist(), "pa": pa.tolist(), "p4": p4.tolist()}, "dir3": {"pp": pz.tolist()}}
    r0, r3 = mr.slice_sums(even, odd, dims, 0), mr.slice_sums(even, odd, dims, 3)
    sum_abs = {"dir0": {k: r0["sum_abs_" + k].tolist() for k in ("pp", "pa", "p4")}, "dir3": {"pp": r3["sum_abs_pp"].tolist()}}
    dev = {"slices_dir0": {k: float(np.abs(r0[k] - v).max()) for k, v in (("pp", pp), ("pa", pa), ("p4", p4))},
           "slices_dir3": {"pp": float(np.abs(r3["pp"] - pz).max())}}

    # ---- the two correlator measurements themselves, and everything else that writes files, in a directory of its own
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            ml.tmmeas_correlators(TRAJ, KAPPA, MU)
            ml.tmmeas_pion_norm(TRAJ)
            assert ml.tmmeas_polyakov_loop_dir(0, 0) == 0 and ml.tmmeas_polyakov_loop_dir(0, 3) == 0
            assert ml.tmmeas_polyakov_loop_dir(0, 1) == -1
            ml.tmmeas_oriented_plaquettes_measurement(TRAJ)
        finally:
            os.chdir(cwd)
        scal["onlinemeas_text"] = open(os.path.join(d, "onlinemeas.%06d" % TRAJ)).read()
        scal["pionnorm_text"] = open(os.path.join(d, "pionnormcorrelator_finiteT.%06d" % TRAJ)).read()
        scal["polyakovloop_dir0_text"] = open(os.path.join(d, "polyakovloop_dir0")).read()
        scal["polyakovloop_dir3_text"] = open(os.path.join(d, "polyakovloop_dir3")).read()
        scal["oriented_line"] = open(os.path.join(d, "oriented_plaquettes.data")).read()
    t0s = [t for t in range(T) if mr.onlinemeas_text(pp, pa, p4, t, KAPPA, dims) == scal["onlinemeas_text"]]
    z0s = [z for z in range(L) if mr.pionnorm_text(pz, z, dims) == scal["pionnorm_text"]]
    assert len(t0s) == 1 and len(z0s) == 1, (t0s, z0s)
    scal["t0"], scal["z0"] = t0s[0], z0s[0]
    assert np.array_equal(g0, r.gauge())

    # ---- Polyakov loop: %25.16e prints 17 significant digits, which gives the double back exactly
    pol, pol_abs = {}, {}
    for dir_ in (0, 3):
        f = scal["polyakovloop_dir%d_text" % dir_].split()
        assert int(f[0]) == 0 and int(f[1]) == dir_
        pol["dir%d" % dir_] = [float(f[2]), float(f[3])]
    for lib, mu in ((ml, 2), (ml2, 3)):
        pl = np.zeros(2)
        lib.tmmeas_polyakov_loop(mu, pl.ctypes.data_as(pd))
        pol["loop%d" % mu] = pl.tolist()
    scal["polyakov"] = pol
    dev["polyakov"] = {}
    for dir_ in range(4):
        v, sa = mr.polyakov_loop(g0, dims, dir_)
        pol_abs[str(dir_)] = sa
        for key in ("dir%d" % dir_, "loop%d" % dir_):
            if key in pol:
                dev["polyakov"][key] = abs(v - complex(*pol[key]))
    sum_abs["polyakov"] = pol_abs

    # ---- oriented plaquettes
    pq = np.zeros(6)
    ml.tmmeas_oriented_plaquettes(pq.ctypes.data_as(pd))
    scal["oriented"] = pq.tolist()
    v, sa = mr.oriented_plaquettes(g0, dims)
    sum_abs["oriented"] = sa
    dev["oriented"] = float(np.abs(np.array(v) - pq).max())
    assert mr.oriented_line(TRAJ, pq) == scal["oriented_line"]

    scal["sum_abs"], scal["restate_vs_ref"] = sum_abs, dev
    print("%dx%d" % (T, L), "t0", scal["t0"], "z0", scal["z0"], dev, file=sys.stderr)
    json.dump(scal, open(os.path.join(GOLD, "ref_meas_scalars_%dx%d.json" % (T, L)), "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=3, metavar=("T", "L", "SO"))
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        gen(int(a.child[0]), int(a.child[1]), a.child[2])
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_meas.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for T, L in ((4, 4), (6, 4)):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(T), str(L), so])
