"""TEST INFRASTRUCTURE ONLY: fixtures of the Wilson gradient flow (tests/golden/ref_flow_*).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_flow.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

oracle/Makefile builds none of meas/gradient_flow.c, meas/measure_clover_field_strength_observables.c, matrix_utils.c, get_staples.c,
measure_gauge_action.c and aligned_malloc.c.  They are compiled here, in place from the reference tree, into a temporary directory
(nothing is copied into this repository), linked with tools/flow_harness.c against libtmref.so, and run
  4^4        on the seed-123456 RANLUX gauge field (the `gauge` of ref_fields_4x4.npz): the links after 1 and after 6 steps of
             step_gradient_flow at eps = 0.02 (ref_flow_4x4.npz), P, E, Q at t = 0 and after each step, and the rows and the text of
             the gradflow.000007 that gradient_flow_measurement writes for eps = 0.02, tmax = 0.1, traj = 7
  T=6, L=4   on tests.util.random_gauge(64, V): the same scalars
Each JSON also holds `sum_abs_q` (the scale of Q's rounding error, from the restatement tests/flow_restate.py) and `restate_vs_ref`:
the largest absolute deviations of the restatement from the reference after the 6 steps, from which the GPU tests derive their bounds.
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
SRCS = ["meas/gradient_flow.c", "meas/measure_clover_field_strength_observables.c", "matrix_utils.c", "get_staples.c",
        "measure_gauge_action.c", "aligned_malloc.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
EPS, NSTEPS, TMAX, TRAJ = 0.02, 6, 0.1, 7
SEED_6x4 = 64


def build_lib(ref, tmp, omp=False):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref_omp.so" if omp else "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/%s missing: run build() first" % os.path.basename(refso))
    flags = ["-O3", "-march=x86-64-v3", "-fopenmp", "-DTM_USE_OMP=1"] if omp else ["-O2"]
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "flow_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + (".omp.o" if omp else ".o"))
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-I" + ref] + flags + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmflow_omp.so" if omp else "libtmflow.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + (["-fopenmp"] if omp else []) +
                          ["-L" + os.path.dirname(refso), "-l:" + os.path.basename(refso),
                           "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def bind(so):
    fl = C.CDLL(so)
    fl.tmflow_step.argtypes = [C.c_double]
    fl.tmflow_links.argtypes = [C.c_void_p]
    fl.tmflow_observables.argtypes = [C.POINTER(C.c_double)]
    fl.tmflow_observables_resident.argtypes = [C.POINTER(C.c_double)]
    fl.tmflow_measurement.argtypes = [C.c_int, C.c_double, C.c_double]
    fl.tmflow_time.argtypes = [C.c_double, C.c_int]
    fl.tmflow_time.restype = C.c_double
    return fl


def gen(T, L, so, full):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    from tests import flow_restate as fr
    from tests.util import random_gauge
    r = RefLattice(T, L, L, L, kappa=0.125, mu=0.0)
    fl = bind(so)
    V, dims = r.V, (T, L, L, L)
    if full:
        r.random_fields(123456)
        stored = np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"]
        assert np.array_equal(stored[:V], r.gauge()), "the RANLUX field is not the one of ref_fields_4x4.npz"
        gauge_note = "gauge of ref_fields_4x4.npz (RANLUX, seed 123456)"
    else:
        r.gauge()[:] = random_gauge(SEED_6x4, V)
        r.mark_gauge_dirty()
        gauge_note = "tests.util.random_gauge(%d, V)" % SEED_6x4
    g0 = np.array(r.gauge())

    def obs(fn):
        peq = (C.c_double * 3)()
        fn(peq)
        return {"P": peq[0], "E": peq[1], "Q": peq[2]}

    scal = {"T": T, "L": L, "eps": EPS, "nsteps": NSTEPS, "tmax": TMAX, "traj": TRAJ, "gauge": gauge_note,
            "resident": obs(fl.tmflow_observables_resident)}
    fl.tmflow_begin()
    steps, arrs = [obs(fl.tmflow_observables)], {}
    assert steps[0] == scal["resident"]
    for n in range(1, NSTEPS + 1):
        fl.tmflow_step(EPS)
        steps.append(obs(fl.tmflow_observables))
        if n in (1, NSTEPS):
            out = np.zeros((V, 4, 3, 3, 2))
            fl.tmflow_links(out.ctypes.data_as(C.c_void_p))
            arrs["links_step%d" % n] = out
    scal["steps"] = steps                                     # [0] = t 0, [n] = after n steps
    assert np.array_equal(g0, r.gauge()), "the flow modified g_gauge_field"
    # the measurement itself, in a directory of its own
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            fl.tmflow_measurement(TRAJ, EPS, TMAX)
        finally:
            os.chdir(cwd)
        text = open(os.path.join(d, "gradflow.%06d" % TRAJ)).read()
    scal["gradflow_text"] = text
    # the rows in full precision: the same loop on the harness' own steps and measures (the file holds 12 digits)
    fl.tmflow_begin()
    t, P, E, Q = [0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3
    o = obs(fl.tmflow_observables)
    P[2], E[2], Q[2] = o["P"], o["E"], o["Q"]
    rows = []
    while t[1] < TMAX:
        t[0], E[0], Q[0], P[0] = t[2], E[2], Q[2], P[2]
        for step in (1, 2):
            t[step] = t[step - 1] + EPS
            fl.tmflow_step(EPS)
            o = obs(fl.tmflow_observables)
            P[step], E[step], Q[step] = o["P"], o["E"], o["Q"]
        W = t[1] * t[1] * (2 * E[1] + t[1] * ((E[2] - E[0]) / (2 * EPS)))
        rows.append([t[1], P[1], 36 * (1 - P[1]), E[1], t[1] * t[1] * 36 * (1 - P[1]), t[1] * t[1] * E[1], W, Q[1]])
    scal["rows"] = rows
    assert fr.gradflow_text(TRAJ, rows) == text, "the rows rebuilt from the harness do not print as the reference's file"
    # the restatement against the reference
    gr6 = fr.step_gradient_flow(g0, dims, EPS, NSTEPS)
    p, e, q = fr.observables(gr6, dims)
    scal["sum_abs_q"] = fr.sum_abs_q(g0, dims)
    scal["restate_vs_ref"] = {"d_link": float(np.abs(gr6 - arrs["links_step%d" % NSTEPS]).max()), "d_P": float(abs(p - steps[-1]["P"])),
                              "d_E": float(abs(e - steps[-1]["E"])), "d_Q": float(abs(q - steps[-1]["Q"]))}
    print("%dx%d" % (T, L), scal["restate_vs_ref"], "sum_abs_q %.3e" % scal["sum_abs_q"], "rows", len(rows), file=sys.stderr)
    tag = "%dx%d" % (T, L)
    json.dump(scal, open(os.path.join(GOLD, "ref_flow_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_flow_%s.npz" % tag), **arrs)


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
        sys.exit("make_golden_flow.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for T, L in ((4, 4), (6, 4)):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(T), str(L), so])
