"""TEST INFRASTRUCTURE ONLY: fixtures of mixed_cg_mms_tm_nd (tests/golden/ref_mixed_mms_*).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref_hs.so, the half-spinor build of the reference tree and
the only one with the fp32 twins):

    python tools/make_golden_mixed_mms.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

oracle/Makefile does not build solver/mixed_cg_mms_tm_nd.c, solver/cg_mms_tm_nd.c, operator/tm_operators_nd.c,
operator/tm_operators_nd_32.c, linalg/assign_mul_add_mul_r.c, linalg/assign_mul_add_mul_r_32.c or linalg/mul_r_32.c.  They are
compiled here, in place from the reference tree, into a temporary directory (nothing is copied into this repository), linked with
tools/mixed_mms_harness.c against libtmref_hs.so, and run on the seed-123456 random gauge field, the sources of
tests/golden/ref_nd32_* and the doublet parameters and shifts of tests/golden/ref_nd_*.

Every run of RUNS must converge in the reference, one must do a reliable update, one must remove a shift and one must take the
fallback to cg_mms_tm_nd (source scaled below |Q|^2 = 1e-4): the tool checks that before it writes anything.  Reliable updates and
removals are read from the solver's own debug prints.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_nd32 import DEFS, captured   # noqa: E402  the same build of the reference, the same capture of its prints

SRCS = ["solver/mixed_cg_mms_tm_nd.c", "solver/cg_mms_tm_nd.c", "operator/tm_operators_nd.c", "operator/tm_operators_nd_32.c",
        "linalg/assign_mul_add_mul_r.c", "linalg/assign_mul_add_mul_r_32.c", "linalg/mul_r_32.c"]
MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.6931
NFIELDS, DUM = 48, 40
SHIFTS = [0.02, 0.15, 0.6, 2.5, 9.0]          # tests/golden/ref_nd_scalars_8x8.json
MAX_ITER = 2000
# name, eps_sq, rel_prec, factor on the source
RUNS = [("rel_1e-14", 1e-14, 1, 1.0),         # tight enough for rel_delta = 1e-10 to fire
        ("rel_1e-8", 1e-8, 1, 1.0),
        ("abs_1e-9", 1e-9, 0, 1.0),
        ("one_shift", 1e-12, 1, 1.0),         # nshifts = 1: the first shift alone
        ("fallback", 1e-16, 1, 1e-5)]         # |Q|^2 * 1e-10 < 1e-4 on both lattices
CG_MMS = {"eps_sq": 1e-22, "rel_prec": 0}      # the fp64 solve the mixed one is compared with (the precision of ref_nd_*)


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref_hs.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref_hs.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "mixed_mms_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmmixedmms.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref_hs.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def gen(T, L, so, full):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    kappa = 0.125
    r = RefLattice(T, L, L, L, kappa=kappa, mu=0.0, nfields=NFIELDS, hs=True)
    mm = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    mm.tmmm_set.argtypes = [d, d, d]
    mm.tmmm_set_dum.argtypes = [i]
    mm.tmmm_set_debug.argtypes = [i]
    mm.Qtm_pm_ndpsi.argtypes = [vp] * 4
    mm.tmmm_solve.argtypes = [i, C.POINTER(vp), C.POINTER(vp), vp, vp, C.POINTER(d), i, i, d, i, i]
    mm.tmmm_set_dum(DUM)
    mm.tmmm_set(MUBAR, EPSBAR, INVMAXEV)
    r.random_fields(123456)          # the gauge field, then tmref_convert_gauge_32()
    for k in (1, 2):
        r.lib.tmref_random_spinor_eo(k)
    N, sp = r.V // 2, r.sp
    ns = len(SHIFTS)
    q_up, q_dn = r.spinor(1, N).copy(), r.spinor(2, N).copy()
    if full:   # neither the links nor the sources are stored again
        if not np.array_equal(r.gauge(), np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))["gauge"]):
            sys.exit("make_golden_mixed_mms.py: the seed-123456 gauge field differs from the one in tests/golden/ref_nd_4x4.npz")
        f32 = np.load(os.path.join(GOLD, "ref_nd32_4x4.npz"))
        if not (np.array_equal(q_up, f32["q_up"]) and np.array_equal(q_dn, f32["q_dn"])):
            sys.exit("make_golden_mixed_mms.py: the sources differ from those in tests/golden/ref_nd32_4x4.npz")
    QU, QD, AU, AD, X0, P0 = 3, 4, 5, 6, 8, 20      # scaled source, A P, cg_mms_tm_nd solutions, mixed solutions
    sh = (d * ns)(*SHIFTS)

    def ptrs(base, n):
        return (vp * n)(*[sp(base + 2 * k) for k in range(n)]), (vp * n)(*[sp(base + 2 * k + 1) for k in range(n)])

    def residuals(base, n, qu, qd):
        """|Q - (A + shift^2) P_s|^2 / |Q|^2 in fp64 with the reference's own Qtm_pm_ndpsi"""
        out = []
        for k in range(n):
            mm.Qtm_pm_ndpsi(sp(AU), sp(AD), sp(base + 2 * k), sp(base + 2 * k + 1))
            s2 = SHIFTS[k] ** 2
            ru = r.spinor(AU, N) + s2 * r.spinor(base + 2 * k, N) - qu
            rd = r.spinor(AD, N) + s2 * r.spinor(base + 2 * k + 1, N) - qd
            out.append(float(((ru ** 2).sum() + (rd ** 2).sum()) / ((qu ** 2).sum() + (qd ** 2).sum())))
        return out

    scal = {"T": T, "L": L, "kappa": kappa, "seed": 123456, "mubar": MUBAR, "epsbar": EPSBAR, "invmaxev": INVMAXEV, "shifts": SHIFTS,
            "max_iter": MAX_ITER, "cg_mms_tm_nd": dict(CG_MMS), "runs": []}
    arrs = {}
    x_cache = {}
    for name, eps_sq, rel_prec, scale in RUNS:
        n = 1 if name == "one_shift" else ns
        r.spinor(QU)[:N] = scale * q_up
        r.spinor(QD)[:N] = scale * q_dn
        qu, qd = r.spinor(QU, N).copy(), r.spinor(QD, N).copy()
        if (n, scale) not in x_cache:   # the fp64 multi-shift solve of the same source
            up, dn = ptrs(X0, n)
            it64 = mm.tmmm_solve(0, up, dn, sp(QU), sp(QD), sh, n, MAX_ITER, CG_MMS["eps_sq"], CG_MMS["rel_prec"], N)
            x_cache[(n, scale)] = (it64, [(r.spinor(X0 + 2 * k, N).copy(), r.spinor(X0 + 2 * k + 1, N).copy()) for k in range(n)])
        it64, X = x_cache[(n, scale)]
        up, dn = ptrs(P0, n)
        for k in range(2 * n):
            r.spinor(P0 + k)[:] = 7.0                # the solver zeroes P itself
        mm.tmmm_set_debug(4)
        it, log = captured(lambda: mm.tmmm_solve(1, up, dn, sp(QU), sp(QD), sh, n, MAX_ITER, eps_sq, rel_prec, N))
        mm.tmmm_set_debug(0)
        # the iteration of an update is the one whose "mms iteration j = .." line precedes the "triggered a reliable update" line
        updates, removals, j = [], [], -1
        for line in log.splitlines():
            m = re.search(r"CGMMSND_mixed: mms iteration j = (\d+):", line)
            if m:
                j = int(m.group(1))
            m = re.search(r"CGMMSND_mixed: Shift (\d+) with offset squared \S+ triggered a reliable update", line)
            if m:
                updates.append([j, int(m.group(1))])
            m = re.search(r"CGMMSND_mixed: at iteration (\d+) removed one shift, (\d+) remaining", line)
            if m:
                removals.append([int(m.group(1)), int(m.group(2))])
        run = {"name": name, "eps_sq": eps_sq, "rel_prec": rel_prec, "source_scale": scale, "nshifts": n, "iters": it,
               "source_norm": float((qu ** 2).sum() + (qd ** 2).sum()), "fallback": "falling back to double mms solver" in log,
               "reliable_updates": updates, "removals": removals, "got_larger": "got larger after rel. update" in log,
               "cg_mms_tm_nd_iters": it64}
        run["true_residual_rel"] = residuals(P0, n, qu, qd)
        run["distance_to_cg_mms_tm_nd"] = []
        for k in range(n):
            du, dd = r.spinor(P0 + 2 * k, N) - X[k][0], r.spinor(P0 + 2 * k + 1, N) - X[k][1]
            run["distance_to_cg_mms_tm_nd"].append(float(np.sqrt(((du ** 2).sum() + (dd ** 2).sum()) / ((X[k][0] ** 2).sum() + (X[k][1] ** 2).sum()))))
        if full and name == RUNS[0][0]:              # the solutions of one run; the others are pinned by their distances below
            for k in range(n):
                arrs["%s_up_%d" % (name, k)] = r.spinor(P0 + 2 * k, N).copy()
                arrs["%s_dn_%d" % (name, k)] = r.spinor(P0 + 2 * k + 1, N).copy()
        scal["runs"].append(run)
    if full:
        it64, X = x_cache[(ns, 1.0)]
        for k in range(ns):
            arrs["cg_mms_up_%d" % k], arrs["cg_mms_dn_%d" % k] = X[k]
    tag = "%dx%d" % (T, L)
    for run in scal["runs"]:
        print(tag, {k: v for k, v in run.items()})
    # the four conditions on the reference's own runs
    runs = scal["runs"]
    ok = [all(x["iters"] > 0 for x in runs), any(x["reliable_updates"] for x in runs), any(x["removals"] for x in runs),
          any(x["fallback"] and x["source_norm"] < 1e-4 for x in runs), not any(x["fallback"] for x in runs if x["source_scale"] == 1.0)]
    if not all(ok):
        sys.exit("make_golden_mixed_mms.py: %s: converged / reliable update / removal / fallback / no stray fallback = %s" % (tag, ok))
    json.dump(scal, open(os.path.join(GOLD, "ref_mixed_mms_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_mixed_mms_%s.npz" % tag), **arrs)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=2, metavar=("L", "SO"))
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        L = int(a.child[0])
        gen(L, L, a.child[1], L == 4)
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_mixed_mms.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for L in (4, 8):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(L), so])
