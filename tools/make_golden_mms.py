"""TEST INFRASTRUCTURE ONLY: fixtures of the single-flavour multi-shift CG (tests/golden/ref_mms_*).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_mms.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

oracle/Makefile does not build solver/cg_mms_tm.c or linalg/assign_mul_add_mul_r.c.  They are compiled here, in place from the
reference tree, into a temporary directory (nothing is copied into this repository), linked with tools/mms_harness.c against
libtmref.so, and run on the existing seed-123456 random gauge field.  The drop schedule is read off the reference's own
g_debug_level > 2 output (cg_mms_tm.c:150-152).  Cases (CASES below):
  qtm        Qtm_pm_psi, mu != 0, five shifts, eps_sq 1e-22 absolute: the last shift is dropped
  qsw        Qsw_pm_psi, c_sw > 0, mu != 0 (sw_term + sw_invert(EE, mu) of the reference)
  qpm_full   Q_pm_psi on VOLUME sites set up as invert_eo.c:463-490 does: g_mu = 0, shifts = {mu, three extra masses}
  qtm_rel    Qtm_pm_psi with rel_prec = 1
  qtm_cut    Qtm_pm_psi cut off by max_iter: returns -1
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
SRCS = ["solver/cg_mms_tm.c", "linalg/assign_mul_add_mul_r.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
NFIELDS = 40
KAPPA, MU, C_SW = 0.125, 0.02, 1.2        # MU is g_mu = 2 kappa mu as the reference stores it
# name: (op 0 Qtm_pm_psi / 1 Qsw_pm_psi / 2 Q_pm_psi, g_mu, shifts, eps_sq, rel_prec, max_iter)
# qpm_full runs FIRST: init_mms_tm (cg_mms_tm.c:207-228) keeps its shifted fields from an earlier call whenever that call had as
# many shifts, whatever their size, so a VOLUME solve behind a VOLUME/2 one would work on overlapping fields
CASES = {
    "qpm_full": (2, 0.0, [MU, 0.05, 0.3, 1.5], 1e-20, 0, 1000),
    "qtm": (0, MU, [0.02, 0.15, 0.6, 2.5, 9.0], 1e-22, 0, 1000),
    "qsw": (1, MU, [0.03, 0.2, 1.1, 4.0], 1e-22, 0, 1000),
    "qtm_rel": (0, MU, [0.02, 0.4, 3.0], 1e-18, 1, 1000),
    "qtm_cut": (0, MU, [0.02, 0.4, 3.0], 1e-22, 0, 15),
}


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "mms_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmmms.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def run_captured(fn):
    """fn() with the process's stdout captured (the reference prints its drop schedule there)"""
    with tempfile.TemporaryFile() as cap:
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(cap.fileno(), 1)
        try:
            out = fn()
        finally:
            C.CDLL(None).fflush(None)
            os.dup2(saved, 1)
            os.close(saved)
        cap.seek(0)
        return out, cap.read().decode()


def gen(T, L, so, full):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    r = RefLattice(T, L, L, L, kappa=KAPPA, mu=MU, nfields=NFIELDS)
    mm = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    mm.tmmms_cg_mms_tm.argtypes = [C.POINTER(vp), vp, C.POINTER(d), i, i, d, i, i, i, C.POINTER(d)]
    mm.tmmms_set_debug.argtypes = [i]
    mm.tmmms_set_sloppy.argtypes = [i]
    r.random_fields(123456)
    r.lib.tmref_random_spinor_eo(0)                               # the e/o source
    V, N = r.V, r.V // 2
    rng = np.random.default_rng(20261016)
    r.spinor(1)[:] = rng.standard_normal((V, 4, 3, 2))            # the full-lattice source (lexicographic)
    lib = r.lib
    scal = {"T": T, "L": L, "kappa": KAPPA, "c_sw": C_SW, "seed": 123456, "cases": {}}
    arrs = {}
    if full:
        arrs["gauge"] = r.gauge().copy()
        arrs["q_eo"] = r.spinor(0, N).copy()
        arrs["q_full"] = r.spinor(1, V).copy()
    clover_ready = False
    for name, (op, gmu, shifts, eps_sq, rel, max_iter) in CASES.items():
        if op == 1 and not clover_ready:
            r.set_kappa_mu(KAPPA, gmu)
            r.clover(C_SW, gmu)
            clover_ready = True
        r.set_kappa_mu(KAPPA, gmu)
        n = len(shifts)
        sites = V if op == 2 else N
        first = 2                                                  # solution fields 2 .. 2 + n - 1 (< DUM_DERI = NFIELDS - 4)
        for k in range(n):
            r.spinor(first + k)[:] = 7.0                           # any content: cg_mms_tm ignores it
        P = (vp * n)(*[r.sp(first + k) for k in range(n)])
        sh = (d * n)(*shifts)
        reached = d(-1.0)
        mm.tmmms_set_sloppy(1)
        mm.tmmms_set_debug(3)
        it, log = run_captured(lambda: mm.tmmms_cg_mms_tm(P, r.sp(1 if op == 2 else 0), sh, n, max_iter, eps_sq, rel, sites, op,
                                                          C.byref(reached)))
        mm.tmmms_set_debug(0)
        drops = [[int(m.group(1)), int(m.group(2))] for m in re.finditer(r"at iteration (\d+) removed one shift, (\d+) remaining", log)]
        norms = [lib.square_norm(r.sp(first + k), sites, 0) for k in range(n)]
        scal["cases"][name] = {"op": ["Qtm_pm_psi", "Qsw_pm_psi", "Q_pm_psi"][op], "g_mu": gmu, "shifts": shifts, "eps_sq": eps_sq,
                               "rel_prec": rel, "max_iter": max_iter, "iters": it, "reached_prec": reached.value, "drops": drops,
                               "active_at_exit": n - len(drops), "sol_norms": norms, "sloppy_after": mm.tmmms_get_sloppy()}
        if full:
            for k in range(n):
                arrs["%s_P%d" % (name, k)] = r.spinor(first + k, sites).copy()
        print("%dx%d %-9s iters %4d drops %s reached %.3e" % (T, L, name, it, drops, reached.value), file=sys.stderr)
    tag = "%dx%d" % (T, L)
    json.dump(scal, open(os.path.join(GOLD, "ref_mms_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_mms_%s.npz" % tag), **arrs)


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
        sys.exit("make_golden_mms.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for L in (4, 8):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(L), so])
