"""TEST INFRASTRUCTURE ONLY: fixtures of the non-degenerate twisted-mass doublet (tests/golden/ref_nd_*).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_nd.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

oracle/Makefile does not build operator/tm_operators_nd.c, solver/cg_her_nd.c, solver/cg_mms_tm_nd.c or
linalg/assign_mul_add_mul_r.c.  They are compiled here, in place from the reference tree, into a temporary directory
(nothing is copied into this repository), linked with tools/nd_harness.c against libtmref.so, and run on the
existing seed-123456 random gauge field with non-trivial g_mubar, g_epsbar and phmc_invmaxev.
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
SRCS = ["operator/tm_operators_nd.c", "solver/cg_her_nd.c", "solver/cg_mms_tm_nd.c", "linalg/assign_mul_add_mul_r.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
# the parameters of the fixtures (g_mubar, g_epsbar are 2 kappa mubar, 2 kappa epsbar as the reference stores them)
MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.6931
NFIELDS, DUM = 40, 32
SHIFTS = [0.02, 0.15, 0.6, 2.5, 9.0]


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "nd_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmnd.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def gen(T, L, so, full, shifts_out):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    kappa = 0.125
    r = RefLattice(T, L, L, L, kappa=kappa, mu=0.0, nfields=NFIELDS)
    nd = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    nd.tmnd_set.argtypes = [d, d, d]
    nd.tmnd_set_dum.argtypes = [i]
    nd.tmnd_set_debug.argtypes = [i]
    for n in ("Qtm_ndpsi", "Qtm_dagger_ndpsi", "Qtm_pm_ndpsi"):
        getattr(nd, n).argtypes = [vp] * 4
    nd.M_ee_inv_ndpsi.argtypes = [vp] * 4 + [d, d]
    nd.M_oo_sub_g5_ndpsi.argtypes = [vp] * 6 + [d, d]
    nd.H_eo_tm_ndpsi.argtypes = [vp] * 4 + [i]
    nd.cg_her_nd.argtypes = [vp] * 4 + [i, d, i, i, vp]
    nd.tmnd_cg_mms_tm_nd.argtypes = [C.POINTER(vp), C.POINTER(vp), vp, vp, C.POINTER(d), i, i, d, i, i]
    nd.tmnd_set_dum(DUM)
    nd.tmnd_set(MUBAR, EPSBAR, INVMAXEV)
    r.random_fields(123456)
    for k in (1, 2, 3):
        r.lib.tmref_random_spinor_eo(k)
    lib, N, sp = r.lib, r.V // 2, r.sp
    scal = {"T": T, "L": L, "kappa": kappa, "seed": 123456, "mubar": MUBAR, "epsbar": EPSBAR, "invmaxev": INVMAXEV}
    arrs = {}
    if full:
        arrs["gauge"] = r.gauge().copy()
        for k, name in enumerate(("k_s", "k_c", "j_s", "j_c")):
            arrs[name] = r.spinor(k, N).copy()
    nd.M_ee_inv_ndpsi(sp(4), sp(5), sp(0), sp(1), MUBAR, EPSBAR)
    nd.M_oo_sub_g5_ndpsi(sp(6), sp(7), sp(0), sp(1), sp(2), sp(3), MUBAR, EPSBAR)
    nd.Qtm_ndpsi(sp(8), sp(9), sp(0), sp(1))
    nd.Qtm_dagger_ndpsi(sp(10), sp(11), sp(0), sp(1))
    nd.Qtm_pm_ndpsi(sp(12), sp(13), sp(0), sp(1))
    pairs = {"M_ee_inv_ndpsi": (4, 5), "M_oo_sub_g5_ndpsi": (6, 7), "Qtm_ndpsi": (8, 9), "Qtm_dagger_ndpsi": (10, 11), "Qtm_pm_ndpsi": (12, 13)}
    for ieo in (0, 1):
        nd.H_eo_tm_ndpsi(sp(14), sp(15), sp(0), sp(1), ieo)
        for f, fl in ((14, "s"), (15, "c")):
            if full:
                arrs["H_eo_tm_ndpsi_%d_%s" % (ieo, fl)] = r.spinor(f, N).copy()
    for name, (a, b) in pairs.items():
        scal["norm_" + name] = lib.square_norm(sp(a), N, 0) + lib.square_norm(sp(b), N, 0)
        if full:
            arrs[name + "_s"] = r.spinor(a, N).copy()
            arrs[name + "_c"] = r.spinor(b, N).copy()
    # cg_her_nd(P, Q = (k_s, k_c)) on Qtm_pm_ndpsi from a zero start (nddetratio_monomial.c:63-65)
    eps_sq, rel = 1e-20, 1
    r.spinor(16)[:] = 0
    r.spinor(17)[:] = 0
    it = nd.cg_her_nd(sp(16), sp(17), sp(0), sp(1), 1000, eps_sq, rel, N, C.cast(nd.Qtm_pm_ndpsi, vp))
    scal["cg_her_nd"] = {"eps_sq": eps_sq, "rel_prec": rel, "max_iter": 1000, "iters": it,
                         "sol_norm": lib.square_norm(sp(16), N, 0) + lib.square_norm(sp(17), N, 0)}
    if full:
        arrs["cg_her_nd_up"] = r.spinor(16, N).copy()
        arrs["cg_her_nd_dn"] = r.spinor(17, N).copy()
    # cg_mms_tm_nd with len(SHIFTS) shifts; the number of shifts left is read off the reference's own debug output
    ns = len(SHIFTS)
    up = (vp * ns)(*[sp(18 + 2 * k) for k in range(ns)])
    dn = (vp * ns)(*[sp(19 + 2 * k) for k in range(ns)])
    sh = (C.c_double * ns)(*SHIFTS)
    eps_mms, rel_mms = 1e-22, 0
    with tempfile.TemporaryFile() as cap:
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(cap.fileno(), 1)
        nd.tmnd_set_debug(3)
        it = nd.tmnd_cg_mms_tm_nd(up, dn, sp(0), sp(1), sh, ns, 1000, eps_mms, rel_mms, N)
        nd.tmnd_set_debug(0)
        C.CDLL(None).fflush(None)
        os.dup2(saved, 1)
        os.close(saved)
        cap.seek(0)
        log = cap.read().decode()
    drops = [[int(m.group(1)), int(m.group(2))] for m in re.finditer(r"at iteration (\d+) removed one shift, (\d+) remaining", log)]
    scal["cg_mms_tm_nd"] = {"shifts": SHIFTS, "eps_sq": eps_mms, "rel_prec": rel_mms, "max_iter": 1000, "iters": it, "drops": drops,
                            "sol_norms": [lib.square_norm(sp(18 + 2 * k), N, 0) + lib.square_norm(sp(19 + 2 * k), N, 0) for k in range(ns)]}
    if full:
        for k in range(ns):
            arrs["cg_mms_up_%d" % k] = r.spinor(18 + 2 * k, N).copy()
            arrs["cg_mms_dn_%d" % k] = r.spinor(19 + 2 * k, N).copy()
    tag = "%dx%d" % (T, L)
    json.dump(scal, open(os.path.join(GOLD, "ref_nd_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_nd_%s.npz" % tag), **arrs)
    shifts_out.append((tag, scal["cg_her_nd"]["iters"], scal["cg_mms_tm_nd"]["iters"], drops))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=2, metavar=("L", "SO"))
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        out = []
        L = int(a.child[0])
        gen(L, L, a.child[1], L == 4, out)
        print(out)
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_nd.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for L in (4, 8):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(L), so])
