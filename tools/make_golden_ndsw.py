"""TEST INFRASTRUCTURE ONLY: fixtures of the clover doublet (tests/golden/ref_ndsw_4x4.npz, ref_ndsw_scalars_{4x4,8x8}.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_ndsw.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

operator/tm_operators_nd.c, solver/cg_her_nd.c, solver/cg_mms_tm_nd.c, linalg/assign_mul_add_mul_r.c and linalg/assign_add_mul.c are
compiled here, in place from the reference tree, into a temporary directory (nothing is copied into this repository), linked with
tools/ndsw_harness.c against libtmref.so (which holds the clover functions), and run on the seed-123456 gauge field with c_sw != 0:
sw_term and sw_invert_nd, the three site-local functions, the six Qsw operators, sw_deriv_nd(EE), the statements of
ndrat_monomial.c:114-184, :235-254 and :299-309 for NDCLOVERRAT on given solution fields (np = 3, no solve inside), and
cg_her_nd / cg_mms_tm_nd on Qsw_pm_ndpsi for their iteration counts (4^4 and 8^4).

The gauge field and the four random spinors are those of tests/golden/ref_nd_4x4.npz (same seed, same calls -- asserted here), so
they are not stored again.  To stay within the size of the other fixtures every per-site output is stored on every second site
(SITES); the square norm over ALL sites of each goes to the scalars file.
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
SRCS = ["operator/tm_operators_nd.c", "solver/cg_her_nd.c", "solver/cg_mms_tm_nd.c", "linalg/assign_mul_add_mul_r.c", "linalg/assign_add_mul.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.6931      # those of ref_nd_* / ref_rat_*
KAPPA, C_SW = 0.125, 1.57
NFIELDS, DUM = 48, 40
SITES = slice(0, None, 2)
SHIFTS = [0.02, 0.15, 0.6, 2.5, 9.0]
MU, RMU = [0.031, 0.27, 1.9], [0.0042, 0.057, 0.81]
NU, RNU = [0.019, 0.16, 1.1], [0.0031, 0.044, 0.63]
EO, OE, EE, OO = 0, 1, 0, 1


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "ndsw_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmndsw.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def gen(T, L, so, full):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    r = RefLattice(T, L, L, L, kappa=KAPPA, mu=0.0, nfields=NFIELDS)
    nd = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    nd.tmndsw_set.argtypes = [d, d, d]
    nd.tmndsw_set_dum.argtypes = [i]
    nd.tmndsw_set_debug.argtypes = [i]
    for n in ("Qsw_ndpsi", "Qsw_dagger_ndpsi", "Qsw_pm_ndpsi", "H_eo_sw_ndpsi", "Msw_ee_inv_ndpsi"):
        getattr(nd, n).argtypes = [vp] * 4
    # _Complex double by value: SysV passes (re, im) as two consecutive doubles in SSE registers
    nd.Qsw_tau1_sub_const_ndpsi.argtypes = [vp] * 4 + [d, d, d, d]
    nd.assign_add_mul.argtypes = [vp, vp, d, d, i]
    nd.cg_her_nd.argtypes = [vp] * 4 + [i, d, i, i, vp]
    nd.tmndsw_cg_mms_tm_nd.argtypes = [C.POINTER(vp), C.POINTER(vp), vp, vp, C.POINTER(d), i, i, d, i, i]
    nd.tmndsw_set_dum(DUM)
    nd.tmndsw_set(MUBAR, EPSBAR, INVMAXEV)
    r.random_fields(123456)
    for k in (1, 2, 3):
        r.lib.tmref_random_spinor_eo(k)
    lib, N, sp = r.lib, r.V // 2, r.sp
    lib.sw_invert_nd.argtypes = [d]
    lib.assign_mul_one_sw_pm_imu_eps.argtypes = [i] + [vp] * 4 + [d, d]
    lib.clover_inv_nd.argtypes = [i, vp, vp]
    lib.clover_gamma5_nd.argtypes = [i] + [vp] * 6 + [d, d]
    lib.sw_deriv_nd.argtypes = [i]
    lib.sw_spinor_eo.argtypes = [i, vp, vp, d]
    lib.tmref_sw_all.argtypes = [d, d]
    mshift = MUBAR * MUBAR - EPSBAR * EPSBAR
    sw, swi = r.clover(C_SW, 0.0)                     # init_sw_fields, sw_term
    lib.sw_invert_nd(mshift)                          # overwrites sw_inv[icx < V/2]
    tag = "%dx%d" % (T, L)
    scal = {"T": T, "L": L, "kappa": KAPPA, "c_sw": C_SW, "seed": 123456, "mubar": MUBAR, "epsbar": EPSBAR, "invmaxev": INVMAXEV,
            "mshift": mshift, "mu": MU, "rmu": RMU, "nu": NU, "rnu": RNU, "np": len(MU), "norms": {}}
    arrs = {}
    nsq = lambda a, b: lib.square_norm(sp(a), N, 0) + lib.square_norm(sp(b), N, 0)

    def keep(name, a, b):
        scal["norms"][name] = nsq(a, b)
        if full:
            arrs[name + "_s"] = r.spinor(a, N)[SITES].copy()
            arrs[name + "_c"] = r.spinor(b, N)[SITES].copy()

    if full:
        base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
        assert np.array_equal(base["gauge"], r.gauge())
        for k, name in enumerate(("k_s", "k_c", "j_s", "j_c")):
            assert np.array_equal(base[name], r.spinor(k, N)), name
        arrs["sw_inv_nd"] = swi[:N][SITES].copy()
        scal["sw_norm"] = float((sw ** 2).sum())
        scal["sw_inv_nd_norm"] = float((swi[:N] ** 2).sum())
    KS, KC, JS, JC = 0, 1, 2, 3
    # ---- site-local: (k_s, k_c) = assign_mul_one_sw_pm_imu_eps(EE; l = (k_s, k_c)), clover_inv_nd on a copy of that, clover_gamma5_nd(OO)
    lib.assign_mul_one_sw_pm_imu_eps(EE, sp(4), sp(5), sp(KS), sp(KC), MUBAR, EPSBAR)
    keep("assign_mul_one_sw_pm_imu_eps", 4, 5)
    lib.clover_inv_nd(EE, sp(5), sp(4))
    keep("clover_inv_nd", 4, 5)
    lib.clover_gamma5_nd(OO, sp(7), sp(6), sp(KC), sp(KS), sp(JC), sp(JS), MUBAR, -EPSBAR)
    keep("clover_gamma5_nd", 6, 7)
    # ---- operators
    for n, (a, b) in (("Qsw_ndpsi", (8, 9)), ("Qsw_dagger_ndpsi", (10, 11)), ("Qsw_pm_ndpsi", (12, 13)), ("H_eo_sw_ndpsi", (14, 15)),
                      ("Msw_ee_inv_ndpsi", (16, 17))):
        getattr(nd, n)(sp(a), sp(b), sp(KS), sp(KC))
        keep(n, a, b)
    nd.Qsw_tau1_sub_const_ndpsi(sp(18), sp(19), sp(KS), sp(KC), 0.3, -0.7, 1.1, INVMAXEV)
    keep("Qsw_tau1_sub_const_ndpsi", 18, 19)
    scal["tau1_args"] = {"z": [0.3, -0.7], "Cpol": 1.1, "invev": INVMAXEV}
    if full:
        # ---- sw_deriv_nd(EE) on zeroed accumulators: the even sites only
        lex = r.eo2lexic()[:N]
        lib.tmref_swpm_zero()
        lib.sw_deriv_nd(EE)
        swm, swp = r.swpm()
        arrs["sw_deriv_nd_swm"] = swm[lex][SITES].copy()
        arrs["sw_deriv_nd_swp"] = swp[lex][SITES].copy()
        scal["sw_deriv_nd_norms"] = [float((swm ** 2).sum()), float((swp ** 2).sum())]
        # ---- the monomial on chi_0 = (k_s, k_c), chi_1 = (j_s, j_c), chi_2 = (j_c, k_s), eta = (k_c, j_s)
        CU, CD, ETA_U, ETA_D = [KS, JS, JC], [KC, JC, KS], KC, JS
        W, TMP_U, TMP_D, PF_U, PF_D = [20, 21, 22, 23, 24, 25], 26, 27, 28, 29
        scal["chi"] = [["k_s", "k_c"], ["j_s", "j_c"], ["j_c", "k_s"]]
        scal["eta"] = ["k_c", "j_s"]
        for trlog in (0, 1):                          # ndrat_monomial.c:80-86, :114-184 (forcefactor = EVMaxInv, :94)
            r.derivative()[:] = 0
            lib.tmref_swpm_zero()
            for j in range(len(MU) - 1, -1, -1):
                f = RMU[j] * INVMAXEV
                nd.Qsw_tau1_sub_const_ndpsi(sp(W[0]), sp(W[1]), sp(CU[j]), sp(CD[j]), 0.0, -MU[j], 1., INVMAXEV)
                nd.H_eo_sw_ndpsi(sp(W[2]), sp(W[3]), sp(CU[j]), sp(CD[j]))
                r.deriv_Sb(EO, W[2], W[0], f)
                r.deriv_Sb(EO, W[3], W[1], f)
                nd.H_eo_sw_ndpsi(sp(W[4]), sp(W[5]), sp(W[0]), sp(W[1]))
                r.deriv_Sb(OE, CU[j], W[4], f)
                r.deriv_Sb(OE, CD[j], W[5], f)
                lib.sw_spinor_eo(EE, sp(W[5]), sp(W[2]), f)
                lib.sw_spinor_eo(OO, sp(CU[j]), sp(W[1]), f)
                lib.sw_spinor_eo(EE, sp(W[4]), sp(W[3]), f)
                lib.sw_spinor_eo(OO, sp(CD[j]), sp(W[0]), f)
            if trlog:
                lib.sw_deriv_nd(EE)
            lib.tmref_sw_all(KAPPA, C_SW)
            arrs["ndcloverrat_derivative_trlog%d" % trlog] = r.derivative().copy()
        # heatbath, :212-217 and :235-254
        lib.assign(sp(PF_U), sp(ETA_U), N)
        lib.assign(sp(PF_D), sp(ETA_D), N)
        scal["ndcloverrat_energy0"] = lib.square_norm(sp(PF_U), N, 1) + lib.square_norm(sp(PF_D), N, 1)
        for j in range(len(NU) - 1, -1, -1):
            nd.Qsw_tau1_sub_const_ndpsi(sp(TMP_U), sp(TMP_D), sp(CU[j]), sp(CD[j]), 0.0, NU[j], 1., INVMAXEV)
            nd.assign_add_mul(sp(PF_U), sp(TMP_U), 0.0, RNU[j], N)
            nd.assign_add_mul(sp(PF_D), sp(TMP_D), 0.0, RNU[j], N)
        keep("ndcloverrat_pf", PF_U, PF_D)
        # acceptance, :299-309, on pf = eta
        lib.assign(sp(W[0]), sp(ETA_U), N)
        lib.assign(sp(W[1]), sp(ETA_D), N)
        for j in range(len(MU) - 1, -1, -1):
            lib.assign_add_mul_r(sp(W[0]), sp(CU[j]), RMU[j], N)
            lib.assign_add_mul_r(sp(W[1]), sp(CD[j]), RMU[j], N)
        scal["ndcloverrat_energy1"] = lib.scalar_prod_r(sp(ETA_U), sp(W[0]), N, 1) + lib.scalar_prod_r(sp(ETA_D), sp(W[1]), N, 1)
    # ---- solvers on Qsw_pm_ndpsi: iteration counts
    eps_sq, rel = 1e-20, 1
    r.spinor(30)[:] = 0
    r.spinor(31)[:] = 0
    it = nd.cg_her_nd(sp(30), sp(31), sp(KS), sp(KC), 1000, eps_sq, rel, N, C.cast(nd.Qsw_pm_ndpsi, vp))
    scal["cg_her_nd"] = {"eps_sq": eps_sq, "rel_prec": rel, "max_iter": 1000, "iters": it, "sol_norm": nsq(30, 31)}
    ns = len(SHIFTS)
    up = (vp * ns)(*[sp(20 + 2 * k) for k in range(ns)])
    dn = (vp * ns)(*[sp(21 + 2 * k) for k in range(ns)])
    sh = (C.c_double * ns)(*SHIFTS)
    eps_mms, rel_mms = 1e-22, 0
    with tempfile.TemporaryFile() as cap:
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(cap.fileno(), 1)
        nd.tmndsw_set_debug(3)
        it = nd.tmndsw_cg_mms_tm_nd(up, dn, sp(KS), sp(KC), sh, ns, 1000, eps_mms, rel_mms, N)
        nd.tmndsw_set_debug(0)
        C.CDLL(None).fflush(None)
        os.dup2(saved, 1)
        os.close(saved)
        cap.seek(0)
        log = cap.read().decode()
    drops = [[int(m.group(1)), int(m.group(2))] for m in re.finditer(r"at iteration (\d+) removed one shift, (\d+) remaining", log)]
    scal["cg_mms_tm_nd"] = {"shifts": SHIFTS, "eps_sq": eps_mms, "rel_prec": rel_mms, "max_iter": 1000, "iters": it, "drops": drops,
                            "sol_norms": [nsq(20 + 2 * k, 21 + 2 * k) for k in range(ns)]}
    json.dump(scal, open(os.path.join(GOLD, "ref_ndsw_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_ndsw_%s.npz" % tag), **arrs)
    print(tag, "cg_her_nd", scal["cg_her_nd"]["iters"], "cg_mms_tm_nd", it, drops)


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
        sys.exit("make_golden_ndsw.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for L in (4, 8):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(L), so])
