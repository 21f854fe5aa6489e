"""TEST INFRASTRUCTURE ONLY: fixtures of the rational monomials (tests/golden/ref_rat_4x4.npz, ref_rat_scalars_4x4.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_rat.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

operator/tm_operators_nd.c and linalg/assign_add_mul.c are compiled here, in place from the reference tree, into a temporary
directory (nothing is copied into this repository), linked with tools/rat_harness.c against libtmref.so, and the statements of
ndrat_monomial.c:114-160, :235-254, :299-309 and rat_monomial.c:95-132, :191-199, :244-250 (type NDRAT / RAT) are run on the
seed-123456 4^4 gauge field: the reference's own functions, called in the reference's order, on random solution fields chi_j
(np = 3) and a random eta -- no solve inside.  rat runs at g_mu = 0 as the monomial sets it.
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
SRCS = ["operator/tm_operators_nd.c", "linalg/assign_add_mul.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.6931
NFIELDS, DUM = 40, 32
# a three-term partial fraction: any real numbers exercise the statements (the coefficients of a run come from init_rational)
MU, RMU = [0.031, 0.27, 1.9], [0.0042, 0.057, 0.81]
NU, RNU = [0.019, 0.16, 1.1], [0.0031, 0.044, 0.63]
EO, OE = 0, 1


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "rat_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmrat.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def gen(so):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    T = L = 4
    kappa = 0.125
    r = RefLattice(T, L, L, L, kappa=kappa, mu=0.0, nfields=NFIELDS)
    nd = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    nd.tmrat_set.argtypes = [d, d, d]
    nd.tmrat_set_dum.argtypes = [i]
    # _Complex double by value: SysV passes (re, im) as two consecutive doubles in SSE registers
    nd.Q_tau1_sub_const_ndpsi.argtypes = [vp] * 4 + [d, d, d, d]
    nd.H_eo_tm_ndpsi.argtypes = [vp] * 4 + [i]
    nd.assign_add_mul.argtypes = [vp, vp, d, d, i]
    nd.tmrat_set_dum(DUM)
    nd.tmrat_set(MUBAR, EPSBAR, INVMAXEV)
    r.random_fields(123456)
    for k in range(8):
        r.lib.tmref_random_spinor_eo(k)
    lib, N, sp = r.lib, r.V // 2, r.sp
    np_ = len(MU)
    CU, CD, ETA_U, ETA_D, W, TMP_U, TMP_D, PF_U, PF_D = [0, 1, 2], [3, 4, 5], 6, 7, [8, 9, 10, 11, 12, 13], 14, 15, 16, 17
    scal = {"T": T, "L": L, "kappa": kappa, "seed": 123456, "mubar": MUBAR, "epsbar": EPSBAR, "invmaxev": INVMAXEV,
            "mu": MU, "rmu": RMU, "nu": NU, "rnu": RNU, "np": np_}
    arrs = {"gauge": r.gauge().copy(), "eta_up": r.spinor(ETA_U, N).copy(), "eta_dn": r.spinor(ETA_D, N).copy()}
    for j in range(np_):
        arrs["chi_up_%d" % j] = r.spinor(CU[j], N).copy()
        arrs["chi_dn_%d" % j] = r.spinor(CD[j], N).copy()

    # ---- ndrat: the force loop, ndrat_monomial.c:114-160 (forcefactor = EVMaxInv, :94)
    r.derivative()[:] = 0
    for j in range(np_ - 1, -1, -1):
        nd.Q_tau1_sub_const_ndpsi(sp(W[0]), sp(W[1]), sp(CU[j]), sp(CD[j]), 0.0, -MU[j], 1., INVMAXEV)
        if j == 0:
            arrs["Q_tau1_s"] = r.spinor(W[0], N).copy()
            arrs["Q_tau1_c"] = r.spinor(W[1], N).copy()
        nd.H_eo_tm_ndpsi(sp(W[2]), sp(W[3]), sp(CU[j]), sp(CD[j]), EO)
        r.deriv_Sb(EO, W[2], W[0], RMU[j] * INVMAXEV)
        r.deriv_Sb(EO, W[3], W[1], RMU[j] * INVMAXEV)
        nd.H_eo_tm_ndpsi(sp(W[4]), sp(W[5]), sp(W[0]), sp(W[1]), EO)
        r.deriv_Sb(OE, CU[j], W[4], RMU[j] * INVMAXEV)
        r.deriv_Sb(OE, CD[j], W[5], RMU[j] * INVMAXEV)
    arrs["ndrat_derivative"] = r.derivative().copy()
    # heatbath, :212-217 and :235-254
    lib.assign(sp(PF_U), sp(ETA_U), N)
    lib.assign(sp(PF_D), sp(ETA_D), N)
    scal["ndrat_energy0"] = lib.square_norm(sp(PF_U), N, 1) + lib.square_norm(sp(PF_D), N, 1)
    for j in range(np_ - 1, -1, -1):
        nd.Q_tau1_sub_const_ndpsi(sp(TMP_U), sp(TMP_D), sp(CU[j]), sp(CD[j]), 0.0, NU[j], 1., INVMAXEV)
        nd.assign_add_mul(sp(PF_U), sp(TMP_U), 0.0, RNU[j], N)
        nd.assign_add_mul(sp(PF_D), sp(TMP_D), 0.0, RNU[j], N)
    arrs["ndrat_pf_up"] = r.spinor(PF_U, N).copy()
    arrs["ndrat_pf_dn"] = r.spinor(PF_D, N).copy()
    # acceptance, :299-309, on pf = eta
    lib.assign(sp(W[0]), sp(ETA_U), N)
    lib.assign(sp(W[1]), sp(ETA_D), N)
    for j in range(np_ - 1, -1, -1):
        lib.assign_add_mul_r(sp(W[0]), sp(CU[j]), RMU[j], N)
        lib.assign_add_mul_r(sp(W[1]), sp(CD[j]), RMU[j], N)
    scal["ndrat_energy1"] = lib.scalar_prod_r(sp(ETA_U), sp(W[0]), N, 1) + lib.scalar_prod_r(sp(ETA_D), sp(W[1]), N, 1)

    # ---- rat (type RAT: Qp = Qtm_plus_psi at g_mu = 0): rat_monomial.c:95-132 (forcefactor = 1, :81)
    r.set_kappa_mu(kappa, 0.0)
    r.derivative()[:] = 0
    for j in range(np_ - 1, -1, -1):
        lib.Qtm_plus_psi(sp(W[0]), sp(CU[j]))
        lib.H_eo_tm_inv_psi(sp(W[2]), sp(CU[j]), EO, -1.)
        r.deriv_Sb(OE, W[0], W[2], RMU[j])
        lib.H_eo_tm_inv_psi(sp(W[3]), sp(W[0]), EO, +1.)
        r.deriv_Sb(EO, W[3], CU[j], RMU[j])
    arrs["rat_derivative"] = r.derivative().copy()
    # heatbath, :175-177 and :191-199
    lib.assign(sp(PF_U), sp(ETA_U), N)
    scal["rat_energy0"] = lib.square_norm(sp(PF_U), N, 1)
    for j in range(np_ - 1, -1, -1):
        lib.Qtm_plus_psi(sp(TMP_U), sp(CU[j]))
        nd.assign_add_mul(sp(TMP_U), sp(CU[j]), 0.0, -NU[j], N)
        nd.assign_add_mul(sp(PF_U), sp(TMP_U), 0.0, RNU[j], N)
    arrs["rat_pf"] = r.spinor(PF_U, N).copy()
    # acceptance, :244-250
    lib.assign(sp(W[0]), sp(ETA_U), N)
    for j in range(np_ - 1, -1, -1):
        lib.assign_add_mul_r(sp(W[0]), sp(CU[j]), RMU[j], N)
    scal["rat_energy1"] = lib.scalar_prod_r(sp(ETA_U), sp(W[0]), N, 1)

    json.dump(scal, open(os.path.join(GOLD, "ref_rat_scalars_4x4.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(GOLD, "ref_rat_4x4.npz"), **arrs)
    print({k: v for k, v in scal.items() if "energy" in k})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", metavar="SO")
    a = ap.parse_args()
    if a.child:   # own process: the reference keeps its state in C globals
        gen(a.child)
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_rat.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", so])
