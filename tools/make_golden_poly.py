"""TEST INFRASTRUCTURE ONLY: fixtures of the polynomial monomial NDPOLY (tests/golden/ref_poly_4x4.npz, ref_poly_scalars_4x4.json,
ref_poly_scalars_6x4.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_poly.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

monomial/ndpoly_monomial.c, Ptilde_nd.c, chebyshev_polynomial_nd.c, linalg/assign_mul_add_mul_add_mul_add_mul_r.c,
operator/tm_operators_nd.c and init/init_chi_spinor_field.c are compiled here, in place from the reference tree, into a temporary
directory (nothing is copied into this repository) and linked with tools/poly_harness.c against libtmref.so.  The monomial is the
NDPOLY block of sample-input/sample-hmc2.input (StildeMin / StildeMax, 2Kappamubar / 2Kappaepsbar, PrecisionPtilde,
DegreeOfMDPolynomial 48 -> MDPolyDegree n = 49), its roots are sample-input/Square_root_BR_roots.dat and its constant the number in
sample-input/normierungLocal.dat: the reference's init_ndpoly_monomial reads them, and what it made of them -- MDPolyCoefs, PtildeCoefs,
PtildeDegree, the 96 roots -- goes into the fixture as numbers.  Then the reference's own ndpoly_derivative, ndpoly_heatbath and
ndpoly_acc run.  ndpoly_acc keeps its Ener[j] to itself, so its statements :287-366 are replayed here call by call on the reference's
functions, and the replay must reproduce the energy1 of the function bit for bit.

4^4: the seed-123456 RANLUX gauge field of the other fixtures; 6 x 4^3: tests.util.random_gauge(66, V), scalars only.
Every quantity also carries the deviation of tests/poly_restate.py from it (`restate_vs_ref`): the GPU tests take 8 x that as their bound.
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRCS = ["monomial/ndpoly_monomial.c", "Ptilde_nd.c", "chebyshev_polynomial_nd.c", "linalg/assign_mul_add_mul_add_mul_add_mul_r.c",
        "operator/tm_operators_nd.c", "init/init_chi_spinor_field.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
# BeginMonomial NDPOLY of sample-input/sample-hmc2.input
STILDE_MIN, STILDE_MAX, PRECISION_PTILDE, DEGREE, PRECISION_HFINAL = 0.013577, 3.096935, 1e-05, 48, 1e-10
MUBAR, EPSBAR = 0.1105, 0.0935
KAPPA = 0.125
NFIELDS, DUM = 40, 32
SEED_6x4, SEED_HB = 66, 4711
PF_U, PF_D, W0, W1, ETA_U, ETA_D, S_U, S_D, R_U, R_D, CHI0 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
EO, OE = 0, 1


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "poly_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmpoly.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def bind(so):
    nd = C.CDLL(so)
    vp, d, i, pd = C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_double)
    nd.tmpoly_set_dum.argtypes = [i]
    nd.tmpoly_init.argtypes = [d] * 7 + [i, d, C.c_char_p] + [vp] * 4 + [i]
    nd.tmpoly_set_precision_hfinal.argtypes = [d]
    for n in ("tmpoly_md_coefs", "tmpoly_ptilde_coefs", "tmpoly_roots", "tmpoly_derivative"):
        getattr(nd, n).restype = pd
    for n in ("tmpoly_evmin", "tmpoly_evmaxinv", "tmpoly_energy0", "tmpoly_energy1", "tmpoly_forcefactor", "tmpoly_call_acc"):
        getattr(nd, n).restype = d
    nd.tmpoly_call_heatbath.argtypes = [i, vp, vp]
    # _Complex double by value: SysV passes (re, im) as two consecutive doubles in SSE registers
    nd.Q_tau1_sub_const_ndpsi.argtypes = [vp] * 4 + [d, d, d, d]
    nd.Qtm_ndpsi.argtypes = [vp] * 4
    nd.Qtm_dagger_ndpsi.argtypes = [vp] * 4
    nd.Ptilde_ndpsi.argtypes = [vp, vp, pd, i, vp, vp, vp]
    return nd


def gen(T, L, so, ref, full):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.oraclebind import Oracle
    from oracle.nd_restate import cplx, real
    from oracle.refbind import RefLattice
    from tests.poly_restate import Poly
    from tests.util import random_gauge, random_spinor
    r = RefLattice(T, L, L, L, kappa=KAPPA, mu=0.0, nfields=NFIELDS)
    nd = bind(so)
    nd.tmpoly_set_dum(DUM)
    lib, V, N, sp = r.lib, r.V, r.V // 2, r.sp
    if full:
        r.random_fields(123456)
        stored = np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"]
        assert np.array_equal(stored[:V], r.gauge()), "the RANLUX field is not the one of ref_fields_4x4.npz"
        gauge_note = "gauge of ref_fields_4x4.npz (RANLUX, seed 123456)"
    else:
        r.gauge()[:] = random_gauge(SEED_6x4, V)
        r.mark_gauge_dirty()
        gauge_note = "tests.util.random_gauge(%d, V)" % SEED_6x4
    locnorm = float(open(os.path.join(ref, "sample-input", "normierungLocal.dat")).read().split()[0])
    roots_file = os.path.join(ref, "sample-input", "Square_root_BR_roots.dat").encode()
    rc = nd.tmpoly_init(KAPPA, MUBAR, EPSBAR, STILDE_MIN, STILDE_MAX, locnorm, PRECISION_PTILDE, DEGREE, PRECISION_HFINAL, roots_file,
                        sp(PF_U), sp(PF_D), sp(W0), sp(W1), 0)
    assert rc == 0
    n, npt = nd.tmpoly_md_degree(), nd.tmpoly_ptilde_degree()
    md = [nd.tmpoly_md_coefs()[k] for k in range(n)]
    pt = [nd.tmpoly_ptilde_coefs()[k] for k in range(npt)]
    rt = [nd.tmpoly_roots()[k] for k in range(2 * (2 * n - 2))]
    roots = [complex(rt[2 * k], rt[2 * k + 1]) for k in range(2 * n - 2)]
    evmin, invmaxev, Cpol = nd.tmpoly_evmin(), nd.tmpoly_evmaxinv(), math.sqrt(locnorm)
    scal = {"T": T, "L": L, "kappa": KAPPA, "gauge": gauge_note, "mubar": MUBAR, "epsbar": EPSBAR, "StildeMin": STILDE_MIN, "StildeMax": STILDE_MAX,
            "LocNormConst": locnorm, "PrecisionPtilde": PRECISION_PTILDE, "PrecisionHfinal": PRECISION_HFINAL, "MDPolyDegree": n,
            "PtildeDegree": npt, "MDPolyCoefs": md, "PtildeCoefs": pt, "MDPolyRoots": [[z.real, z.imag] for z in roots],
            "evmin": evmin, "evmax": 1.0, "invmaxev": invmaxev, "Cpol": Cpol,
            "fields": "S = tests.util.random_spinor(31 / 32, V/2), phi = random_spinor(33 / 34, V/2); eta: RANLUX seed %d" % SEED_HB}
    arrs = {}
    qsq = C.cast(nd.Qtm_pm_ndpsi, C.c_void_p)
    pdbl = lambda x: (C.c_double * len(x))(*x)

    def put(i, a):
        r.spinor(i, N)[:] = a

    # ---- one Ptilde_ndpsi
    S = random_spinor(31, N), random_spinor(32, N)
    put(S_U, S[0]); put(S_D, S[1])
    nd.Ptilde_ndpsi(sp(R_U), sp(R_D), pdbl(pt), npt, sp(S_U), sp(S_D), qsq)
    pt_out = r.spinor(R_U, N).copy(), r.spinor(R_D, N).copy()
    # ---- the force on phi
    phi = random_spinor(33, N), random_spinor(34, N)
    put(PF_U, phi[0]); put(PF_D, phi[1])
    df = np.frombuffer((C.c_double * (V * 32)).from_address(C.addressof(nd.tmpoly_derivative().contents)), dtype=np.float64).reshape(V, 4, 8)
    df[:] = 0
    nd.tmpoly_call_derivative()
    force = df.copy()
    assert nd.tmpoly_forcefactor() == -Cpol * invmaxev
    # ---- the heatbath
    nd.tmpoly_call_heatbath(SEED_HB, sp(ETA_U), sp(ETA_D))
    eta = r.spinor(ETA_U, N).copy(), r.spinor(ETA_D, N).copy()
    pf = r.spinor(PF_U, N).copy(), r.spinor(PF_D, N).copy()
    scal["energy0"] = nd.tmpoly_energy0()
    assert scal["energy0"] == lib.square_norm(sp(ETA_U), N, 1) + lib.square_norm(sp(ETA_D), N, 1), "eta is not the field the heatbath drew"
    # ---- the acceptance step on that pf and on phi, with the sample's PrecisionHfinal and with 0 (all seven corrections)
    chi = [(CHI0 + 2 * j, CHI0 + 2 * j + 1) for j in range(8)]
    nsq = lambda c: lib.square_norm(sp(c[0]), N, 1) + lib.square_norm(sp(c[1]), N, 1)
    P = lambda dst, coefs, src: nd.Ptilde_ndpsi(sp(dst[0]), sp(dst[1]), pdbl(coefs), len(coefs), sp(src[0]), sp(src[1]), qsq)

    def acc(field, e0):
        """-> (energy1, energy1 with PrecisionHfinal 0, Ener[0 .. 7], corrections)"""
        put(PF_U, field[0]); put(PF_D, field[1])
        dH = nd.tmpoly_call_acc()
        e1 = nd.tmpoly_energy1()
        assert e0 is None or dH == e1 - e0
        nd.tmpoly_set_precision_hfinal(0.0)
        nd.tmpoly_call_acc()
        e1_all = nd.tmpoly_energy1()
        nd.tmpoly_set_precision_hfinal(PRECISION_HFINAL)
        assert np.array_equal(r.spinor(PF_U, N), field[0]) and np.array_equal(r.spinor(PF_D, N), field[1])
        # the replay of :287-366 for Ener[0 .. 7]
        a, b = chi[0], chi[1]
        lib.assign(sp(a[0]), sp(PF_U), N); lib.assign(sp(a[1]), sp(PF_D), N)
        for j in range(1, n):
            nd.Q_tau1_sub_const_ndpsi(sp(b[0]), sp(b[1]), sp(a[0]), sp(a[1]), roots[j - 1].real, roots[j - 1].imag, Cpol, invmaxev)
            a, b = b, a
        if a != chi[0]:
            lib.assign(sp(chi[0][0]), sp(a[0]), N); lib.assign(sp(chi[0][1]), sp(a[1]), N)
        Ener, factor, diffs = [0.0] * 8, [1.0] * 8, [0.0] * 8
        for j in range(1, 8):
            factor[j] = j * factor[j - 1]
        Ener[0] = nsq(chi[0])
        for j in range(1, 8):
            if j % 2:
                P(chi[j], pt, chi[j - 1]); P(chi[j - 1], md, chi[j])
                nd.Qtm_dagger_ndpsi(sp(chi[j][0]), sp(chi[j][1]), sp(chi[j - 1][0]), sp(chi[j - 1][1]))
            else:
                nd.Qtm_ndpsi(sp(chi[j][0]), sp(chi[j][1]), sp(chi[j - 1][0]), sp(chi[j - 1][1]))
                P(chi[j - 1], md, chi[j]); P(chi[j], pt, chi[j - 1])
            Ener[j] = Ener[j - 1] + Ener[0]
            sgn = -1.0
            for ij in range(1, j):
                Ener[j] += sgn * (factor[j] / (factor[ij] * factor[j - ij])) * Ener[ij]
                sgn = -sgn
            Ener[j] += sgn * nsq(chi[j])
            diffs[j] = abs(Ener[j] - Ener[j - 1])
        corrections = next((j for j in range(1, 8) if diffs[j] < PRECISION_HFINAL), 7)
        assert Ener[corrections] == e1 and Ener[7] == e1_all, ("the replay of ndpoly_acc is not the function", Ener, e1, e1_all)
        return e1, e1_all, Ener, corrections

    scal["energy1"], scal["energy1_all_seven"], Ener, corrections = acc(pf, scal["energy0"])
    scal["Ener"], scal["corrections"] = Ener, corrections
    # ... and on phi, the field a lattice without stored fields can rebuild
    scal["phi_energy1"], _, Ener_phi, scal["phi_corrections"] = acc(phi, None)
    scal["phi_Ener"] = Ener_phi

    # ---- the restatement against all of it
    orc = Oracle(T, L, L, L, kappa=KAPPA, mu=0.0)
    g = np.zeros((orc.VPR, 4, 3, 3, 2))
    g[:V] = r.gauge()
    orc.set_gauge(g)
    po = Poly(orc, MUBAR, EPSBAR, invmaxev)
    rel = lambda x, y: float(np.abs(x - y).max() / np.abs(y).max())
    q = po.Ptilde(pt, cplx(S[0]), cplx(S[1]), evmin, 1.0)
    dev = {"ptilde": max(rel(real(q[0]), pt_out[0]), rel(real(q[1]), pt_out[1]))}
    dfr = po.derivative(cplx(phi[0]), cplx(phi[1]), roots, Cpol, np.zeros((orc.VPR, 4, 8)))
    dev["force"] = rel(dfr[:V], force)
    e0, hu, hd = po.heatbath(cplx(eta[0]), cplx(eta[1]), roots, Cpol, pt, evmin, 1.0)
    dev["pf"] = max(rel(real(hu), pf[0]), rel(real(hd), pf[1]))
    dev["energy0"] = abs(e0 - scal["energy0"]) / abs(scal["energy0"])
    e1, steps, en = po.acc(cplx(pf[0]), cplx(pf[1]), roots, Cpol, md, pt, evmin, 1.0, 0.0)
    dev["Ener"] = [abs(x - y) / abs(y) for x, y in zip(en, Ener)]
    e1, steps, en = po.acc(cplx(phi[0]), cplx(phi[1]), roots, Cpol, md, pt, evmin, 1.0, 0.0)
    dev["phi_Ener"] = [abs(x - y) / abs(y) for x, y in zip(en, Ener_phi)]
    scal["restate_vs_ref"] = dev
    # scalars of the fields, for the lattice whose fields are not stored
    scal["ptilde_sqnorm"] = float((pt_out[0] ** 2).sum() + (pt_out[1] ** 2).sum())
    scal["force_sqnorm"] = float((force ** 2).sum())
    scal["force_absmax"] = float(np.abs(force).max())
    scal["pf_sqnorm"] = float((pf[0] ** 2).sum() + (pf[1] ** 2).sum())
    print("%dx%d" % (T, L), "n", n, "PtildeDegree", npt, "energy0", scal["energy0"], "Ener", Ener, "corrections", corrections, file=sys.stderr)
    print("   restatement vs reference:", dev, file=sys.stderr)
    tag = "%dx%d" % (T, L)
    json.dump(scal, open(os.path.join(GOLD, "ref_poly_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        arrs.update(S_up=S[0], S_dn=S[1], ptilde_up=pt_out[0], ptilde_dn=pt_out[1], phi_up=phi[0], phi_dn=phi[1], force=force,
                    eta_up=eta[0], eta_dn=eta[1], pf_up=pf[0], pf_dn=pf[1])
        np.savez_compressed(os.path.join(GOLD, "ref_poly_%s.npz" % tag), **arrs)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=3, metavar=("T", "L", "SO"))
    a = ap.parse_args()
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_poly.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        T, L = int(a.child[0]), int(a.child[1])
        gen(T, L, a.child[2], a.ref, T == 4)
        sys.exit(0)
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for T, L in ((4, 4), (6, 4)):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--ref", a.ref, "--child", str(T), str(L), so])
