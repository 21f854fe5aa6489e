"""TEST INFRASTRUCTURE ONLY: fixtures of the correction monomials RATCOR / CLOVERRATCOR / NDRATCOR / NDCLOVERRATCOR
(tests/golden/ref_ratcor_4x4.npz, ref_ratcor_scalars_{4x4,8x8}.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_ratcor.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

solver/cg_mms_tm.c, solver/cg_mms_tm_nd.c, operator/tm_operators_nd.c, linalg/assign_mul_add_mul_r.c and linalg/assign_add_mul.c are
compiled here, in place from the reference tree, into a temporary directory (nothing is copied into this repository), linked with
tools/ratcor_harness.c against libtmref.so, and the reference's own functions are run in the order of apply_Z_psi / apply_Z_ndpsi and of
the four series loops (monomial/ratcor_monomial.c, monomial/ndratcor_monomial.c), for the four types
    ratcor (Qtm_pm_psi at mu = 0), cloverratcor (Qsw_pm_psi after sw_term + sw_invert(EE, 0.)),
    ndratcor (Qtm_pm_ndpsi), ndcloverratcor (Qsw_pm_ndpsi after sw_term + sw_invert_nd(mubar^2 - epsbar^2)).

Two coefficient sets per type:
  "arb"  arbitrary (mu, rmu, A), np = 3: one application of Z.
  "fit"  a real approximation, so that the series converge: the spectral interval [lo, hi] of the type's operator on the 4^4 field by a
         dense eigvalsh of its matrix (built column by column from the reference's operator), then A (1 + sum_j r_j / (x + mu_j^2)) ~
         x^(-1/2) by linear least squares in the relative error on np = 8 geometrically spaced poles.  mu, rmu, A, the interval and
         the fit error go to the scalars file.  One application of Z on eta, the heatbath on eta, the acceptance step on its result.
         The generator REFUSES to write anything unless heatbath and acceptance each break after 2 .. 5 applications of Z.

4^4: the seed-123456 gauge field and random spinors of tests/golden/ref_nd_4x4.npz (asserted here, not stored again); eta = (k_s, k_c).
8^4: scalars only, on tests.util.random_gauge / random_spinor with the seeds recorded and the "fit" coefficients of 4^4 (the interval of
the 8^4 field is not computed: its matrix is too large; the generator's 2 .. 5 check holds there too).
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
SRCS = ["operator/tm_operators_nd.c", "solver/cg_mms_tm.c", "solver/cg_mms_tm_nd.c", "linalg/assign_mul_add_mul_r.c", "linalg/assign_add_mul.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.6931      # those of ref_nd_* / ref_rat_*
KAPPA, C_SW = 0.125, 1.57                             # those of ref_ndsw_* / ref_cloverrat_*
NFIELDS, DUM = 48, 40
ARB = {"mu": [0.31, 0.9, 2.1], "rmu": [0.12, -0.07, 0.3], "A": 0.8, "max_iter": 2000, "accprec": 1e-22, "rel_prec": 0}
FIT_NP, FIT_ACCPREC, FIT_REL, FIT_MAXITER = 8, 1e-20, 1, 5000
SEED8 = (8131, 8132, 8133)                            # 8^4: random_gauge / random_spinor seeds (gauge, eta_up, eta_dn)
TYPES = [("ratcor", 0, 0), ("ndratcor", 1, 0), ("cloverratcor", 0, 1), ("ndcloverratcor", 1, 1)]   # (name, nd, sw), in the order they are run
CHI_UP, CHI_DN, W, PF, PF2, ZU, ZD, E0, E1, E2, E3 = 4, 13, 22, 28, 29, 30, 31, 32, 33, 34, 35


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "ratcor_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmratcor.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def fit_inverse_sqrt(lo, hi, npoles):
    """A, r_j, mu_j with A (1 + sum_j r_j / (x + mu_j^2)) ~ x^(-1/2) on [lo, hi]: least squares in the relative error on a logarithmic
    grid, poles mu_j^2 spaced geometrically from lo / 4 to 4 hi.  Returns (mu, rmu, A, largest relative error on a finer grid)."""
    import numpy as np
    m2 = np.geomspace(lo / 4.0, 4.0 * hi, npoles)

    def design(x):
        return np.concatenate([np.sqrt(x)[:, None], np.sqrt(x)[:, None] / (x[:, None] + m2[None, :])], axis=1)
    x = np.geomspace(lo, hi, 4000)
    c = np.linalg.lstsq(design(x), np.ones_like(x), rcond=None)[0]
    xf = np.geomspace(lo, hi, 40001)
    err = float(np.abs(design(xf) @ c - 1.0).max())
    return [float(v) for v in np.sqrt(m2)], [float(v) for v in c[1:] / c[0]], float(c[0]), err


def gen(T, L, so, full, fits):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    from tests.util import random_gauge, random_spinor
    r = RefLattice(T, L, L, L, kappa=KAPPA, mu=0.0, nfields=NFIELDS)
    h = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    pd, pi = C.POINTER(d), C.POINTER(i)
    h.tmrc_set_nd.argtypes = [d, d, d]
    h.tmrc_set_mu.argtypes = [d, d]
    h.tmrc_set_dum.argtypes = [i]
    h.tmrc_monomial.argtypes = [i, i, C.POINTER(vp), C.POINTER(vp), pd, pd, d, i, i, d, i, i]
    h.tmrc_apply_Z.restype = d; h.tmrc_apply_Z.argtypes = [vp] * 4
    h.tmrc_heatbath.restype = d; h.tmrc_heatbath.argtypes = [vp, vp, C.POINTER(vp), d, pd, pi]
    h.tmrc_acc.restype = d; h.tmrc_acc.argtypes = [vp, vp, C.POINTER(vp), d, pd, pi]
    for n in ("Qtm_pm_ndpsi", "Qsw_pm_ndpsi"):
        getattr(h, n).argtypes = [vp] * 4
    lib, N, sp = r.lib, r.V // 2, r.sp
    lib.sw_invert_nd.argtypes = [d]
    lib.sw_invert.argtypes = [i, d]
    h.tmrc_set_dum(DUM)
    h.tmrc_set_nd(MUBAR, EPSBAR, INVMAXEV)
    h.tmrc_set_mu(0.0, 0.0)                                                  # ratcor_monomial.c:67-68, ndratcor_monomial.c:73
    tag = "%dx%d" % (T, L)
    scal = {"T": T, "L": L, "kappa": KAPPA, "c_sw": C_SW, "mubar": MUBAR, "epsbar": EPSBAR, "invmaxev": INVMAXEV, "types": {}}
    arrs = {}
    if full:
        r.random_fields(123456)
        for k in (1, 2, 3):
            lib.tmref_random_spinor_eo(k)
        base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
        assert np.array_equal(base["gauge"], r.gauge())
        for k, name in enumerate(("k_s", "k_c", "j_s", "j_c")):
            assert np.array_equal(base[name], r.spinor(k, N)), name
        scal["seed"], scal["eta"] = 123456, ["k_s", "k_c"]
    else:
        r.gauge()[:] = random_gauge(SEED8[0], r.V)
        r.mark_gauge_dirty()
        r.spinor(0, N)[:] = random_spinor(SEED8[1], N)
        r.spinor(1, N)[:] = random_spinor(SEED8[2], N)
        scal["gauge_seed"], scal["eta_seeds"] = SEED8[0], list(SEED8[1:])
    chi_up = (vp * (FIT_NP + 1))(*[sp(CHI_UP + k) for k in range(FIT_NP + 1)])
    chi_dn = (vp * (FIT_NP + 1))(*[sp(CHI_DN + k) for k in range(FIT_NP + 1)])
    w = (vp * 6)(*[sp(W + k) for k in range(6)])

    def cvec(idx):
        return r.spinor(idx, N).reshape(N * 12, 2)

    def interval(nd, sw):
        """smallest and largest eigenvalue of the type's operator: its matrix column by column, then eigvalsh"""
        n = N * 12 * (2 if nd else 1)
        M = np.empty((n, n), dtype=np.complex128)
        for col in range(n):
            for f in (E0, E1):
                r.spinor(f, N)[:] = 0.0
            cvec(E0 if col < N * 12 else E1)[col % (N * 12), 0] = 1.0
            if nd:
                (h.Qsw_pm_ndpsi if sw else h.Qtm_pm_ndpsi)(sp(E2), sp(E3), sp(E0), sp(E1))
                out = np.concatenate([cvec(E2), cvec(E3)])
            else:
                (lib.Qsw_pm_psi if sw else lib.Qtm_pm_psi)(sp(E2), sp(E0))
                out = cvec(E2)
            M[:, col] = out[:, 0] + 1j * out[:, 1]
        herm = float(np.abs(M - M.conj().T).max())
        ev = np.linalg.eigvalsh(0.5 * (M + M.conj().T))
        return float(ev[0]), float(ev[-1]), herm

    def monomial(nd, sw, c, np_):
        mu, rmu = (d * np_)(*c["mu"]), (d * np_)(*c["rmu"])
        h.tmrc_monomial(nd, sw, chi_up, chi_dn, mu, rmu, c["A"], np_, c["max_iter"], c["accprec"], c["rel_prec"], N)
        return mu, rmu                                                       # kept alive by the caller

    clover_made = False
    for name, nd, sw in TYPES:
        if sw and not clover_made:
            lib.Qsw_pm_psi.argtypes = [vp, vp]
            r.clover(C_SW, 0.0)                                              # init_sw_fields, sw_term, sw_invert(EE, 0.)
            clover_made = True
        if sw and nd:
            lib.sw_invert_nd(MUBAR * MUBAR - EPSBAR * EPSBAR)                # ndratcor_monomial.c:78 (after the single-flavour type: it overwrites sw_inv)
        out = scal["types"][name] = {"nd": nd, "sw": sw}
        # ---- arbitrary coefficients: one application of Z on eta
        keep = monomial(nd, sw, ARB, 3)
        delta = h.tmrc_apply_Z(sp(ZU), sp(ZD), sp(0), sp(1))
        out["arb"] = dict(ARB, np=3, delta=delta, iters=h.tmrc_iter0(),
                          norms=[lib.square_norm(sp(ZU), N, 0)] + ([lib.square_norm(sp(ZD), N, 0)] if nd else []))
        if full:
            arrs[name + "_arb_Z_up"] = r.spinor(ZU, N).copy()
            if nd:
                arrs[name + "_arb_Z_dn"] = r.spinor(ZD, N).copy()
        # ---- the fitted approximation
        if full:
            lo, hi, herm = interval(nd, sw)
            mu, rmu, A, err = fit_inverse_sqrt(0.95 * lo, 1.05 * hi, FIT_NP)
            fits[name] = {"mu": mu, "rmu": rmu, "A": A, "np": FIT_NP, "interval": [lo, hi], "fitted_on": [0.95 * lo, 1.05 * hi], "fit_error": err,
                          "hermiticity_defect": herm, "max_iter": FIT_MAXITER, "accprec": FIT_ACCPREC, "rel_prec": FIT_REL}
        c = fits[name]
        keep = monomial(nd, sw, c, FIT_NP)
        delta = h.tmrc_apply_Z(sp(ZU), sp(ZD), sp(0), sp(1))
        fit = out["fit"] = dict(c, delta=delta, iters=h.tmrc_iter0(),
                                norms=[lib.square_norm(sp(ZU), N, 0)] + ([lib.square_norm(sp(ZD), N, 0)] if nd else []))
        if full:
            arrs[name + "_fit_Z_up"] = r.spinor(ZU, N).copy()
            if nd:
                arrs[name + "_fit_Z_dn"] = r.spinor(ZD, N).copy()
        lib.assign(sp(PF), sp(0), N)
        lib.assign(sp(PF2), sp(1), N)
        deltas, napp = (d * 6)(), i()
        keep = monomial(nd, sw, c, FIT_NP)
        e0 = h.tmrc_heatbath(sp(PF), sp(PF2), w, c["accprec"], deltas, C.byref(napp))
        if not 2 <= napp.value <= 5:
            sys.exit("%s %s: the heatbath took %d applications of Z (deltas %s): no fixture written" % (tag, name, napp.value, list(deltas)))
        fit["heatbath"] = {"energy0": e0, "napp": napp.value, "deltas": list(deltas)[:napp.value], "iters": h.tmrc_iter0(),
                           "pf_norms": [lib.square_norm(sp(PF), N, 0)] + ([lib.square_norm(sp(PF2), N, 0)] if nd else [])}
        if full:
            arrs[name + "_pf_up"] = r.spinor(PF, N).copy()
            if nd:
                arrs[name + "_pf_dn"] = r.spinor(PF2, N).copy()
        keep = monomial(nd, sw, c, FIT_NP)
        e1 = h.tmrc_acc(sp(PF), sp(PF2), w, c["accprec"], deltas, C.byref(napp))
        if not 2 <= napp.value <= 5:
            sys.exit("%s %s: the acceptance step took %d applications of Z (deltas %s): no fixture written" % (tag, name, napp.value, list(deltas)))
        fit["acc"] = {"energy1": e1, "napp": napp.value, "deltas": list(deltas)[:napp.value], "iters": h.tmrc_iter0(), "dH": e1 - e0,
                      "w_norms": [lib.square_norm(sp(W + 4), N, 0)] + ([lib.square_norm(sp(W + 5), N, 0)] if nd else [])}
        if full:
            arrs[name + "_w4"] = r.spinor(W + 4, N).copy()
            if nd:
                arrs[name + "_w5"] = r.spinor(W + 5, N).copy()
        del keep
        print(tag, name, "fit error %.2e" % c["fit_error"], "Z: delta %.3e" % fit["delta"], "heatbath", fit["heatbath"]["napp"], fit["heatbath"]["deltas"],
              "acc", fit["acc"]["napp"], fit["acc"]["deltas"], "dH %.3e" % fit["acc"]["dH"])
    return scal, arrs


def restate(scal, arrs):
    """Every quantity also carries the deviation of tests/ratcor_restate.py from it (`restate_vs_ref`): the GPU tests take 8 x that as
    their bound.  The restatement must take the reference's number of applications and of iterations."""
    import numpy as np
    from oracle.nd_restate import cplx
    from oracle.oraclebind import Oracle
    from tests import ratcor_restate as rr
    from tests.util import random_gauge, random_spinor
    T, L = scal["T"], scal["L"]
    orc = Oracle(T, L, L, L, kappa=scal["kappa"], mu=0.0, threads=8)
    if arrs is not None:
        base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
        orc.set_gauge(base["gauge"])
        eta = (cplx(base["k_s"]), cplx(base["k_c"]))
    else:
        orc.set_gauge(random_gauge(scal["gauge_seed"], orc.VPR))
        eta = tuple(cplx(random_spinor(s, orc.Vh)) for s in scal["eta_seeds"])
    for name, t in scal["types"].items():
        dev, counts = rr.deviations(rr.RatCor(orc, name, scal), t["nd"], t, eta[:2 if t["nd"] else 1], arrs, name)
        want = {"arb_iters": t["arb"]["iters"], "fit_iters": t["fit"]["iters"], "heatbath_napp": t["fit"]["heatbath"]["napp"],
                "heatbath_iters": t["fit"]["heatbath"]["iters"], "acc_napp": t["fit"]["acc"]["napp"], "acc_iters": t["fit"]["acc"]["iters"]}
        if counts != want:
            sys.exit("%s: the restatement counts %s, the reference %s: no fixture written" % (name, counts, want))
        t["restate_vs_ref"] = dev
        print("%dx%d" % (T, L), name, "restatement vs reference:", dev)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=3, metavar=("L", "SO", "OUT"))
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        import numpy as np
        L, out = int(a.child[0]), a.child[2]
        fits = {} if L == 4 else json.load(open(os.path.join(out, "fits.json")))
        scal, arrs = gen(L, L, a.child[1], L == 4, fits)
        restate(scal, arrs if L == 4 else None)
        json.dump(scal, open(os.path.join(out, "ref_ratcor_scalars_%dx%d.json" % (L, L)), "w"), indent=1)
        if L == 4:
            json.dump(fits, open(os.path.join(out, "fits.json"), "w"))
            np.savez_compressed(os.path.join(out, "ref_ratcor_4x4.npz"), **arrs)
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_ratcor.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for L in (4, 8):   # everything is written to the temporary directory first: a refusal leaves tests/golden as it was
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(L), so, tmp])
        for f in ("ref_ratcor_scalars_4x4.json", "ref_ratcor_scalars_8x8.json", "ref_ratcor_4x4.npz"):
            shutil.copyfile(os.path.join(tmp, f), os.path.join(GOLD, f))
