"""TEST INFRASTRUCTURE ONLY: fixtures of the clover rational monomial and the tr-log energies
(tests/golden/ref_cloverrat_4x4.npz, ref_cloverrat_scalars_{4x4,8x8}.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_cloverrat.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

operator/clover_det.c, solver/cg_mms_tm.c, linalg/assign_mul_add_mul_r.c and linalg/assign_add_mul.c are compiled here, in place from the
reference tree, into a temporary directory (nothing is copied into this repository), linked with tools/cloverrat_harness.c against
libtmref.so (which holds the clover operators), and run with c_sw != 0 after sw_term + sw_invert(EE, 0.):
sw_trace(EE, mu) for mu = 0 and one mu != 0, sw_trace(OO, mu), sw_trace_nd(EE, mubar, epsbar) at the points of
tests/ndsw_restate.POINTS; the statements of rat_monomial.c:95-139 for CLOVERRAT on given solution fields (np = 3, no solve inside,
trlog 0 and 1), :194-199 and :244-250; and cg_mms_tm on Qsw_pm_psi for its iteration count.

4^4: the seed-123456 gauge field and the four random spinors of tests/golden/ref_nd_4x4.npz (same seed, same calls -- asserted here), so
they are not stored again; per-site outputs are stored on every second site (SITES) with the square norm over ALL sites in the scalars
file.  8^4: scalars only (the traces and the iteration count), on tests.util.random_gauge / random_spinor with the seeds recorded, so
that a test needs no reference library to rebuild the inputs.

Every trace is also compared with tests/cloverrat_restate.py (numpy.linalg.slogdet / det on the CPU oracle's sw): the distance in
units of sum |per-site term| goes to the scalars file ("trace_distance"); tests/test_gpu_trlog.py allows 1e-13 of that scale.
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
SRCS = ["operator/clover_det.c", "solver/cg_mms_tm.c", "linalg/assign_mul_add_mul_r.c", "linalg/assign_add_mul.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
KAPPA, C_SW = 0.125, 1.57                             # those of ref_ndsw_*
NFIELDS = 48
SITES = slice(0, None, 2)
TRACE_MU = 0.23
MU, RMU = [0.031, 0.27, 1.9], [0.0042, 0.057, 0.81]
NU, RNU = [0.019, 0.16, 1.1], [0.0031, 0.044, 0.63]
SHIFTS = [0.02, 0.15, 0.6, 2.5, 9.0]
SEED8 = (8123, 8124)                                  # 8^4: random_gauge / random_spinor seeds
EO, OE, EE, OO = 0, 1, 0, 1


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "cloverrat_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmcloverrat.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def gen(T, L, so, full):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.oraclebind import Oracle
    from oracle.refbind import RefLattice
    from tests import cloverrat_restate as cr
    from tests import ndsw_restate as sw
    from tests.util import random_gauge, random_spinor
    r = RefLattice(T, L, L, L, kappa=KAPPA, mu=0.0, nfields=NFIELDS)
    h = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    h.sw_trace.restype = d; h.sw_trace.argtypes = [i, d]
    h.sw_trace_nd.restype = d; h.sw_trace_nd.argtypes = [i, d, d]
    h.assign_add_mul.argtypes = [vp, vp, d, d, i]     # _Complex double by value: (re, im) as two consecutive doubles in SSE registers
    h.tmcr_cg_mms_tm.argtypes = [C.POINTER(vp), vp, C.POINTER(d), i, i, d, i, i, C.POINTER(d)]
    lib, N, sp = r.lib, r.V // 2, r.sp
    tag = "%dx%d" % (T, L)
    scal = {"T": T, "L": L, "kappa": KAPPA, "c_sw": C_SW, "mu": MU, "rmu": RMU, "nu": NU, "rnu": RNU, "np": len(MU), "norms": {}}
    if full:
        r.random_fields(123456)
        for k in (1, 2, 3):
            lib.tmref_random_spinor_eo(k)
        base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
        assert np.array_equal(base["gauge"], r.gauge())
        for k, name in enumerate(("k_s", "k_c", "j_s", "j_c")):
            assert np.array_equal(base[name], r.spinor(k, N)), name
        scal["seed"] = 123456
    else:
        r.gauge()[:] = random_gauge(SEED8[0], r.V)
        r.mark_gauge_dirty()
        r.spinor(0, N)[:] = random_spinor(SEED8[1], N)
        scal["gauge_seed"], scal["source_seed"] = SEED8
    for n in ("Qsw_plus_psi", "Qsw_pm_psi"):
        getattr(lib, n).argtypes = [vp, vp]
        getattr(lib, n).restype = None
    lib.H_eo_sw_inv_psi.argtypes = [vp, vp, i, i, d]
    lib.sw_spinor_eo.argtypes = [i, vp, vp, d]
    lib.sw_deriv.argtypes = [i, d]
    lib.tmref_sw_all.argtypes = [d, d]
    lib.assign.argtypes = [vp, vp, i]
    lib.assign_add_mul_r.argtypes = [vp, vp, d, i]
    lib.square_norm.restype = d; lib.square_norm.argtypes = [vp, i, i]
    lib.scalar_prod_r.restype = d; lib.scalar_prod_r.argtypes = [vp, vp, i, i]
    sw_ref, swi = r.clover(C_SW, 0.0)                 # init_sw_fields, sw_term, sw_invert(EE, 0.)  (rat_monomial.c:76-78)
    scal["sw_norm"] = float((sw_ref ** 2).sum())
    # ---- the tr-log energies, and their distance to the restatement over the CPU oracle
    orc = Oracle(T, L, L, L, kappa=KAPPA, mu=0.0)
    orc.set_gauge(r.gauge().copy())
    cl = cr.clover_of(orc, KAPPA, C_SW)
    tr, dist = {}, {}

    def trace(name, ref_val, restated):
        want, scale = restated
        tr[name] = ref_val
        dist[name] = abs(ref_val - want) / scale
        scal.setdefault("trace_scale", {})[name] = scale
    trace("sw_trace_EE_0", h.sw_trace(EE, 0.0), cr.sw_trace(cl, EE, 0.0))
    trace("sw_trace_EE_mu", h.sw_trace(EE, TRACE_MU), cr.sw_trace(cl, EE, TRACE_MU))
    trace("sw_trace_OO_mu", h.sw_trace(OO, TRACE_MU), cr.sw_trace(cl, OO, TRACE_MU))
    for name, (mb, eb, _) in sw.POINTS.items():
        trace("sw_trace_nd_EE_" + name, h.sw_trace_nd(EE, mb, eb), cr.sw_trace_nd(cl, EE, mb, eb))
    scal["trace_mu"], scal["points"] = TRACE_MU, {k: list(v[:2]) for k, v in sw.POINTS.items()}
    scal["traces"], scal["trace_distance"] = tr, dist
    arrs = {}
    if full:
        # ---- the monomial on chi = (k_s, k_c, j_s), eta = j_c
        CHI, ETA = [0, 1, 2], 3
        W0, W2, W3, TMP, PF = 20, 22, 23, 24, 25
        scal["chi"], scal["eta"] = ["k_s", "k_c", "j_s"], "j_c"
        for trlog in (0, 1):                          # rat_monomial.c:66-73, :95-139 (forcefactor = 1, :81)
            r.derivative()[:] = 0
            lib.tmref_swpm_zero()
            for j in range(len(MU) - 1, -1, -1):
                lib.Qsw_plus_psi(sp(W0), sp(CHI[j]))
                lib.H_eo_sw_inv_psi(sp(W2), sp(CHI[j]), EO, -1, 0.0)
                r.deriv_Sb(OE, W0, W2, RMU[j])
                lib.H_eo_sw_inv_psi(sp(W3), sp(W0), EO, +1, 0.0)
                r.deriv_Sb(EO, W3, CHI[j], RMU[j])
                lib.sw_spinor_eo(EE, sp(W2), sp(W3), RMU[j])
                lib.sw_spinor_eo(OO, sp(W0), sp(CHI[j]), RMU[j])
            if trlog:
                lib.sw_deriv(EE, 0.0)
            lib.tmref_sw_all(KAPPA, C_SW)
            arrs["cloverrat_derivative_trlog%d" % trlog] = r.derivative().copy()
        # heatbath, :177 and :194-199
        lib.assign(sp(PF), sp(ETA), N)
        scal["cloverrat_energy0"] = lib.square_norm(sp(PF), N, 1)
        for j in range(len(NU) - 1, -1, -1):
            lib.Qsw_plus_psi(sp(TMP), sp(CHI[j]))
            h.assign_add_mul(sp(TMP), sp(CHI[j]), 0.0, -NU[j], N)
            h.assign_add_mul(sp(PF), sp(TMP), 0.0, RNU[j], N)
        scal["norms"]["cloverrat_pf"] = lib.square_norm(sp(PF), N, 0)
        arrs["cloverrat_pf"] = r.spinor(PF, N)[SITES].copy()
        # acceptance, :244-250, on pf = eta
        lib.assign(sp(W0), sp(ETA), N)
        for j in range(len(MU) - 1, -1, -1):
            lib.assign_add_mul_r(sp(W0), sp(CHI[j]), RMU[j], N)
        scal["cloverrat_energy1"] = lib.scalar_prod_r(sp(ETA), sp(W0), N, 1)
    # ---- cg_mms_tm on Qsw_pm_psi at twisted mass 0: the iteration count
    ns = len(SHIFTS)
    P = (vp * ns)(*[sp(30 + k) for k in range(ns)])
    sh = (d * ns)(*SHIFTS)
    eps_sq, rel, reached = 1e-22, 0, d()
    it = h.tmcr_cg_mms_tm(P, sp(0), sh, ns, 2000, eps_sq, rel, N, C.byref(reached))
    scal["cg_mms_tm"] = {"op": "Qsw_pm_psi", "shifts": SHIFTS, "eps_sq": eps_sq, "rel_prec": rel, "max_iter": 2000, "iters": it,
                         "sol_norms": [lib.square_norm(sp(30 + k), N, 0) for k in range(ns)]}
    json.dump(scal, open(os.path.join(GOLD, "ref_cloverrat_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_cloverrat_%s.npz" % tag), **arrs)
    print(tag, "cg_mms_tm", it, "largest trace distance / scale %.2e" % max(dist.values()))


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
        sys.exit("make_golden_cloverrat.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for L in (4, 8):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(L), so])
