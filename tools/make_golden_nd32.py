"""TEST INFRASTRUCTURE ONLY: fixtures of the fp32 doublet and of rg_mixed_cg_her_nd (tests/golden/ref_nd32_*).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref_hs.so, the half-spinor build of the reference tree and
the only one with the fp32 twins):

    python tools/make_golden_nd32.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

oracle/Makefile does not build operator/tm_operators_nd.c, operator/tm_operators_nd_32.c, solver/rg_mixed_cg_her_nd.c,
solver/cg_her_nd.c or linalg/mul_r_32.c.  They are compiled here, in place from the reference tree, into a temporary directory
(nothing is copied into this repository), linked with tools/nd32_harness.c against libtmref_hs.so, and run on the seed-123456
random gauge field and its fp32 conversion, with the parameters of tests/golden/ref_nd_*.
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
SRCS = ["operator/tm_operators_nd.c", "operator/tm_operators_nd_32.c", "solver/rg_mixed_cg_her_nd.c", "solver/cg_her_nd.c", "linalg/mul_r_32.c"]
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1",
        "-D_USE_HALFSPINOR=1"]
MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.6931
NFIELDS, DUM = 40, 32
DELTAS = [0.1, 0.01, 1e-3, 1e-5, 0.5]
MAX_ITER, EPS_SQ, REL_PREC = 5000, 1e-20, 1


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref_hs.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref_hs.so missing: run build() first")
    objs = []
    for f in SRCS + [os.path.join(ROOT, "tools", "nd32_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmnd32.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref_hs.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def captured(call):
    """call() with the C library's stdout captured: (its return value, the text)."""
    with tempfile.TemporaryFile() as cap:
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(cap.fileno(), 1)
        try:
            ret = call()
            C.CDLL(None).fflush(None)
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        cap.seek(0)
        return ret, cap.read().decode()


def gen(T, L, so, full):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    kappa = 0.125
    r = RefLattice(T, L, L, L, kappa=kappa, mu=0.0, nfields=NFIELDS, hs=True)
    nd = C.CDLL(so)
    vp, d, i, fl = C.c_void_p, C.c_double, C.c_int, C.c_float
    nd.tmnd32_set.argtypes = [d, d, d]
    nd.tmnd32_set_dum.argtypes = [i]
    nd.tmnd32_set_debug.argtypes = [i]
    nd.Qtm_pm_ndpsi.argtypes = [vp] * 4
    nd.Qtm_pm_ndpsi_32.argtypes = [vp] * 4
    nd.M_ee_inv_ndpsi_32.argtypes = [vp] * 4 + [fl, fl]
    nd.M_oo_sub_g5_ndpsi_32.argtypes = [vp] * 6 + [fl, fl]
    nd.cg_her_nd.argtypes = [vp] * 4 + [i, d, i, i, vp]
    nd.tmnd32_rg_mixed_cg_her_nd.argtypes = [vp] * 4 + [d, i, d, i, i]
    nd.tmnd32_set_dum(DUM)
    nd.tmnd32_set(MUBAR, EPSBAR, INVMAXEV)
    r.random_fields(123456)          # the gauge field, then tmref_convert_gauge_32()
    for k in (1, 2):
        r.lib.tmref_random_spinor_eo(k)
    lib, N, sp = r.lib, r.V // 2, r.sp
    scal = {"T": T, "L": L, "kappa": kappa, "seed": 123456, "mubar": MUBAR, "epsbar": EPSBAR, "invmaxev": INVMAXEV,
            "max_iter": MAX_ITER, "eps_sq": EPS_SQ, "rel_prec": REL_PREC}
    arrs = {}

    def f32():   # a spinor32 field of our own: g_spinor_field32[0..5] are Qtm_pm_ndpsi_32's scratch
        return np.zeros((N + 1, 4, 3, 2), dtype=np.float32)

    def p32(a):
        return a.ctypes.data_as(vp)

    q_up, q_dn = r.spinor(1, N), r.spinor(2, N)
    k_s, k_c, l_s, l_c, e_s, e_c, o_s, o_c = (f32() for _ in range(8))
    lib.assign_to_32(p32(k_s), sp(1), N)
    lib.assign_to_32(p32(k_c), sp(2), N)
    nd.Qtm_pm_ndpsi_32(p32(l_s), p32(l_c), p32(k_s), p32(k_c))
    nd.M_ee_inv_ndpsi_32(p32(e_s), p32(e_c), p32(k_s), p32(k_c), MUBAR, EPSBAR)
    nd.M_oo_sub_g5_ndpsi_32(p32(o_s), p32(o_c), p32(k_s), p32(k_c), p32(l_s), p32(l_c), MUBAR, EPSBAR)   # j = the Qtm_pm_ndpsi_32 pair
    # the reference's own fp32 operator against its fp64 one, L2-relative over both flavours
    nd.Qtm_pm_ndpsi(sp(3), sp(4), sp(1), sp(2))
    a64 = np.concatenate([r.spinor(3, N).ravel(), r.spinor(4, N).ravel()])
    a32 = np.concatenate([l_s[:N].ravel(), l_c[:N].ravel()]).astype(np.float64)
    scal["op32_vs_op64"] = float(np.linalg.norm(a32 - a64) / np.linalg.norm(a64))
    if full:
        # the links are not stored again: they are those of ref_nd_4x4.npz (the same seed in either build of the reference)
        if not np.array_equal(r.gauge(), np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))["gauge"]):
            sys.exit("make_golden_nd32.py: the seed-%d gauge field differs from the one in tests/golden/ref_nd_4x4.npz" % scal["seed"])
        arrs.update(q_up=q_up.copy(), q_dn=q_dn.copy(), q32_up=k_s[:N].copy(), q32_dn=k_c[:N].copy(),
                    Qtm_pm_ndpsi_32_s=l_s[:N].copy(), Qtm_pm_ndpsi_32_c=l_c[:N].copy(),
                    M_ee_inv_ndpsi_32_s=e_s[:N].copy(), M_ee_inv_ndpsi_32_c=e_c[:N].copy(),
                    M_oo_sub_g5_ndpsi_32_s=o_s[:N].copy(), M_oo_sub_g5_ndpsi_32_c=o_c[:N].copy())
    # cg_her_nd from a zero start: the fp64 solve the mixed one is compared with
    r.spinor(5)[:] = 0
    r.spinor(6)[:] = 0
    it = nd.cg_her_nd(sp(5), sp(6), sp(1), sp(2), MAX_ITER, EPS_SQ, REL_PREC, N, C.cast(nd.Qtm_pm_ndpsi, vp))
    scal["cg_her_nd"] = {"iters": it}
    x_up, x_dn = r.spinor(5, N).copy(), r.spinor(6, N).copy()
    if full:
        arrs.update(cg_her_nd_up=x_up, cg_her_nd_dn=x_dn)
    qnorm = float(np.sum(q_up ** 2) + np.sum(q_dn ** 2))
    runs = []
    for delta in DELTAS:
        nd.tmnd32_set_debug(1)
        it, log = captured(lambda: nd.tmnd32_rg_mixed_cg_her_nd(sp(7), sp(8), sp(1), sp(2), delta, MAX_ITER, EPS_SQ, REL_PREC, N))
        nd.tmnd32_set_debug(0)
        run = {"delta": delta, "iters": it, "switched_to_dp": "switching to DP" in log}
        m = re.search(r"RG_mixed CG_ND: iter_out: (\d+) iter_in_sp: (\d+) iter_in_dp: (\d+)", log)   # the solver's own debug-level-1 line
        if m:
            run.update(iter_out=int(m.group(1)), iter_in_sp=int(m.group(2)), iter_in_dp=int(m.group(3)))
        m = re.search(r"N_outer: (\d+)", log)
        if m:
            run["N_outer"] = int(m.group(1))
        if it > 0:
            nd.Qtm_pm_ndpsi(sp(9), sp(10), sp(7), sp(8))
            res = float(np.sum((r.spinor(9, N) - q_up) ** 2) + np.sum((r.spinor(10, N) - q_dn) ** 2))
            run["true_residual_rel"] = res / qnorm
            du, dd = r.spinor(7, N) - x_up, r.spinor(8, N) - x_dn
            run["distance_to_cg_her_nd"] = float(np.sqrt((np.sum(du ** 2) + np.sum(dd ** 2)) / (np.sum(x_up ** 2) + np.sum(x_dn ** 2))))
            if full:
                arrs["rg_up_%g" % delta] = r.spinor(7, N).copy()
                arrs["rg_dn_%g" % delta] = r.spinor(8, N).copy()
        runs.append(run)
    scal["rg_mixed_cg_her_nd"] = runs
    tag = "%dx%d" % (T, L)
    json.dump(scal, open(os.path.join(GOLD, "ref_nd32_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_nd32_%s.npz" % tag), **arrs)
    print(tag, "cg_her_nd", scal["cg_her_nd"]["iters"], "op32_vs_op64 %.2e" % scal["op32_vs_op64"])
    for run in runs:
        print("  ", run)


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
        sys.exit("make_golden_nd32.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for L in (4, 8):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(L), so])
