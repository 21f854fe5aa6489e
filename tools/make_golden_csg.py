"""TEST INFRASTRUCTURE ONLY: fixtures of the chronological solver guess (tests/golden/ref_csg_4x4.npz, ref_csg_scalars_4x4.json,
ref_csg_scalars_8x8.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_csg.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

solver/chrono_guess.c, solver/lu_solve.c and whichever of linalg/scalar_prod.c, assign_diff_mul.c, mul.c and assign_add_mul.c
libtmref.so does not define are compiled here, in place from the reference tree, into a temporary directory (nothing is copied into
this repository), linked with tools/csg_harness.c against libtmref.so, and the statements of a det-type monomial are run with
f = Qtm_pm_psi: for every right-hand side b_k   chrono_guess; cg_her from the trial vector; chrono_add_solution   into a list of
csg_N = 5 vectors.  The first right-hand side meets an empty list and starts from zero (the reference's chrono_guess reads
index_array[-1] there).  b_k = phi0 + 0.1 k d + 0.1 r_k with independent random r_k, so the solutions span as many dimensions as
there are vectors in the list.  Recorded while the list holds n = 1, 2 and 5 vectors: the list before and after chrono_guess, phi,
the trial vector, G and bn -- the reference keeps them in static buffers, so they are taken again with the reference's own
scalar_prod and Qtm_pm_psi on the list chrono_guess left behind, in its order -- bn after the reference's LUSolve, cond(G), and
the iterations of the reference's cg_her from zero and from the trial vector.  4^4: the seed-123456 gauge field of the other
fixtures, kappa 0.125, mu 0.05.  8^4 (scalars only): tests.util.random_gauge(123456), mu 0.01.  The spinors come from
tests/csg_restate.py rhs_fields, so that a test can make them again.
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
SRCS = ["solver/chrono_guess.c", "solver/lu_solve.c"]
LINALG = {"scalar_prod": "linalg/scalar_prod.c", "assign_diff_mul": "linalg/assign_diff_mul.c", "mul": "linalg/mul.c",
          "assign_add_mul": "linalg/assign_add_mul.c"}
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
KAPPA, MU = 0.125, {4: 0.05, 8: 0.01}
CSG_N, RECORD = 5, (1, 2, 5)
EPS_SQ, MAX_ITER = 1e-14, 2000
NFIELDS = 24


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    have = subprocess.run(["nm", "-D", "--defined-only", refso], stdout=subprocess.PIPE, text=True, check=True).stdout
    have = {l.split()[-1] for l in have.splitlines() if l.strip()}
    srcs = SRCS + [f for name, f in LINALG.items() if name not in have]
    objs = []
    for f in srcs + [os.path.join(ROOT, "tools", "csg_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmcsg.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


def gen(L, so):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.refbind import RefLattice
    from tests.csg_restate import NRHS, SPINOR_SEED, rhs_fields
    from tests.util import random_gauge
    T, mu, full = L, MU[L], L == 4
    r = RefLattice(T, L, L, L, kappa=KAPPA, mu=mu, nfields=NFIELDS)
    cs = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    pi = C.POINTER(i)

    class Cplx(C.Structure):   # _Complex double by value: (re, im) in two SSE registers, returned in xmm0:xmm1
        _fields_ = [("re", d), ("im", d)]
    cs.chrono_guess.argtypes = [vp, vp, C.POINTER(vp), pi, i, i, i, vp]
    cs.chrono_guess.restype = i
    cs.chrono_add_solution.argtypes = [vp, C.POINTER(vp), pi, i, pi, i]
    cs.chrono_add_solution.restype = None
    cs.scalar_prod.argtypes = [vp, vp, i, i]
    cs.scalar_prod.restype = Cplx
    cs.tmcsg_lusolve.argtypes = [i, vp, i, vp]
    cs.tmcsg_set_debug.argtypes = [i]
    cs.tmcsg_set_debug(0)
    r.random_fields(123456)
    if not full:
        r.gauge()[:] = random_gauge(123456, r.V)
        r.mark_gauge_dirty()
    lib, N, sp = r.lib, r.V // 2, r.sp
    f = r.fnptr("Qtm_pm_psi")
    B, TRIAL, ZERO, WORK, LIST, SEQ = 0, 1, 2, 3, 4, 10     # field numbers: right-hand side, guess, zero-start solve, A v_j, the list, the N = 3 list
    b = rhs_fields(N)
    v = (vp * CSG_N)(*[sp(LIST + k) for k in range(CSG_N)])
    idx, n = (i * CSG_N)(), i(0)
    scal = {"T": T, "L": L, "kappa": KAPPA, "mu": mu, "seed": 123456, "spinor_seed": SPINOR_SEED, "csg_N": CSG_N, "nrhs": NRHS,
            "eps_sq": EPS_SQ, "rel_prec": 1, "max_iter": MAX_ITER, "op": "Qtm_pm_psi", "cases": {}, "iters": []}
    arrs = {}
    if full:
        other = np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))
        assert np.array_equal(other["gauge"], r.gauge()), "the seed-123456 gauge field of ref_fields_4x4.npz"
        scal["gauge_from"] = "ref_fields_4x4.npz"

    def dot(a, c):
        z = cs.scalar_prod(a, c, N, 1)
        return complex(z.re, z.im)

    for k in range(NRHS):
        r.spinor(B, N)[:] = b[k]
        nn = n.value
        order = [idx[j] for j in range(nn)]
        before = [r.spinor(LIST + s, N).copy() for s in order]
        if nn == 0:
            r.spinor(TRIAL, N)[:] = 0      # the monomial's first call: nothing stored yet
        else:
            cs.chrono_guess(sp(TRIAL), sp(B), v, idx, CSG_N, nn, N, f)
        guess = r.spinor(TRIAL, N).copy()
        r.spinor(ZERO, N)[:] = 0
        it_zero = lib.cg_her(sp(ZERO), sp(B), MAX_ITER, EPS_SQ, 1, N, f)
        if nn in RECORD and k == nn:
            G = np.zeros((nn, nn), dtype=np.complex128)
            bn = np.zeros(nn, dtype=np.complex128)
            for j in range(nn):
                lib.Qtm_pm_psi(sp(WORK), sp(LIST + order[j]))
                for m in range(j + 1):
                    G[m, j] = dot(sp(LIST + order[m]), sp(WORK))
                    if m != j:
                        G[j, m] = np.conj(G[m, j])
                bn[j] = dot(sp(LIST + order[j]), sp(B))
            Gw, y = G.copy(), bn.copy()
            cs.tmcsg_lusolve(nn, Gw.ctypes.data_as(vp), nn, y.ctypes.data_as(vp))
            after = [r.spinor(LIST + s, N).copy() for s in order]
            comb = sum(y[j] * (after[j][..., 0] + 1j * after[j][..., 1]) for j in range(nn))
            gz = guess[..., 0] + 1j * guess[..., 1]
            assert np.abs(comb - gz).max() <= 1e-10 * np.abs(gz).max(), "G and bn taken again do not give the reference's trial vector"
            case = {"n": nn, "k": k, "G": [[[z.real, z.imag] for z in row] for row in G], "bn": [[z.real, z.imag] for z in bn],
                    "y": [[z.real, z.imag] for z in y], "cond": float(np.linalg.cond(G)), "trial_norm": lib.square_norm(sp(TRIAL), N, 1)}
            if full:
                arrs["n%d_phi" % nn] = b[k].copy()
                arrs["n%d_trial" % nn] = guess
                arrs["n%d_before" % nn] = np.stack(before)
                arrs["n%d_after" % nn] = np.stack(after)
        it_guess = lib.cg_her(sp(TRIAL), sp(B), MAX_ITER, EPS_SQ, 1, N, f)
        if nn in RECORD and k == nn:
            case["iters_zero"], case["iters_guess"] = it_zero, it_guess
            scal["cases"][str(nn)] = case
        scal["iters"].append({"k": k, "n": nn, "zero": it_zero, "guess": it_guess})
        cs.chrono_add_solution(sp(TRIAL), v, idx, CSG_N, C.byref(n), N)
        print("%d^4 k %d n %d: cg_her from zero %d, from the guess %d" % (L, k, nn, it_zero, it_guess), file=sys.stderr)

    # the rotation of the list: seven solutions into a list of three
    v3 = (vp * 3)(*[sp(SEQ + k) for k in range(3)])
    idx3, n3 = (i * 3)(-1, -1, -1), i(0)
    seq = []
    for k in range(7):
        r.spinor(B, N)[:] = b[k % NRHS]
        cs.chrono_add_solution(sp(B), v3, idx3, 3, C.byref(n3), N)
        seq.append({"index_array": [idx3[j] for j in range(3)], "n": n3.value})
    scal["add_sequence_N3"] = seq
    tag = "%dx%d" % (T, L)
    json.dump(scal, open(os.path.join(GOLD, "ref_csg_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_csg_%s.npz" % tag), **arrs)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=2, metavar=("L", "SO"))
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        gen(int(a.child[0]), a.child[1])
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_csg.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for L in (4, 8):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(L), so])
