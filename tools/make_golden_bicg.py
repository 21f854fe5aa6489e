"""TEST INFRASTRUCTURE ONLY: fixtures of BiCGstab (tests/golden/ref_bicg_4x4.npz, ref_bicg_scalars_4x4.json,
ref_bicg_scalars_8x6x4x12.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_bicg.py --ref /path/to/tmLQCD        (or TMLQCD_REF=/path/to/tmLQCD in the environment)

solver/bicgstab_complex.c and whichever of linalg/scalar_prod.c, assign_diff_mul.c, assign_add_mul_add_mul.c and
assign_mul_bra_add_mul_ket_add.c libtmref.so does not define are compiled here, in place from the reference tree, into a temporary
directory (nothing is copied into this repository), linked with tools/bicg_harness.c against libtmref.so, and the reference's
bicgstab_complex is run on every case of CASES below: one per operator, both stopping rules, a non-zero starting guess and a max_iter
cut.  4^4: the gauge field of ref_mms_4x4.npz, the solutions are stored.  8x6x4x12 (scalars only): tests.util.random_gauge(123456).
Sources and the starting guess come from tests/bicg_restate.py fields(), so that a test can make them again.

Recorded per case: the return value; the recursive residual of the last stopping test (the reference prints it at debug level 3);
the true residual |Q - A P|^2 with the reference's own operator; their ratio; the norm of the solution.  `margin` = 10 x the largest
ratio of all cases of both shapes is what a test allows a true residual above the stopping bound.  4^4 only: sigma_min(A) from a
dense SVD of the operator of the CPU oracle, for the bound |P_a - P_b| <= 2 sqrt(bound) / sigma_min(A) between two solutions that both
meet the stopping bound.  The generator also repeats every KIND_M case in the NumPy restatement with every scalar product multiplied
by 1 + 1e-13 N(0,1) and refuses to write a fixture whose count moves: those counts are what the tests pin.
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
SRCS = ["solver/bicgstab_complex.c"]
LINALG = {"scalar_prod": "linalg/scalar_prod.c", "assign_diff_mul": "linalg/assign_diff_mul.c",
          "assign_add_mul_add_mul": "linalg/assign_add_mul_add_mul.c", "assign_mul_bra_add_mul_ket_add": "linalg/assign_mul_bra_add_mul_ket_add.c"}
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
KAPPA, MU_CLOVER = 0.125, 0.02
SHAPES = {"4x4": (4, 4, 4, 4), "8x6x4x12": (8, 6, 4, 12)}


def case(op, g_mu=0.02, eps_sq=1e-18, rel_prec=1, guess=False, max_iter=1000):
    return {"op": op, "g_mu": g_mu, "eps_sq": eps_sq, "rel_prec": rel_prec, "guess": guess, "max_iter": max_iter}


CASES = {
    "4x4": {
        "qtm_plus": case("Qtm_plus_psi"), "qtm_minus": case("Qtm_minus_psi", g_mu=0.1), "mtm_plus": case("Mtm_plus_psi"),
        "mtm_minus": case("Mtm_minus_psi", g_mu=0.1), "mtm_plus_sym": case("Mtm_plus_sym_psi"), "mtm_minus_sym": case("Mtm_minus_sym_psi"),
        "qsw_plus": case("Qsw_plus_psi", g_mu=MU_CLOVER), "qsw_minus": case("Qsw_minus_psi", g_mu=MU_CLOVER),
        "msw_plus": case("Msw_plus_psi", g_mu=MU_CLOVER), "d_psi": case("D_psi", g_mu=0.1),
        "mtm_plus_sym_abs": case("Mtm_plus_sym_psi", eps_sq=1e-14, rel_prec=0), "d_psi_abs": case("D_psi", g_mu=0.1, eps_sq=1e-14, rel_prec=0),
        "mtm_plus_sym_guess": case("Mtm_plus_sym_psi", guess=True), "mtm_plus_sym_cut": case("Mtm_plus_sym_psi", max_iter=5),
    },
    "8x6x4x12": {
        "mtm_plus_sym": case("Mtm_plus_sym_psi"), "mtm_plus_abs": case("Mtm_plus_psi", eps_sq=1e-14, rel_prec=0),
        "qtm_plus": case("Qtm_plus_psi", g_mu=0.1), "msw_plus": case("Msw_plus_psi", g_mu=MU_CLOVER), "d_psi": case("D_psi", g_mu=0.1),
        "mtm_plus_sym_cut": case("Mtm_plus_sym_psi", max_iter=5),
    },
}


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    have = subprocess.run(["nm", "-D", "--defined-only", refso], stdout=subprocess.PIPE, text=True, check=True).stdout
    have = {l.split()[-1] for l in have.splitlines() if l.strip()}
    srcs = SRCS + [f for name, f in LINALG.items() if name not in have]
    objs = []
    for f in srcs + [os.path.join(ROOT, "tools", "bicg_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmbicg.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,--no-undefined", "-lm"])
    return so


class Capture:
    """what the C library prints on file descriptor 1 while the block runs"""

    def __init__(self, flush):
        self.flush, self.text = flush, ""

    def __enter__(self):
        sys.stdout.flush()
        self.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(1)
        os.dup2(self.tmp.fileno(), 1)
        return self

    def __exit__(self, *exc):
        self.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def sigma_min(A, n):
    import numpy as np
    M = np.zeros((12 * n, 12 * n), dtype=np.complex128)
    e = np.zeros((n, 4, 3), dtype=np.complex128)
    for j in range(12 * n):
        e.reshape(-1)[j] = 1.0
        M[:, j] = A(e).reshape(-1)
        e.reshape(-1)[j] = 0.0
    return float(np.linalg.svd(M, compute_uv=False)[-1])


def gen(tag, so):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.nd_restate import cplx
    from oracle.refbind import RefLattice
    from tests import bicg_restate as br
    from tests.util import random_gauge
    dims = SHAPES[tag]
    full = tag == "4x4"
    r = RefLattice(*dims, kappa=KAPPA, mu=0.02, nfields=16)
    cs = C.CDLL(so)
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    cs.bicgstab_complex.argtypes = [vp, vp, i, d, i, i, vp]
    cs.bicgstab_complex.restype = i
    cs.tmbicg_set_debug.argtypes = [i]
    r.random_fields(123456)
    mms = np.load(os.path.join(GOLD, "ref_mms_4x4.npz"))
    c_sw = json.load(open(os.path.join(GOLD, "ref_mms_scalars_4x4.json")))["c_sw"]
    gauge = mms["gauge"] if full else random_gauge(123456, r.V)
    r.gauge()[:] = gauge
    r.mark_gauge_dirty()
    lib, V, sp = r.lib, r.V, r.sp
    for n in ("Qsw_plus_psi", "Qsw_minus_psi", "Msw_plus_psi"):
        getattr(lib, n).argtypes = [vp, vp]
        getattr(lib, n).restype = None
    B, X, W = 0, 1, 2
    scal = {"dims": list(dims), "kappa": KAPPA, "c_sw": c_sw, "spinor_seed": br.SPINOR_SEED, "cases": {},
            "gauge_from": "ref_mms_4x4.npz" if full else "tests.util.random_gauge(123456, VOLUME)"}
    arrs = {}
    line = re.compile(r"^(\d+) (\d\.\d+e[+-]\d+)\s*$", re.M)
    sig, clover_mu = {}, None
    for name, cse in CASES[tag].items():
        op, mu = cse["op"], cse["g_mu"]
        N = V if op == "D_psi" else V // 2
        r.set_kappa_mu(KAPPA, mu)
        if op in br.CLOVER and clover_mu is None:   # one clover term for all clover cases (MU_CLOVER)
            r.clover(c_sw, mu)
            clover_mu = mu
        assert op not in br.CLOVER or clover_mu == mu
        Q, P0 = br.case_fields(cse, V)
        r.spinor(B, N)[:] = Q
        r.spinor(X, N)[:] = P0
        cs.tmbicg_set_debug(3)
        with Capture(cs.tmbicg_flush) as cap:
            it = cs.bicgstab_complex(sp(X), sp(B), cse["max_iter"], cse["eps_sq"], cse["rel_prec"], N, r.fnptr(op))
        cs.tmbicg_set_debug(0)
        errs = line.findall(cap.text)
        assert errs and (it == -1 or int(errs[-1][0]) == it), (name, it, cap.text[-200:])
        P = r.spinor(X, N).copy()
        getattr(lib, op)(sp(W), sp(X))
        true = float(np.sum((Q - r.spinor(W, N)) ** 2))
        out = dict(cse)
        out.update({"iters": it, "kind": "M" if op in br.KIND_M else "Q", "sol_norm": float(np.sum(P ** 2)), "true_res": true})
        if it > 0:
            out["rec_res"] = float(errs[-1][1])
            out["ratio"] = true / out["rec_res"]
            out["bound"] = br.bound_of(cse, Q)
        # the restatement over the CPU oracle: the counts a test pins must not move with the last bits of the scalar products
        orc = br.oracle_for(dims, gauge, KAPPA, c_sw, cse)
        A = br.operator(orc, op)
        it_np, P_np, _ = br.bicgstab_complex(A, cplx(P0), cplx(Q), cse["max_iter"], cse["eps_sq"], cse["rel_prec"])
        if out["kind"] == "M":
            rng = np.random.default_rng(7)
            it_noise, _, _ = br.bicgstab_complex(A, cplx(P0), cplx(Q), cse["max_iter"], cse["eps_sq"], cse["rel_prec"],
                                                 noise=lambda z: z * (1 + 1e-13 * rng.standard_normal()))
            assert it_np == it and it_noise == it, (name, it, it_np, it_noise)
        out["iters_restated"] = it_np
        if full:
            key = (op, mu)
            if key not in sig:
                sig[key] = sigma_min(A, N)
            out["sigma_min"] = sig[key]
            arrs[name + "_P"] = P
        scal["cases"][name] = out
        print("%s %s: iters %d (restated %d), true residual %.3e, ratio %s" % (tag, name, it, it_np, true, out.get("ratio")), file=sys.stderr)
    scal["max_ratio"] = max(c["ratio"] for c in scal["cases"].values() if "ratio" in c)
    json.dump(scal, open(os.path.join(GOLD, "ref_bicg_scalars_%s.json" % tag), "w"), indent=1)
    if full:
        np.savez_compressed(os.path.join(GOLD, "ref_bicg_%s.npz" % tag), **arrs)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "SO"))
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        gen(a.child[0], a.child[1])
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_bicg.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for tag in SHAPES:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", tag, so])
    # the margin of the true-residual test: 10 x the largest true-to-recursive ratio the reference showed on any case
    files = [os.path.join(GOLD, "ref_bicg_scalars_%s.json" % tag) for tag in SHAPES]
    docs = [json.load(open(f)) for f in files]
    margin = 10.0 * max(dd["max_ratio"] for dd in docs)
    for f, dd in zip(files, docs):
        dd["margin"] = margin
        json.dump(dd, open(f, "w"), indent=1)
