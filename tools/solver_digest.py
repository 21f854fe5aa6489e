"""Digest of a fixed list of solves on one MI355X: one line per solve with the iteration count, the reached precision where the
solver reports one, nd_active_shifts / mms_active_shifts / mms_form, and a SHA-256 over the bytes of every solution field.

    python tools/solver_digest.py [--out FILE]

Only the Python API is used, so the same file runs against any build of the library (put it next to the build to compare two:
`cmp` of the two outputs).  Every sum in the solvers is in fixed order, so two builds that compute the same thing print the same
bytes.  The list: cg_her over both operators, cg_fused_dot 0 / 1 / 2, cg_self 0 / 1, cg_sync 1, loopback 1 / 2 / 3, cg_batch
1 / 4 / 7, max_iter reached before and exactly at convergence; mixed_cg_her and rg_mixed_cg_her over both operators and
cg_fused_dot 0 / 2; cg_her_nd from a zero and a non-zero start; cg_mms_tm_nd and cg_mms_tm with 1 / 5 / 32 shifts (long enough
to drop shifts), nd_fused 0 / 1, all three operators of cg_mms_tm in its fused and unfused forms, rel_prec -1 / 0 / 2;
bicgstab_complex over an e/o, a clover and the FULL operator with bicg_fused 0 / 1; chrono_guess on three vectors with csg_batch
0 / 1; apply_Z and apply_Z_nd over both of their operators with ratcor_fused 0 / 1; Ptilde_ndpsi over both.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import random_gauge, random_spinor   # noqa: E402
from tmlqcd_amd import Lattice                        # noqa: E402
from tmlqcd_amd.hip import TmHipError                 # noqa: E402

KAPPA, MU, CSW = 0.12, 0.05, 1.0
OPS = ("Qtm_pm_psi", "Qsw_pm_psi")
SHIFTS = {1: [0.05], 5: [0.05, 0.15, 0.6, 2.5, 9.0], 32: [0.05 + 0.3 * k for k in range(32)]}
LINES = []


def emit(name, fields, **info):
    h = hashlib.sha256()
    for f in fields:
        h.update(np.ascontiguousarray(f.download()).tobytes())
    line = "%-44s %s sha256=%s" % (name, " ".join("%s=%s" % (k, repr(v)) for k, v in info.items()), h.hexdigest())
    LINES.append(line)
    print(line, flush=True)


def attempt(name, fn):
    """A combination the library refuses is part of the digest as well (the same refusal on every build)."""
    try:
        return fn()
    except TmHipError:
        LINES.append("%-44s refused" % name)
        print(LINES[-1], flush=True)
        return None


def lattice(dims, clover=True):
    lat = Lattice(*dims, kappa=KAPPA, mu=MU)
    g = random_gauge(1, lat.VPR)
    lat.set_gauge(g)
    if clover:
        lat.sw_term(g, KAPPA, CSW)
        lat.sw_invert(0, MU)
    return lat


def options(lat, **kw):
    for k, v in kw.items():
        lat.set_option(k, v)


def cg_her_cases():
    for L in (8, 16):
        lat = lattice((L, L, L, L))
        q, x = lat.field(random_spinor(2, lat.Vh)), lat.field()

        def run(name, op="Qtm_pm_psi", max_iter=1500):
            name = "cg_her L=%d %s %s" % (L, op[:3], name)

            def solve():
                x.zero()
                it, hist = lat.cg_her(x, q, max_iter, 1e-18, 1, lat.Vh, op=op)
                emit(name, [x], it=it, err=float(hist[-1]) if len(hist) else None)
                return it
            return attempt(name, solve)
        for op in OPS:
            for fd in (0, 1, 2):
                for cs in (0, 1):
                    options(lat, cg_fused_dot=fd, cg_self=cs)
                    n = run("fused_dot=%d self=%d" % (fd, cs), op)
            options(lat, cg_fused_dot=2, cg_self=1)
            assert n is not None and n > 3, "the cg_her cases are meant to converge"
            run("max_iter=it", op, max_iter=n)          # converges exactly at max_iter
            run("max_iter=it-3", op, max_iter=n - 3)    # max_iter is reached first
        for batch in (1, 4, 7):
            for cs in (0, 1):
                options(lat, cg_batch=batch, cg_self=cs)
                run("batch=%d self=%d" % (batch, cs))
        options(lat, cg_batch=4, cg_self=1, cg_sync=1)
        run("sync=1")
        options(lat, cg_sync=0)
        if L == 8:
            for loop in (1, 2, 3):      # the split-rank path on one rank: D2D copies, one-rank RCCL, direct stores and direct sums
                lat.set_loopback(loop)
                for op in OPS:
                    for fd in (0, 2):
                        options(lat, cg_fused_dot=fd)
                        run("loopback=%d fused_dot=%d" % (loop, fd), op)
                lat.set_loopback(0)
        lat.close()


def mixed_cases():
    lat = lattice((8, 8, 8, 8))
    q, x = lat.field(random_spinor(2, lat.Vh)), lat.field()

    def mixed(name, op):
        def plain():
            x.zero()
            it, outer = lat.mixed_cg_her(x, q, 3000, 1e-18, 1, lat.Vh, op=op)
            emit("mixed_cg_her " + name, [x], it=it, outer=outer, restarts=lat.mixed_cg_restarts())

        def reliable():
            x.zero()
            it, parts = lat.rg_mixed_cg_her(x, q, 3000, 1e-18, 1, lat.Vh, op=op)
            emit("rg_mixed_cg_her " + name, [x], it=it, parts=parts)
        attempt("mixed_cg_her " + name, plain)
        attempt("rg_mixed_cg_her " + name, reliable)
    for op in OPS:
        for fd in (0, 1, 2):
            options(lat, cg_fused_dot=fd)
            mixed("%s fused_dot=%d" % (op[:3], fd), op)
    options(lat, cg_fused_dot=2)
    for loop in (1, 3):
        lat.set_loopback(loop)
        mixed("Qtm loopback=%d" % loop, "Qtm_pm_psi")
        lat.set_loopback(0)
    lat.close()


def nd_cases():
    for dims in ((8, 8, 8, 8), (4, 6, 4, 6)):
        tag = "x".join(map(str, dims))
        lat = lattice(dims, clover=False)
        lat.set_nd(0.1, 0.05, 0.8)
        qu, qd = lat.field(random_spinor(2, lat.Vh)), lat.field(random_spinor(3, lat.Vh))
        for nf in (1, 0):
            options(lat, nd_fused=nf)
            pu, pd = lat.field(), lat.field()
            it = lat.cg_her_nd(pu, pd, qu, qd, 1500, 1e-18, 1, lat.Vh)
            emit("cg_her_nd %s nd_fused=%d zero start" % (tag, nf), [pu, pd], it=it)
            pu.upload(random_spinor(4, lat.Vh)); pd.upload(random_spinor(5, lat.Vh))
            it = lat.cg_her_nd(pu, pd, qu, qd, 1500, 1e-18, 1, lat.Vh)
            emit("cg_her_nd %s nd_fused=%d start" % (tag, nf), [pu, pd], it=it)
            it = lat.cg_her_nd(pu, pd, qu, qd, 7, 1e-30, 0, lat.Vh)
            emit("cg_her_nd %s nd_fused=%d max_iter=7" % (tag, nf), [pu, pd], it=it)
            for n in (1, 5, 32):
                for rel in (0, 1, -1):
                    it, P = lat.cg_mms_tm_nd(qu, qd, SHIFTS[n], 1500 if rel >= 0 else 45, 1e-18, rel)
                    emit("cg_mms_tm_nd %s nd_fused=%d shifts=%d rel=%d" % (tag, nf, n, rel), [f for p in P for f in p], it=it,
                         active=lat.nd_active_shifts())
                    for p in P:
                        p[0].free(); p[1].free()
        lat.close()


def mms_cases():
    for dims in ((8, 8, 8, 8), (6, 6, 6, 6)):       # 6^4: VOLUME/2 is no multiple of the stencil block, the unfused form
        tag = "x".join(map(str, dims))
        lat = lattice(dims)
        qe, qf = lat.field(random_spinor(2, lat.Vh)), lat.full_field(random_spinor(3, lat.V))
        qq = float(np.sum(qe.download() ** 2))
        for op in ("Qtm_pm_psi", "Qsw_pm_psi", "Q_pm_psi"):
            q = qf if op == "Q_pm_psi" else qe
            for n in (1, 5, 32):
                for rel, eps, max_iter in ((0, 1e-16, 1500), (2, 1e-16 / qq, 1500), (-1, 1e-16, 45)):
                    it, reached, P = lat.cg_mms_tm(q, SHIFTS[n], max_iter, eps, rel, op=op)
                    emit("cg_mms_tm %s %s shifts=%d rel=%d" % (tag, op[:3], n, rel), P, it=it, reached=reached,
                         active=lat.mms_active_shifts(), form=lat.mms_form())
                    if rel == 0 and n == 5 and it > 1:   # the stopping test fires exactly in the last allowed iteration
                        it2, reached2, P2 = lat.cg_mms_tm(q, SHIFTS[n], it, eps, rel, op=op, P=P)
                        emit("cg_mms_tm %s %s shifts=%d max_iter=it" % (tag, op[:3], n), P2, it=it2, reached=reached2,
                             active=lat.mms_active_shifts(), form=lat.mms_form())
                    for p in P:
                        p.free()
        options(lat, cg_fused_dot=0, cg_batch=7)
        it, reached, P = lat.cg_mms_tm(qe, SHIFTS[5], 1500, 1e-16, 0)
        emit("cg_mms_tm %s Qtm fused_dot=0 batch=7" % tag, P, it=it, reached=reached, active=lat.mms_active_shifts(), form=lat.mms_form())
        lat.close()


def bicg_cases():
    lat = lattice((8, 8, 8, 8))
    for op in ("Mtm_plus_sym_psi", "Qsw_plus_psi", "D_psi"):
        full = op == "D_psi"
        n = lat.V if full else lat.Vh
        q, x = lat.field(random_spinor(2, n), kind=int(full)), lat.field(kind=int(full))
        for fused in (1, 0):
            options(lat, bicg_fused=fused)
            name = "bicgstab_complex %s bicg_fused=%d" % (op, fused)

            def solve():
                x.zero()
                it, hist = lat.bicgstab_complex(x, q, 1500, 1e-18, 1, n, op=op)
                emit(name, [x], it=it, err=float(hist[-1]))
            attempt(name, solve)
    options(lat, bicg_fused=1)
    lat.close()


def chrono_cases():
    lat = lattice((8, 8, 8, 8))
    phi = lat.field(random_spinor(2, lat.Vh))
    for op in OPS:
        for batch in (1, 0):
            options(lat, csg_batch=batch)
            vs, trial = [lat.field() for _ in range(3)], lat.field()
            for k, v in enumerate(vs):
                lat.chrono_add_solution(v, lat.field(random_spinor(10 + k, lat.Vh)))
            name = "chrono_guess %s n=3 csg_batch=%d" % (op[:3], batch)

            def guess():
                G, bn = lat.chrono_guess(trial, phi, vs, op=op)
                emit(name, [trial] + vs, G=hashlib.sha256(G.tobytes()).hexdigest()[:16], b=hashlib.sha256(bn.tobytes()).hexdigest()[:16])
            attempt(name, guess)
    options(lat, csg_batch=1)
    lat.close()


def ratcor_poly_cases():
    mu, rmu, A = [0.1, 0.3, 0.9], [0.2, 0.5, 0.1], 1.05
    coefs = [1.0, -0.6, 0.35, -0.2, 0.1, -0.05, 0.02, -0.01]
    lat = lattice((8, 8, 8, 8))
    lat.set_mu(0.0)                      # the correction monomials' clover operator wants the inverse of sw_invert(EE, 0.)
    lat.sw_invert(0, 0.0)
    lat.set_nd(0.1, 0.05, 0.8)
    lat.sw_invert_nd(0.1 * 0.1 - 0.05 * 0.05)
    l = [lat.field(random_spinor(2, lat.Vh)), lat.field(random_spinor(3, lat.Vh))]
    k = [lat.field(), lat.field()]
    for fused in (1, 0):
        options(lat, ratcor_fused=fused)
        for op in OPS:
            name = "apply_Z %s ratcor_fused=%d" % (op[:3], fused)

            def single():
                delta, it = lat.apply_Z(k[0], l[0], mu, rmu, A, 1500, 1e-18, 1, op=op)
                emit(name, k[:1], it=it, delta=delta)
            attempt(name, single)
        for op in ("Qtm_pm_ndpsi", "Qsw_pm_ndpsi"):
            name = "apply_Z_nd %s ratcor_fused=%d" % (op[:3], fused)

            def doublet():
                delta, it = lat.apply_Z_nd(k, l, mu, rmu, A, 1500, 1e-18, 1, op=op)
                emit(name, k, it=it, delta=delta)
            attempt(name, doublet)
    options(lat, ratcor_fused=1)
    for op in ("Qtm_pm_ndpsi", "Qsw_pm_ndpsi"):
        name = "Ptilde_ndpsi %s" % op[:3]

        def ptilde():
            lat.Ptilde_ndpsi(k[0], k[1], coefs, l[0], l[1], 0.01, 1.0, op=op)
            emit(name, k)
        attempt(name, ptilde)
    lat.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    cg_her_cases()
    mixed_cases()
    nd_cases()
    mms_cases()
    bicg_cases()
    chrono_cases()
    ratcor_poly_cases()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
