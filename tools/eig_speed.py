"""Timing of the eigenvalue measurement on the device (writes profiles/r19_eig_speed.log when given --out).

    python tools/eig_speed.py [--sizes 16 32] [--reps 7] [--pair-reps 3] [--cheb 0 4 8 16] [--out profiles/r19_eig_speed.log]

Per size L^4, on the synthetic gauge field:
(a) tmhip_basis_rotate for (n, k) = (24, 12) and (48, 24) on doublet vectors: time and bytes/s, counting n reads and k writes per
    element, next to the copy yardstick of the same run (tmhip_assign: one read, one write);
(b) the non-operator part of one Lanczos step against j + 1 = 13 and 24 basis vectors, single flavour and doublet: the two
    Gram-Schmidt passes on the pieces of "eig_fused" 1 (tmhip_eig_dots, tmhip_eig_project) and on the single entry points of
    "eig_fused" 0 (tmhip_multi_scalar_prod, tmhip_assign_diff_mul per vector, tmhip_square_norm), beside one operator application.
    Both are driven through the PUBLIC calls from Python: every piece has a synchronisation of its own and eig_project a copy of h
    to the device, which the driver's step (one synchronisation, h stays on the device) does not have; the "driver cycle" lines are
    the driver itself: one whole first cycle (24 steps against 1 .. 24 vectors, max_apps cut so that it ends there), with the
    operator's share taken off, per step;
(c) the phmc_compute_ev pair -- lowest + highest eigenvalue of Qtm_pm_ndpsi, nev = 1, prec 1e-7 -- for every --cheb degree and for
    "eig_fused" 0 at degree 0: operator applications, time, and the same time in iterations of cg_her_nd of the same run.
(a), (b): warm-up first, then the median of --reps timings (min .. max) with HIP events around the calls; (c): --pair-reps.
There is no reference timing to set beside these: the reference's Jacobi-Davidson (jdher_bi) needs LAPACK."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.6931


def timed(lat, fn, reps):
    fn(); lat.sync()
    ev = []
    for _ in range(reps):
        lat.sync()
        lat.event_record(0)
        fn()
        lat.event_record(1)
        lat.sync()
        ev.append(lat.event_elapsed_ms(0, 1))
    return statistics.median(ev), min(ev), max(ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pair-reps", type=int, default=3)
    ap.add_argument("--cheb", type=int, nargs="+", default=[0, 4, 8, 16])
    ap.add_argument("--basis", type=int, nargs="*", default=[], help="(c) again at the fastest degree for these values of eig_basis")
    ap.add_argument("--skip-ab", action="store_true", help="leave out (a) and (b)")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--out")
    a = ap.parse_args()
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda r: "%9.3f ms  (%.3f .. %.3f)" % r
    say("no reference timing: the reference's eigensolver (jdher_bi) needs LAPACK, which is not installed here")
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.125, mu=0.01)
        lat.set_gauge(syn.gauge_field(5, L, L, L, L))
        lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
        N = lat.Vh
        fbytes = 12 * N * 16
        say("== %d^4, median of %d (min .. max), HIP events" % (L, a.reps))
        src = [syn.spinor_field_eo(10 + i, 1, L, L, L, L) for i in range(4)]
        if not a.skip_ab:
            part_ab(lat, syn, say, fmt, a, L, N, fbytes, src)
        part_c(lat, say, fmt, a, L, N, src)
        lat.close()
    finish(say, lines, a)


def part_ab(lat, syn, say, fmt, a, L, N, fbytes, src):
    # ---- (a)
    x, y = lat.field(src[0]), lat.field()
    cp = timed(lat, lambda: lat.assign(y, x, N), a.reps)
    say("(a) copy yardstick (assign, one field)   : %s   %.2f TB/s" % (fmt(cp), 2 * fbytes / cp[0] / 1e9))
    nmax = 48
    vs = [(lat.field(src[i % 4]), lat.field(src[(i + 1) % 4])) for i in range(nmax)]
    rng = np.random.default_rng(1)
    for n, k in ((24, 12), (48, 24)):
        q, _ = np.linalg.qr(rng.standard_normal((n, n)))      # orthogonal: repeated rotations keep the magnitudes
        r = timed(lat, lambda: lat.basis_rotate(vs[:n], q[:, :k]), a.reps)
        rate = (n + k) * 2 * fbytes / r[0] / 1e9
        say("(a) basis_rotate n = %d, k = %d, doublet  : %s   %.2f TB/s = %.0f %% of the copy yardstick" %
            (n, k, fmt(r), rate, 100 * rate / (2 * fbytes / cp[0] / 1e9)))
    # ---- (b)
    wu, wd = lat.field(src[2]), lat.field(src[3])
    lu, ld = lat.field(), lat.field()
    for flav in ("single", "doublet"):
        nd = flav == "doublet"
        op = timed(lat, (lambda: lat.Qtm_pm_ndpsi(lu, ld, wu, wd)) if nd else (lambda: lat.Qtm_pm_psi(lu, wu)), a.reps)
        say("(b) %-7s one operator application     : %s" % (flav, fmt(op)))
        for nv in (13, 24):
            basis = vs[:nv] if nd else [v[0] for v in vs[:nv]]
            w = (wu, wd) if nd else wu

            def fused():
                for _ in range(2):
                    h = lat.eig_dots(basis, w)
                    lat.eig_project(basis, w, h * 1e-3)

            def singles():
                for _ in range(2):
                    segs = ((0, wu), (1, wd)) if nd else ((None, wu),)
                    h = sum(np.concatenate([lat.multi_scalar_prod([(b[s] if nd else b) for b in basis[f:f + 20]], ws, N)
                                            for f in range(0, nv, 20)]) for s, ws in segs)
                    for s, ws in segs:
                        for i, b in enumerate(basis):
                            lat.assign_diff_mul(ws, b[s] if nd else b, h[i] * 1e-3, N)
                    for s, ws in segs:
                        lat.square_norm(ws, N)
            rf, rs = timed(lat, fused, a.reps), timed(lat, singles, a.reps)
            say("(b) %-7s step against %2d vectors, eig_fused 1 : %s   = %.2f operator applications" % (flav, nv, fmt(rf), rf[0] / op[0]))
            say("(b) %-7s step against %2d vectors, eig_fused 0 : %s   singles / fused %.2f" % (flav, nv, fmt(rs), rs[0] / rf[0]))
        # the driver itself: a run capped so that it ends with the first cycle (24 steps, then one residual)
        cyc = {}
        for fo in (1, 0):
            lat.set_option("eig_fused", fo)
            run = (lambda: lat.eigenvalues_nd(1, which="highest", prec=1e-30, max_apps=25)) if nd else \
                  (lambda: lat.eigenvalues(1, which="highest", prec=1e-30, max_apps=25))
            cyc[fo] = timed(lat, run, a.reps)
        lat.set_option("eig_fused", 1)
        per = {fo: (cyc[fo][0] - 25 * op[0]) / 24 for fo in (1, 0)}
        say("(b) %-7s driver cycle, eig_fused 1 : %s   vector part per step %.4f ms = %.2f operator applications" % (flav, fmt(cyc[1]), per[1], per[1] / op[0]))
        say("(b) %-7s driver cycle, eig_fused 0 : %s   vector part per step %.4f ms; singles / fused %.2f" % (flav, fmt(cyc[0]), per[0], per[0] / per[1]))
    for f in [x, y, wu, wd, lu, ld] + [g for v in vs for g in v]:
        f.free()


def part_c(lat, say, fmt, a, L, N, src):
    # ---- (c)
    K = 50
    qu, qd, pu, pd = (lat.field(src[i]) for i in range(4))

    def cg():
        pu.zero(); pd.zero()
        lat.cg_her_nd(pu, pd, qu, qd, K, 1e-30, 1, N)
    cgt = timed(lat, cg, a.reps)
    say("(c) cg_her_nd, %d iterations              : %s   %.4f ms per iteration" % (K, fmt(cgt), cgt[0] / K))
    for f in (qu, qd, pu, pd):
        f.free()
    best = None
    for fusedopt, degs in ((1, a.cheb), (0, [0])):
        lat.set_option("eig_fused", fusedopt)
        for d in degs:
            res = {}

            def pair():
                res["lo"] = lat.eigenvalues_nd(1, which="lowest", prec=1e-7, max_apps=200000, cheb=d)
                res["hi"] = lat.eigenvalues_nd(1, which="highest", prec=1e-7, max_apps=200000)
            r = timed(lat, pair, a.pair_reps)
            apps = res["lo"]["apps"] + res["hi"]["apps"]
            say("(c) pair, eig_fused %d, eig_cheb %2d (median of %d): %s   %d + %d applications, converged %d + %d, ev %.6e %.6e, = %.0f cg_her_nd iterations" %
                (fusedopt, d, a.pair_reps, fmt(r), res["lo"]["apps"], res["hi"]["apps"], res["lo"]["converged"], res["hi"]["converged"],
                 res["lo"]["evals"][0], res["hi"]["evals"][0], r[0] / (cgt[0] / K)))
            if fusedopt == 1 and (best is None or r[0] < best[1]):
                best = (d, r[0], apps)
    lat.set_option("eig_fused", 1)
    lat.set_option("eig_cheb", 0)
    say("(c) fastest eig_cheb at %d^4: %d" % (L, best[0]))
    for m in a.basis:
        lat.set_option("eig_basis", m)
        res = {}

        def pair():
            res["lo"] = lat.eigenvalues_nd(1, which="lowest", prec=1e-7, max_apps=200000, cheb=best[0])
            res["hi"] = lat.eigenvalues_nd(1, which="highest", prec=1e-7, max_apps=200000)
        r = timed(lat, pair, a.pair_reps)
        say("(c) pair, eig_fused 1, eig_cheb %2d, eig_basis %2d (median of %d): %s   %d + %d applications, converged %d + %d" %
            (best[0], m, a.pair_reps, fmt(r), res["lo"]["apps"], res["hi"]["apps"], res["lo"]["converged"], res["hi"]["converged"]))
    lat.set_option("eig_basis", 24)


def finish(say, lines, a):
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru) and not a.append:
        for l in open(ru):
            if l.startswith("kernel") or "eighip::" in l:
                say("(d) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
