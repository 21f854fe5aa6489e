"""Timing of the polynomial monomial NDPOLY on the device (writes profiles/r14_poly_speed.log when given --out).

    python tools/poly_speed.py [--sizes 16 32] [--n 49] [--ptilde 98] [--reps 7] [--out profiles/r14_poly_speed.log]

Per size L^4, with n = MDPolyDegree and a Ptilde of `ptilde` coefficients (the degree of the 4^4 fixture):
 (a) one Clenshaw step -- Qtm_pm_ndpsi alone; the rotated form of tmhip_Ptilde_ndpsi (the operator + one launch of the four-term kernel for
     both flavours); the reference's statement sequence of Ptilde_nd.c:155-174 on the entry points that were there before (four assign, the
     operator, two one-field combinations, two assign) -- and the ratios to the operator;
 (b) the force: the reference's call order of ndpoly_monomial.c:79-117 on Q_tau1_sub_const_ndpsi / H_eo_tm_ndpsi / deriv_Sb / assign, against
     tmhip_ndpoly_derivative with poly_batch 1, 2, 4, 12, 32;
 (c) ndpoly_heatbath, and ndpoly_acc with one correction (precision_hfinal = inf);
 (d) the kernel's line of the build's resource table.
Every figure: one warm-up call, then the median of `reps` timings between two HIP events on the context's stream, with the min .. max
spread."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(lat, fn, reps):
    fn(); lat.sync()
    ts = []
    for _ in range(reps):
        lat.sync()
        lat.event_record(0)
        fn()
        lat.event_record(1)
        lat.sync()
        ts.append(lat.event_elapsed_ms(0, 1))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--n", type=int, default=49)
    ap.add_argument("--ptilde", type=int, default=98)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda r: "%9.3f ms  (%.3f .. %.3f)" % r
    n = a.n
    th = np.pi * (np.arange(n - 1) + 0.5) / (n - 1)
    roots = list(0.8 * np.exp(1j * th)) + list(0.8 * np.exp(-1j * th[::-1]))
    md = [2.0] + [0.5 ** j for j in range(1, n)]
    pt = [2.0] + [0.7 ** j for j in range(1, a.ptilde)]
    Cpol, inv, evmin = 1.0, 0.6, 0.005
    EO, OE = 0, 1
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.125, mu=0.0)
        lat.set_gauge(syn.gauge_field(5, L, L, L, L))
        lat.set_nd(0.12, 0.1, inv)
        N = lat.Vh
        say("== %d^4, n = %d, Ptilde of %d coefficients, median of %d (min .. max)" % (L, n, a.ptilde, a.reps))
        pf = lat.field(syn.spinor_field_eo(10, 1, L, L, L, L)), lat.field(syn.spinor_field_eo(11, 1, L, L, L, L))
        # ---- (a) one Clenshaw step
        d, dd, q, sv, aux = ([lat.field(), lat.field()] for _ in range(5))
        lat.assign(d[0], pf[0], N); lat.assign(d[1], pf[1], N)
        f1, f2, c = 4 / (1 - evmin), -2 * (1 + evmin) / (1 - evmin), 0.3
        op = timed(lat, lambda: lat.Qtm_pm_ndpsi(q[0], q[1], d[0], d[1]), a.reps)

        def rotated():
            lat.Qtm_pm_ndpsi(q[0], q[1], d[0], d[1])
            lat.comb4_ndpsi(dd, d, q, dd, pf, f2, f1, -1.0, c)

        def statements():   # Ptilde_nd.c:155-174
            lat.assign(sv[0], d[0], N); lat.assign(sv[1], d[1], N)
            lat.assign(aux[0], d[0], N); lat.assign(aux[1], d[1], N)
            lat.Qtm_pm_ndpsi(q[0], q[1], aux[0], aux[1])
            lat.assign_mul_add_mul_add_mul_add_mul_r(d[0], q[0], dd[0], pf[0], f2, f1, -1.0, c)
            lat.assign_mul_add_mul_add_mul_add_mul_r(d[1], q[1], dd[1], pf[1], f2, f1, -1.0, c)
            lat.assign(dd[0], sv[0], N); lat.assign(dd[1], sv[1], N)
        rot = timed(lat, rotated, a.reps)
        for x in d + dd:
            x.zero()
        sta = timed(lat, statements, a.reps)
        say("(a) Qtm_pm_ndpsi                              : %s" % fmt(op))
        say("    Clenshaw step, rotated (operator + 1 launch): %s   ratio to the operator %.3f" % (fmt(rot), rot[0] / op[0]))
        say("    Clenshaw step, the reference's statements   : %s   ratio to the operator %.3f" % (fmt(sta), sta[0] / op[0]))
        for x in d + dd + q + sv + aux:
            x.free()
        # ---- (b) the force
        chi = [(lat.field(), lat.field()) for _ in range(n + 1)]
        w = lat.field(), lat.field()
        ff = -Cpol * inv

        def baseline():   # ndpoly_monomial.c:79-117
            lat.assign(chi[0][0], pf[0], N); lat.assign(chi[0][1], pf[1], N)
            for k in range(1, n - 1):
                lat.Q_tau1_sub_const_ndpsi(chi[k][0], chi[k][1], chi[k - 1][0], chi[k - 1][1], roots[k - 1], Cpol, inv)
            lat.assign(chi[n][0], chi[n - 2][0], N); lat.assign(chi[n][1], chi[n - 2][1], N)
            for j in range(n - 1, 0, -1):
                lat.assign(chi[n - 1][0], chi[n][0], N); lat.assign(chi[n - 1][1], chi[n][1], N)
                lat.Q_tau1_sub_const_ndpsi(chi[n][0], chi[n][1], chi[n - 1][0], chi[n - 1][1], roots[2 * n - 3 - j], Cpol, inv)
                lat.H_eo_tm_ndpsi(w[0], w[1], chi[j - 1][0], chi[j - 1][1], EO)
                lat.deriv_Sb(EO, w[0], chi[n][0], ff); lat.deriv_Sb(EO, w[1], chi[n][1], ff)
                lat.H_eo_tm_ndpsi(w[0], w[1], chi[n][0], chi[n][1], EO)
                lat.deriv_Sb(OE, chi[j - 1][0], w[0], ff); lat.deriv_Sb(OE, chi[j - 1][1], w[1], ff)
        lat.derivative_zero()
        base = timed(lat, baseline, a.reps)
        say("(b) force, the reference's call order on the single entry points : %s" % fmt(base))
        for x in chi:
            x[0].free(); x[1].free()
        best = None
        for b in (1, 2, 4, 12, 32):
            lat.set_option("poly_batch", b)
            r = timed(lat, lambda: lat.ndpoly_derivative(pf[0], pf[1], roots, Cpol, inv), a.reps)
            say("    ndpoly_derivative, poly_batch %2d                            : %s   baseline / this %.2f" % (b, fmt(r), base[0] / r[0]))
            if best is None or r[0] < best[1]:
                best = (b, r[0])
        say("    fastest: poly_batch %d" % best[0])
        lat.set_option("poly_batch", best[0])
        # ---- (c) heatbath and acceptance
        eta = lat.field(), lat.field()

        def heatbath():
            lat.assign(eta[0], pf[0], N); lat.assign(eta[1], pf[1], N)
            lat.ndpoly_heatbath(eta[0], eta[1], roots, Cpol, inv, pt, evmin, 1.0)
        say("(c) ndpoly_heatbath (+ two assign)            : %s" % fmt(timed(lat, heatbath, a.reps)))
        say("    ndpoly_acc, one correction                : %s" % fmt(timed(lat, lambda: lat.ndpoly_acc(pf[0], pf[1], roots, Cpol, inv, md, pt, evmin, 1.0, np.inf), a.reps)))
        lat.close()
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "comb4_kernel" in l:
                say("(d) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
