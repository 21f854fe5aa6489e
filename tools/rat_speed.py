"""Timing of the rational monomials' force on the device (writes profiles/r08_rat_speed.log when given --out).

    python tools/rat_speed.py [--sizes 16 32] [--np 12] [--reps 7] [--out profiles/r08_rat_speed.log]

Per size L^4: (a) one deriv_Sb_batch launch of n = 2 np pairs against 2 np launches of deriv_Sb on the same fields, (b) ndrat_force
with rat_batch 1, 2, 4, 12, (c) ndrat_derivative split into its solve and its force, (d) the same for rat, (e) the kernel's line of
the build's resource table.  Every figure: warm-up call first, then the median of `reps` timings (host clock around a synchronised
call) with the min .. max spread."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(lat, fn, reps):
    fn(); lat.sync()
    ts = []
    for _ in range(reps):
        lat.sync()
        t0 = time.perf_counter()
        fn()
        lat.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--np", type=int, default=12)
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
    np_ = a.np
    mu = [0.02 * 1.6 ** j for j in range(np_)]
    rmu = [0.01 * 1.5 ** j for j in range(np_)]
    solve = (5000, 1e-16, 1)
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.125, mu=0.0)
        lat.set_gauge(syn.gauge_field(5, L, L, L, L))
        lat.set_nd(0.12, 0.1, 0.6)
        say("== %d^4, np = %d, median of %d (min .. max)" % (L, np_, a.reps))
        chi = [(lat.field(syn.spinor_field_eo(10 + j, 1, L, L, L, L)), lat.field(syn.spinor_field_eo(50 + j, 1, L, L, L, L))) for j in range(np_)]
        ls = [c[0] for c in chi] + [c[1] for c in chi]
        ks = ls[1:] + ls[:1]
        fs = rmu + rmu
        lat.derivative_zero()
        n = len(ls)
        one = timed(lat, lambda: lat.deriv_Sb_batch(0, ls, ks, fs), a.reps)
        seq = timed(lat, lambda: [lat.deriv_Sb(0, l, k, f) for l, k, f in zip(ls, ks, fs)], a.reps)
        say("(a) deriv_Sb_batch, n = %d pairs, one launch : %s" % (n, fmt(one)))
        say("    %d launches of deriv_Sb               : %s   ratio %.2f" % (n, fmt(seq), seq[0] / one[0]))
        for b in (1, 2, 4, 12):
            lat.set_option("rat_batch", b)
            say("(b) ndrat_force, rat_batch %2d              : %s" % (b, fmt(timed(lat, lambda: lat.ndrat_force(chi, mu, rmu, 0.6), a.reps))))
        lat.set_option("rat_batch", 4)
        pu, pd = chi[0]
        P = [(lat.field(), lat.field()) for _ in range(np_)]
        its = []
        sol = timed(lat, lambda: its.append(lat.cg_mms_tm_nd(pu, pd, mu, *solve, P=P)[0]), max(3, a.reps // 2))
        tot = timed(lat, lambda: lat.ndrat_derivative(pu, pd, mu, rmu, 0.6, *solve), max(3, a.reps // 2))
        say("(c) ndrat_derivative                        : %s   of which solve %s (%d iterations)" % (fmt(tot), fmt(sol), its[-1]))
        Q = [lat.field() for _ in range(np_)]
        its = []
        sol = timed(lat, lambda: its.append(lat.cg_mms_tm(pu, mu, *solve, P=Q)[0]), max(3, a.reps // 2))
        tot = timed(lat, lambda: lat.rat_derivative(pu, mu, rmu, *solve), max(3, a.reps // 2))
        frc = timed(lat, lambda: lat.rat_force(Q, rmu), a.reps)
        say("(d) rat_derivative                          : %s   of which solve %s (%d iterations); rat_force alone %s" % (fmt(tot), fmt(sol), its[-1], fmt(frc)))
        lat.close()
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "deriv_Sb_batch" in l:
                say("(e) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
