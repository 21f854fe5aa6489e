"""Timing of the correction monomials' device path (writes profiles/r15_ratcor_speed.log when given --out).

    python tools/ratcor_speed.py [--sizes 16 32] [--np 12] [--reps 7] [--out profiles/r15_ratcor_speed.log]

Per size L^4: (a) one rat_sum launch against the 1 + np single calls it replaces (and 2 + np with the factor A^2), one flavour and both,
(b) diff_sqnorm against diff + square_norm, (c) apply_Z and apply_Z_nd with "ratcor_fused" 1 against "ratcor_fused" 0 (the reference's
call sequence) on the same build, (d) the kernels' lines of the build's resource table.  Every figure: a warm-up call, then the median of
`reps` timings between two HIP events on the context's stream, with the min .. max spread."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(lat, fn, reps):
    fn(); lat.sync()
    ts = []
    for _ in range(reps):
        lat.event_record(0)
        fn()
        lat.event_record(1)
        lat.sync()
        ts.append(lat.event_elapsed_ms(0, 1))
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
    mu = [0.05 * 1.6 ** j for j in range(np_)]
    rmu = [0.01 * 1.5 ** j for j in range(np_)]
    A = 0.9
    solve = (5000, 1e-16, 1)
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.125, mu=0.0)
        lat.set_gauge(syn.gauge_field(5, L, L, L, L))
        lat.set_nd(0.12, 0.1, 0.6)
        N = lat.Vh
        say("== %d^4, np = %d, median of %d (min .. max), HIP events" % (L, np_, a.reps))
        chi = [(lat.field(syn.spinor_field_eo(10 + j, 1, L, L, L, L)), lat.field(syn.spinor_field_eo(50 + j, 1, L, L, L, L))) for j in range(np_)]
        src = (lat.field(syn.spinor_field_eo(3, 1, L, L, L, L)), lat.field(syn.spinor_field_eo(4, 1, L, L, L, L)))
        out, tmp = (lat.field(), lat.field()), (lat.field(), lat.field())

        def singles(nf, c):
            for f in range(nf):
                lat.assign(out[f], src[f], N)
            for j in range(np_ - 1, -1, -1):
                for f in range(nf):
                    lat.assign_add_mul_r(out[f], chi[j][f], rmu[j], N)
            if c != 1.0:
                for f in range(nf):
                    lat.mul_r(tmp[f], c, out[f], N)
        for nf, c in ((1, 1.0), (1, A * A), (2, 1.0), (2, A * A)):
            if nf == 1:
                one = timed(lat, lambda: lat.rat_sum(out[0], src[0], [p[0] for p in chi], rmu, c), a.reps)
            else:
                one = timed(lat, lambda: lat.rat_sum_nd(out, src, chi, rmu, c), a.reps)
            seq = timed(lat, lambda: singles(nf, c), a.reps)
            ncalls = nf * (1 + np_ + (c != 1.0))
            say("(a) rat_sum, %d flavour%s, c %s: one launch %s   %2d single calls %s   ratio %.2f"
                % (nf, " " if nf == 1 else "s", "= 1  " if c == 1.0 else "= A^2", fmt(one), ncalls, fmt(seq), seq[0] / one[0]))
        for nf in (1, 2):
            if nf == 1:
                one = timed(lat, lambda: lat.diff_sqnorm(out[0], src[0]), a.reps)
            else:
                one = timed(lat, lambda: lat.diff_sqnorm_nd(out, src), a.reps)
            seq = timed(lat, lambda: [(lat.diff(out[f], out[f], src[f], N), lat.square_norm(out[f], N, 1)) for f in range(nf)], a.reps)
            say("(b) diff_sqnorm, %d flavour%s     : one launch %s   diff + square_norm %s   ratio %.2f"
                % (nf, " " if nf == 1 else "s", fmt(one), fmt(seq), seq[0] / one[0]))
        reps = max(3, a.reps // 2)
        for nd in (0, 1):
            res = {}
            for fused in (0, 1):
                lat.set_option("ratcor_fused", fused)
                its = []
                if nd:
                    res[fused] = timed(lat, lambda: its.append(lat.apply_Z_nd(out, src, mu, rmu, A, *solve)[1]), reps)
                else:
                    res[fused] = timed(lat, lambda: its.append(lat.apply_Z(out[0], src[0], mu, rmu, A, *solve)[1]), reps)
            say("(c) %s: ratcor_fused 1 %s   ratcor_fused 0 (the call sequence) %s   ratio %.3f   (first solve: %d iterations)"
                % ("apply_Z_nd" if nd else "apply_Z   ", fmt(res[1]), fmt(res[0]), res[0][0] / res[1][0], its[-1]))
        lat.close()
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "rat_sum" in l or "diff_sqnorm" in l:
                say("(d) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
