"""Timing of the chronological solver guess on the device (writes profiles/r11_csg_speed.log when given --out).

    python tools/csg_speed.py [--sizes 16 32] [--ns 2 4 8] [--reps 7] [--out profiles/r11_csg_speed.log]

Per size L^4 and list length n, on the synthetic gauge field: (a) chrono_guess with csg_batch 1 against 0 -- the plain path is the
reference's call sequence on the device, (b) multi_scalar_prod of n fields against n calls of scalar_prod, (c) iterations and
time of cg_her from zero and from the guess, (d) the kernels' lines of the build's resource table.  The list is built as a monomial
builds it (solve, chrono_add_solution) from right-hand sides phi0 + 0.1 k d + 0.1 r_k.  Every figure: warm-up call first, then the
median of `reps` timings with the min .. max spread, taken with HIP events around the call (the stream's time, host round trips
of the reductions included) and, in brackets, the host clock around the synchronised call."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(lat, fn, reps, prepare=None):
    if prepare:
        prepare()
    fn(); lat.sync()
    ev, host = [], []
    for _ in range(reps):
        if prepare:
            prepare()
        lat.sync()
        t0 = time.perf_counter()
        lat.event_record(0)
        fn()
        lat.event_record(1)
        lat.sync()
        host.append((time.perf_counter() - t0) * 1e3)
        ev.append(lat.event_elapsed_ms(0, 1))
    return statistics.median(ev), min(ev), max(ev), statistics.median(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--ns", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda r: "%9.3f ms  (%.3f .. %.3f) [host %.3f]" % r
    solve = (5000, 1e-14, 1)
    slower = []
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.125, mu=0.01)
        lat.set_gauge(syn.gauge_field(5, L, L, L, L))
        N = lat.Vh
        nmax = max(a.ns)
        phi0, d = syn.spinor_field_eo(10, 1, L, L, L, L), syn.spinor_field_eo(11, 1, L, L, L, L)
        rhs = [lat.field(phi0 + 0.1 * k * d + 0.1 * syn.spinor_field_eo(20 + k, 1, L, L, L, L)) for k in range(nmax + 1)]
        sols = []
        for k in range(nmax):                                   # the list: normalised solutions, oldest first
            x = lat.field().zero()
            lat.cg_her(x, rhs[k], *solve, N)
            v = lat.field()
            lat.chrono_add_solution(v, x)
            sols.append(v)
        say("== %d^4, median of %d (min .. max), HIP events [host clock]" % (L, a.reps))
        for n in a.ns:
            keep = [lat.field() for _ in range(n)]
            for k in range(n):
                lat.assign(keep[k], sols[nmax - n + k], N)
            vs = [lat.field() for _ in range(n)]
            phi, trial = rhs[nmax], lat.field()

            def restore():                                       # chrono_guess orthogonalises the list in place: every call starts from the same one
                for k in range(n):
                    lat.assign(vs[k], keep[k], N)
            res = {}
            for b in (1, 0):
                lat.set_option("csg_batch", b)
                res[b] = timed(lat, lambda: lat.chrono_guess(trial, phi, vs), a.reps, restore)
            lat.set_option("csg_batch", 1)
            say("(a) n = %d chrono_guess, csg_batch 1 : %s" % (n, fmt(res[1])))
            say("    n = %d chrono_guess, csg_batch 0 : %s   plain / batched %.2f" % (n, fmt(res[0]), res[0][0] / res[1][0]))
            if res[1][0] > res[0][0]:
                slower.append((L, n))
            one = timed(lat, lambda: lat.multi_scalar_prod(vs, phi, N), a.reps)
            seq = timed(lat, lambda: [lat.scalar_prod(v, phi, N) for v in vs], a.reps)
            say("(b) n = %d multi_scalar_prod         : %s" % (n, fmt(one)))
            say("    n = %d calls of scalar_prod      : %s   ratio %.2f" % (n, fmt(seq), seq[0] / one[0]))
            its = {}
            x = lat.field()
            t0 = timed(lat, lambda: its.__setitem__("zero", lat.cg_her(x, phi, *solve, N)[0]), max(3, a.reps // 2), lambda: x.zero())

            def guess():
                restore()
                lat.chrono_guess(x, phi, vs)
            tg = timed(lat, lambda: its.__setitem__("guess", lat.cg_her(x, phi, *solve, N)[0]), max(3, a.reps // 2), guess)
            say("(c) n = %d cg_her from zero          : %s   %d iterations" % (n, fmt(t0), its["zero"]))
            say("    n = %d cg_her from the guess     : %s   %d iterations; guess + solve %.3f ms against %.3f ms" % (n, fmt(tg), its["guess"], res[1][0] + tg[0], t0[0]))
        lat.close()
    say("batched path slower than the plain path at: %s" % (slower if slower else "no measured point"))
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "csg_" in l or l.startswith("dotr_kernel"):
                say("(d) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
