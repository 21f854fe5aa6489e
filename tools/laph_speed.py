"""Timing of the LapH eigensystem on the device (writes profiles/r22_laph_speed.log when given --out).

    python tools/laph_speed.py [--sizes 16x32 32x64] [--reps 7] [--out profiles/r22_laph_speed.log]

Per size L^3 x T, on the synthetic gauge field:
(1) tmhip_laph_apply on all slices: time and bytes/s on the byte model of the operator -- six links of 144 B, one colour vector in and
    one out of 48 B per site, the six gathered neighbours counted as cache hits -- next to the copy yardstick of the same run
    (tmhip_assign on spinor fields: one read, one write) and to tmhip_measure_oriented_plaquettes, a kernel that walks the same
    lexicographic links (its time per site; it reads 24 links per site where the caches do not help);
(2) the non-operator part of a Lanczos step at basis fill 16, 64 and 127 -- dots, projection, dots, projection, scaling -- batched
    over all T slices in one call each, against the same calls issued slice by slice (nt = 1, T times).  Both go through the PUBLIC
    pieces, every one of which synchronises and copies its scalars; the driver's own step has one synchronisation for all of it;
(3) the Chebyshev step: "laph_fused" 1 (one stencil launch) against 0 (the plain operator and the combination pass);
(4) a whole eigensystem for nev 32 and 64, prec 1e-8: applications per slice, time, the share of host time in the small
    eigenproblems, a sweep of "laph_cheb" (0, 4, 8, 16) and of "laph_basis" (nev + 8, 16, 32) -- the sweeps at the first size only.
(1) - (3): warm-up first, then the median of --reps timings (min .. max) with HIP events around the calls; (4): one run each, host clock.
There is no reference timing to set beside these: the reference's eigen-driver (eigenvalues_Jacobi.c) cannot be built."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--sizes", nargs="+", default=["16x32", "32x64"], help="LxT: an L^3 x T lattice")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nev", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--cheb", type=int, nargs="+", default=[0, 4, 8, 16])
    ap.add_argument("--skip-eig", action="store_true", help="leave out (4)")
    ap.add_argument("--out")
    a = ap.parse_args()
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda r: "%9.3f ms  (%.3f .. %.3f)" % r
    say("no reference timing: the reference's eigen-driver (eigenvalues_Jacobi.c) needs LAPACK and lime.h and does not compile here")
    for si, size in enumerate(a.sizes):
        L, T = (int(x) for x in size.split("x"))
        lat = Lattice(T, L, L, L)
        lat.set_gauge(syn.gauge_field(5, T, L, L, L))
        V, S3 = lat.V, L * L * L
        rng = np.random.default_rng(7)
        say("== %d^3 x %d, median of %d (min .. max), HIP events" % (L, T, a.reps))
        k, l, p = lat.cvfield(rng.standard_normal((T, S3, 3, 2))), lat.cvfield(), lat.cvfield(rng.standard_normal((T, S3, 3, 2)))
        # (1)
        r = timed(lat, lambda: lat.laph_apply(l, k), a.reps)
        say("(1) laph_apply, all %d slices        %s  %7.1f us  %.2f TB/s on 960 B/site" % (T, fmt(r), 1e3 * r[0], V * 960 / r[0] / 1e9))
        f0, f1 = lat.field(syn.spinor_field_eo(3, 1, T, L, L, L)), lat.field()
        r = timed(lat, lambda: lat.assign(f1, f0, lat.Vh), a.reps)
        say("    copy yardstick (tmhip_assign)      %s  %.2f TB/s (one read, one write)" % (fmt(r), 2 * 12 * lat.Vh * 16 / r[0] / 1e9))
        r = timed(lat, lambda: lat.measure_oriented_plaquettes(), a.reps)
        say("    measure_oriented_plaquettes        %s  %.3f ns per site (one synchronisation inside)" % (fmt(r), 1e6 * r[0] / V))
        f0.free(); f1.free()
        # (3)
        coef = np.tile(np.array([[-0.4, 1.2, -1.0]]), (T, 1))
        for fused in (1, 0):
            lat.set_option("laph_fused", fused)
            r = timed(lat, lambda: lat.laph_apply(l, k, coef=coef, prev=p), a.reps)
            say("(3) Chebyshev step, laph_fused %d      %s  (a copy of 3 T coefficients and one synchronisation inside)" % (fused, fmt(r)))
        lat.set_option("laph_fused", 1)
        # (2)
        bh = rng.standard_normal((T, S3, 3, 2))
        basis = [lat.cvfield(bh) for _ in range(127)]   # one host image for all: only the traffic matters here
        for fill in (16, 64, 127):
            vs = basis[:fill]
            h = np.zeros((T, fill), dtype=np.complex128)

            def step(t0, nt):
                hh = lat.laph_dots(vs, l, t0, nt)
                lat.laph_project(vs, l, 1e-3 * hh, t0, nt)
                hh = lat.laph_dots(vs, l, t0, nt)
                lat.laph_project(vs, l, 1e-3 * hh, t0, nt)
                lat.laph_normalise(l, l, t0, nt)
            lat.laph_apply(l, k)
            rb = timed(lat, lambda: step(0, T), a.reps)
            rs = timed(lat, lambda: [step(t, 1) for t in range(T)], max(3, a.reps // 2))
            say("(2) Gram-Schmidt twice + scaling, fill %3d: batched %s   slice by slice %s   ratio %.1f" % (fill, fmt(rb), fmt(rs), rs[0] / rb[0]))
        for f in basis:
            f.free()
        # (4)
        if not a.skip_eig:
            for nev in a.nev:
                def run(tag):
                    t = time.perf_counter()
                    r = lat.laph_eigensystem(nev, prec=1e-8, max_apps=60000)
                    wall = time.perf_counter() - t
                    small, total = lat.laph_timing()
                    say("(4) nev %2d %-28s apps per slice %5d .. %5d  converged %d .. %d  %8.3f s  small eigenproblems %4.1f %% of the host time" % (
                        nev, tag, r["apps"].min(), r["apps"].max(), r["converged"].min(), r["converged"].max(), wall, 100.0 * small / total))
                run("defaults (cheb %d, basis nev + 32)" % lat.get_option("laph_cheb"))
                if si == 0:
                    old = lat.get_option("laph_cheb")
                    for c in a.cheb:
                        lat.set_option("laph_cheb", c)
                        run("laph_cheb %d" % c)
                    lat.set_option("laph_cheb", old)
                    for extra in (8, 16, 32):
                        lat.set_option("laph_basis", nev + extra)
                        run("laph_basis nev + %d" % extra)
                    lat.set_option("laph_basis", 0)
        for f in (k, l, p):
            f.free()
        lat.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
