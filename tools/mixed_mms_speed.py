"""Speed of mixed_cg_mms_tm_nd against cg_mms_tm_nd on one MI355X (writes profiles/r21_mixed_mms_speed.log when given --out).

    python tools/mixed_mms_speed.py [--sizes 16 32] [--reps 7] [--out profiles/r21_mixed_mms_speed.log]

Per size L^4, on the synthetic gauge field, in one process, np = 12 shifts; every figure is the median of --reps timings (min .. max)
with HIP events around the calls, after a warm-up.  A time per iteration is (t(K2) - t(K1)) / (K2 - K1) of two runs with an unreachable
target, so that the start-up and the end of a solve cancel.  K1 = 4 and K2 = 14, and the timing runs of (a) and (b) use twelve shifts
that lie close together (0.01 + 0.001 k): a kernel's time does not depend on the value of a shift, and on this well-conditioned system
(a solve to 1e-14 takes 26 iterations) neither |r|^2 nor a zita falls by rel_delta = 1e-10 within 14 iterations, so that no reliable
update interrupts the loop that is timed (the count is printed with every figure; it must be 0).  What updates cost shows in (c).
(a) the vector part of the eleven further shifts, t(12 shifts) - t(1 shift) per iteration, for "mms32_fused" 0 and 1 and for the fp64
    solver (nd_x_kernel + nd_p_kernel), with the bytes per second each achieves -- 4 x 96 B (fused), 6 x 96 B (unfused), 6 x 192 B (fp64)
    per site, shift and flavour, the shared r not counted -- against a copy of an fp64 field (tmhip_assign, 2 x 192 B/site) from the same run;
(b) a whole iteration at 12 shifts, both forms, against one of cg_mms_tm_nd;
(c) (median of max(3, reps / 2)) a solve on the shifts 0.01 + 0.1 k of tools/mms_speed.py: mixed_cg_mms_tm_nd to eps_sq = 1e-14 relative, then cg_mms_tm_nd to the
    true relative residual^2 the mixed solve reached on shift 0 (computed on the device in fp64), with iteration counts, reliable
    updates and removed shifts.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.83
K1, K2 = 4, 14
NP = 12


def timed(lat, fn, reps):
    """(median, min, max) of the time of one fn() in ms"""
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
    ap.add_argument("--out")
    a = ap.parse_args()
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ms = lambda r: "%9.3f ms  (%.3f .. %.3f)" % r
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.1373, mu=0.0035, theta=(1.0, 0.0, 0.0, 0.0))
        lat.set_gauge(syn.gauge_field(5, L, L, L, L))
        lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
        N = lat.Vh
        say("== %d^4, %d shifts, median of %d (min .. max), HIP events" % (L, NP, a.reps))
        src = [syn.spinor_field_eo(10 + i, 1, L, L, L, L) for i in range(2)]
        qu, qd, au, ad = lat.field(src[0]), lat.field(src[1]), lat.field(), lat.field()
        P = [(lat.field(), lat.field()) for _ in range(NP)]
        close = [0.01 + 0.001 * k for k in range(NP)]
        res = {}

        def mixed(K, n, shifts=close, eps=0.0):
            def run():
                res["it"], res["counts"], _ = lat.mixed_cg_mms_tm_nd(qu, qd, shifts[:n], K, eps, 1, P=P[:n])
            return run

        def fp64(K, n, shifts=close, eps=0.0):
            def run():
                res["it"], _ = lat.cg_mms_tm_nd(qu, qd, shifts[:n], K, eps, 1, P=P[:n])
            return run

        def per_iteration(mk, n):
            t1, t2 = timed(lat, mk(K1, n), a.reps), timed(lat, mk(K2, n), a.reps)
            return (t2[0] - t1[0]) / (K2 - K1), t1, t2
        copy = timed(lat, lambda: [lat.assign(au, qu, N) for _ in range(50)], a.reps)
        copy_bw = 50 * 2 * 192.0 * N / (copy[0] * 1e-3)
        say("    copy of an fp64 field (tmhip_assign)                : %8.1f us = %.2f TB/s" % (1e3 * copy[0] / 50, copy_bw / 1e12))
        it = {}
        updates = {}
        for fused in (0, 1):
            lat.set_option("mms32_fused", fused)
            for n in (1, NP):
                it[("mixed", fused, n)] = per_iteration(mixed, n)
                updates[(fused, n)] = res["counts"][0]
        lat.set_option("mms32_fused", 1)
        for n in (1, NP):
            it[("fp64", n)] = per_iteration(fp64, n)
        # ---- (a)
        vec64 = it[("fp64", NP)][0] - it[("fp64", 1)][0]
        bw64 = (NP - 1) * 2 * 6 * 192.0 * N / (vec64 * 1e-3)
        say("(a) vector part of %d shifts, cg_mms_tm_nd (fp64)          : %8.1f us = %.2f TB/s (%3.0f %% of the copy)"
            % (NP - 1, 1e3 * vec64, bw64 / 1e12, 100 * bw64 / copy_bw))
        for fused, passes in ((0, 6), (1, 4)):
            vec = it[("mixed", fused, NP)][0] - it[("mixed", fused, 1)][0]
            bw = (NP - 1) * 2 * passes * 96.0 * N / (vec * 1e-3)
            say("(a) vector part of %d shifts, mixed, mms32_fused %d        : %8.1f us = %.2f TB/s (%3.0f %% of the copy)   fp64 / this = %.2f   [reliable updates in the timing runs: %d]"
                % (NP - 1, fused, 1e3 * vec, bw / 1e12, 100 * bw / copy_bw, vec64 / vec, updates[(fused, NP)]))
        # ---- (b)
        t64 = it[("fp64", NP)]
        say("(b) iteration of cg_mms_tm_nd, %d shifts                   : %8.1f us   [%d its %s, %d its %s]" % (NP, 1e3 * t64[0], K1, ms(t64[1]), K2, ms(t64[2])))
        for fused in (0, 1):
            t = it[("mixed", fused, NP)]
            say("(b) iteration of mixed_cg_mms_tm_nd, mms32_fused %d        : %8.1f us   [%d its %s, %d its %s]   fp64 / this = %.2f"
                % (fused, 1e3 * t[0], K1, ms(t[1]), K2, ms(t[2]), t64[0] / t[0]))
        for n in (1,):
            say("(b) one shift: cg_mms_tm_nd %.1f us, mixed %.1f us (mms32_fused 0), %.1f us (mms32_fused 1)"
                % (1e3 * it[("fp64", n)][0], 1e3 * it[("mixed", 0, n)][0], 1e3 * it[("mixed", 1, n)][0]))
        # ---- (c)
        shifts = [0.01 + 0.1 * k for k in range(NP)]
        qnorm = lat.square_norm(qu, N) + lat.square_norm(qd, N)

        def true_residual0():
            lat.Qtm_pm_ndpsi(au, ad, P[0][0], P[0][1])
            lat.assign_add_mul_r(au, P[0][0], shifts[0] ** 2, N); lat.assign_add_mul_r(ad, P[0][1], shifts[0] ** 2, N)
            lat.diff(au, qu, au, N); lat.diff(ad, qd, ad, N)
            return (lat.square_norm(au, N) + lat.square_norm(ad, N)) / qnorm
        for fused in (0, 1):
            lat.set_option("mms32_fused", fused)
            tm = timed(lat, mixed(5000, NP, shifts, 1e-14), max(3, a.reps // 2))
            r0 = true_residual0()
            say("(c) mixed_cg_mms_tm_nd, eps_sq 1e-14 relative, mms32_fused %d : %s   %d iterations, %d reliable updates, %d shifts removed, true residual^2 of shift 0 %.2e"
                % (fused, ms(tm), res["it"], res["counts"][0], res["counts"][1], r0))
        t6 = timed(lat, fp64(5000, NP, shifts, r0), max(3, a.reps // 2))
        say("(c) cg_mms_tm_nd to that residual (eps_sq %.2e relative)   : %s   %d iterations, %d shifts left, true residual^2 of shift 0 %.2e   cg_mms_tm_nd / mixed = %.2f"
            % (r0, ms(t6), res["it"], lat.nd_active_shifts(), true_residual0(), t6[0] / tm[0]))
        lat.close()
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "mms32_" in l:
                say("(d) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
