"""Speed of the fp32 doublet and of rg_mixed_cg_her_nd on one MI355X (writes profiles/r20_nd32_speed.log when given --out).

    python tools/nd32_speed.py [--sizes 16 32] [--reps 7] [--calls 50] [--out profiles/r20_nd32_speed.log]

Per size L^4, on the synthetic gauge field, in one process; every figure is the median of --reps timings (min .. max) with HIP
events around the calls, after a warm-up:
(a) us per Qtm_pm_ndpsi_32 with the doublet stencil ("nd_fused" 1, 4 launches) and from two Hopping_Matrix_32 per hop plus a mixing
    kernel ("nd_fused" 0, 12 launches), next to the fp64 Qtm_pm_ndpsi and to 2 x Qtm_pm_psi_32, the single-flavour fp32 operator
    applied to both flavours; a timing is --calls calls between two events;
(b) one CG iteration on the doublet in fp32 and in fp64: the fp32 inner loop of rg_mixed_cg_her_nd and cg_her_nd, each run for K2 and
    for K1 iterations with unreachable targets, (t(K2) - t(K1)) / (K2 - K1), so that the start-up of a solve cancels;
(c) rg_mixed_cg_her_nd at delta 1e-1, 1e-3, 1e-5 and cg_her_nd to eps_sq = 1e-20 relative, with the iteration counts and the true
    relative residual^2 |Q - A x|^2 / |Q|^2 each reached (computed on the device in fp64).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MUBAR, EPSBAR, INVMAXEV = 0.1375, 0.1175, 0.83
K1, K2 = 20, 60


def timed(lat, fn, reps, calls=1):
    """(median, min, max) of the time of one fn() in ms"""
    fn(); lat.sync()
    ev = []
    for _ in range(reps):
        lat.sync()
        lat.event_record(0)
        for _ in range(calls):
            fn()
        lat.event_record(1)
        lat.sync()
        ev.append(lat.event_elapsed_ms(0, 1) / calls)
    return statistics.median(ev), min(ev), max(ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    us = lambda r: "%8.1f us  (%.1f .. %.1f)" % tuple(1e3 * x for x in r)
    ms = lambda r: "%9.3f ms  (%.3f .. %.3f)" % r
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.1373, mu=0.0035, theta=(1.0, 0.0, 0.0, 0.0))
        lat.set_gauge(syn.gauge_field(5, L, L, L, L))
        lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
        N = lat.Vh
        say("== %d^4, median of %d (min .. max), HIP events" % (L, a.reps))
        src = [syn.spinor_field_eo(10 + i, 1, L, L, L, L) for i in range(2)]
        qu, qd, pu, pd, au, ad = lat.field(src[0]), lat.field(src[1]), lat.field(), lat.field(), lat.field(), lat.field()
        k32 = lat.field32(), lat.field32()
        l32 = lat.field32(), lat.field32()
        lat.assign_to_32(k32[0], qu, N); lat.assign_to_32(k32[1], qd, N)
        # ---- (a)
        op = {}
        for fused in (1, 0):
            lat.set_option("nd_fused", fused)
            op[fused] = timed(lat, lambda: lat.Qtm_pm_ndpsi_32(l32[0], l32[1], k32[0], k32[1]), a.reps, a.calls)
        lat.set_option("nd_fused", 1)
        op64 = timed(lat, lambda: lat.Qtm_pm_ndpsi(au, ad, qu, qd), a.reps, a.calls)

        def two_single():
            lat.Qtm_pm_psi_32(l32[0], k32[0])
            lat.Qtm_pm_psi_32(l32[1], k32[1])
        op2 = timed(lat, two_single, a.reps, a.calls)
        say("(a) Qtm_pm_ndpsi_32, nd_fused 1 (doublet stencil)       : %s" % us(op[1]))
        say("(a) Qtm_pm_ndpsi_32, nd_fused 0 (two stencils + mixing) : %s   nd_fused 0 / nd_fused 1 = %.2f" % (us(op[0]), op[0][0] / op[1][0]))
        say("(a) Qtm_pm_ndpsi (fp64, nd_fused 1)                     : %s   fp64 / fp32 = %.2f" % (us(op64), op64[0] / op[1][0]))
        say("(a) 2 x Qtm_pm_psi_32                                   : %s   2 x single / doublet = %.2f" % (us(op2), op2[0] / op[1][0]))
        # ---- (b)
        def sp(K):
            return lambda: lat.rg_mixed_cg_her_nd(pu, pd, qu, qd, K, 1e-30, 1, N, delta=1e-30)

        def dp(K):
            def run():
                pu.zero(); pd.zero()
                lat.cg_her_nd(pu, pd, qu, qd, K, 1e-30, 1, N)
            return run
        t = {(name, K): timed(lat, mk(K), a.reps) for name, mk in (("sp", sp), ("dp", dp)) for K in (K1, K2)}
        it32 = (t[("sp", K2)][0] - t[("sp", K1)][0]) / (K2 - K1)
        it64 = (t[("dp", K2)][0] - t[("dp", K1)][0]) / (K2 - K1)
        say("(b) fp32 doublet CG iteration (inner loop of rg_mixed_cg_her_nd) : %8.1f us   [%d its %s, %d its %s]"
            % (1e3 * it32, K1 + 1, ms(t[("sp", K1)]), K2 + 1, ms(t[("sp", K2)])))
        say("(b) fp64 doublet CG iteration (cg_her_nd)                        : %8.1f us   [%d its %s, %d its %s]   fp64 / fp32 = %.2f"
            % (1e3 * it64, K1, ms(t[("dp", K1)]), K2, ms(t[("dp", K2)]), it64 / it32))
        # ---- (c)
        qnorm = lat.square_norm(qu, N) + lat.square_norm(qd, N)

        def true_residual():
            lat.Qtm_pm_ndpsi(au, ad, pu, pd)
            lat.diff(au, qu, au, N); lat.diff(ad, qd, ad, N)
            return (lat.square_norm(au, N) + lat.square_norm(ad, N)) / qnorm
        res = {}

        def her():
            pu.zero(); pd.zero()
            res["it"] = lat.cg_her_nd(pu, pd, qu, qd, 5000, 1e-20, 1, N)
        th = timed(lat, her, a.reps)
        say("(c) cg_her_nd, eps_sq 1e-20 relative             : %s   %d iterations, true residual^2 %.2e" % (ms(th), res["it"], true_residual()))
        for delta in (1e-1, 1e-3, 1e-5):
            def rg():
                res["it"], res["counts"] = lat.rg_mixed_cg_her_nd(pu, pd, qu, qd, 5000, 1e-20, 1, N, delta=delta)
            tr = timed(lat, rg, a.reps)
            say("(c) rg_mixed_cg_her_nd, delta %-5g               : %s   %d = %d + %d + %d iterations, true residual^2 %.2e, cg_her_nd / rg_mixed = %.2f"
                % (delta, ms(tr), res["it"], res["counts"][0], res["counts"][1], res["counts"][2], true_residual(), th[0] / tr[0]))
        lat.close()
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "nd32_" in l:
                say("(d) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
