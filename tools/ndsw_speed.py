"""Timing of the clover doublet on the device (writes profiles/r09_ndsw_speed.log when given --out).

    python tools/ndsw_speed.py [--sizes 16 32] [--np 12] [--reps 9] [--out profiles/r09_ndsw_speed.log]

All variants of a group are timed INTERLEAVED in one process: every repetition runs one batch of `calls` calls of each variant in
turn (host clock around a synchronised batch), and the figure is the median over the repetitions with the min .. max spread.
Per size L^4:
 (a) Qsw_pm_ndpsi with "nd_fused" 1 / 0, two Qsw_pm_psi (the yardstick of the twisted-mass doublet) and Qtm_pm_ndpsi, us per call;
 (b) cg_her_nd_op iterations per second on both operators (a fixed number of iterations: rel_prec 2 never converges);
 (c) cg_mms_tm_nd_op per iteration at 1 / 4 / 12 shifts on the clover operator;
 (d) sw_invert_nd and sw_deriv_nd;
 (e) ndcloverrat_force at np shifts with "rat_batch" 1 / np, and its parts: the 4 np sw_spinor_eo launches, the 2 deriv_Sb_batch launches
     per group, sw_all;
 (f) ndcloverrat_derivative (solve + force);
 (g) the new kernels' lines of the build's resource table.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def interleaved(lat, variants, reps, calls):
    """variants: {name: (prepare or None, fn)} -> {name: (median, min, max)} in us per call"""
    for prep, fn in variants.values():
        if prep:
            prep()
        fn(); lat.sync()
    ts = {k: [] for k in variants}
    for _ in range(reps):
        for k, (prep, fn) in variants.items():
            if prep:
                prep()
            fn(); lat.sync()                       # first call after a switch of options is not timed
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            lat.sync()
            ts[k].append((time.perf_counter() - t0) * 1e6 / calls)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--np", type=int, default=12)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda r: "%10.1f us  (%.1f .. %.1f)" % r
    np_ = a.np
    kappa, c_sw, mb, eb, inv = 0.125, 1.2, 0.12, 0.1, 0.6
    mu = [0.02 * 1.6 ** j for j in range(np_)]
    rmu = [0.01 * 1.5 ** j for j in range(np_)]
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=kappa, mu=mb)
        g = syn.gauge_field(5, L, L, L, L)
        lat.set_gauge(g)
        lat.set_nd(mb, eb, inv)
        lat.sw_term(g, kappa, c_sw)
        lat.sw_invert(0, mb)
        lat.sw_invert_nd(mb * mb - eb * eb)
        assert lat.sw_invert_failures() == 0
        say("== %d^4, median of %d interleaved repetitions (min .. max)" % (L, a.reps))
        ks, kc = lat.field(syn.spinor_field_eo(10, 1, L, L, L, L)), lat.field(syn.spinor_field_eo(11, 1, L, L, L, L))
        ls, lc = lat.field(), lat.field()
        calls = 40 if L <= 16 else 12
        fused = lambda v: (lambda: lat.set_option("nd_fused", v))
        r = interleaved(lat, {
            "Qsw_pm_ndpsi fused": (fused(1), lambda: lat.Qsw_pm_ndpsi(ls, lc, ks, kc)),
            "Qsw_pm_ndpsi plain": (fused(0), lambda: lat.Qsw_pm_ndpsi(ls, lc, ks, kc)),
            "2 x Qsw_pm_psi": (None, lambda: (lat.op("Qsw_pm_psi", ls, ks), lat.op("Qsw_pm_psi", lc, kc))),
            "Qtm_pm_ndpsi fused": (fused(1), lambda: lat.Qtm_pm_ndpsi(ls, lc, ks, kc)),
            "Qtm_pm_ndpsi plain": (fused(0), lambda: lat.Qtm_pm_ndpsi(ls, lc, ks, kc)),
        }, a.reps, calls)
        for k, v in r.items():
            say("(a) %-22s : %s" % (k, fmt(v)))
        say("    fused / plain %.3f   clover doublet / two single-flavour %.3f   clover / twisted-mass doublet %.3f"
            % (r["Qsw_pm_ndpsi fused"][0] / r["Qsw_pm_ndpsi plain"][0], r["Qsw_pm_ndpsi fused"][0] / r["2 x Qsw_pm_psi"][0],
               r["Qsw_pm_ndpsi fused"][0] / r["Qtm_pm_ndpsi fused"][0]))
        best = 1 if r["Qsw_pm_ndpsi fused"][0] <= r["Qsw_pm_ndpsi plain"][0] else 0
        # (b) a fixed number of CG iterations
        iters = 100
        pu, pd = lat.field(), lat.field()

        def her(op):
            pu.zero(); pd.zero()
            lat.cg_her_nd(pu, pd, ks, kc, iters, 1e-30, 2, lat.Vh, op=op)
        r = interleaved(lat, {"cg_her_nd Qsw_pm_ndpsi fused": (fused(1), lambda: her("Qsw_pm_ndpsi")),
                              "cg_her_nd Qsw_pm_ndpsi plain": (fused(0), lambda: her("Qsw_pm_ndpsi")),
                              "cg_her_nd Qtm_pm_ndpsi fused": (fused(1), lambda: her("Qtm_pm_ndpsi"))}, max(3, a.reps // 2), 1)
        for k, v in r.items():
            say("(b) %-28s : %8.0f iterations/s  (%s per %d iterations)" % (k, iters * 1e6 / v[0], fmt(v), iters))
        lat.set_option("nd_fused", best)
        # (c) multi-shift CG per iteration
        P = [(lat.field(), lat.field()) for _ in range(np_)]
        for ns in (1, 4, 12):
            ns = min(ns, np_)
            v = interleaved(lat, {"x": (None, lambda: lat.cg_mms_tm_nd(ks, kc, mu[:ns], iters, 1e-30, -1, P=P[:ns], op="Qsw_pm_ndpsi"))}, max(3, a.reps // 2), 1)["x"]
            say("(c) cg_mms_tm_nd_op, %2d shifts, nd_fused %d : %8.1f us per iteration  (%s per %d iterations)" % (ns, best, v[0] / iters, fmt(v), iters))
        # (d)
        lat.swpm_zero()
        r = interleaved(lat, {"sw_invert_nd": (None, lambda: lat.sw_invert_nd(mb * mb - eb * eb)), "sw_deriv_nd": (None, lambda: lat.sw_deriv_nd(0)),
                              "sw_invert (cloverdet's)": (None, lambda: lat.sw_invert(0, mb)), "sw_deriv (cloverdet's)": (None, lambda: lat.sw_deriv(0, mb))}, a.reps, 5)
        for k, v in r.items():
            say("(d) %-24s : %s" % (k, fmt(v)))
        # (e) the force and its parts
        chi = [(lat.field(syn.spinor_field_eo(20 + j, 1, L, L, L, L)), lat.field(syn.spinor_field_eo(60 + j, 1, L, L, L, L))) for j in range(np_)]
        lat.derivative_zero()
        batch = lambda v: (lambda: lat.set_option("rat_batch", v))
        fl = [c[0] for c in chi] + [c[1] for c in chi]
        fk = fl[1:] + fl[:1]
        r = interleaved(lat, {
            "ndcloverrat_force rat_batch 1": (batch(1), lambda: lat.ndcloverrat_force(chi, mu, rmu, inv, kappa, c_sw, 1)),
            "ndcloverrat_force rat_batch %d" % np_: (batch(np_), lambda: lat.ndcloverrat_force(chi, mu, rmu, inv, kappa, c_sw, 1)),
            "ndrat_force rat_batch %d" % np_: (batch(np_), lambda: lat.ndrat_force(chi, mu, rmu, inv)),
            "%d x sw_spinor_eo" % (4 * np_): (None, lambda: [lat.sw_spinor_eo(q & 1, chi[j][0], chi[j][1], 0.1) for j in range(np_) for q in range(4)]),
            "2 x deriv_Sb_batch (%d pairs)" % (2 * np_): (None, lambda: (lat.deriv_Sb_batch(0, fl, fk, rmu + rmu), lat.deriv_Sb_batch(1, fl, fk, rmu + rmu))),
            "sw_all": (None, lambda: lat.sw_all(kappa, c_sw)),
        }, max(3, a.reps // 2), 2)
        for k, v in r.items():
            say("(e) %-32s : %s" % (k, fmt(v)))
        tot = r["ndcloverrat_force rat_batch %d" % np_][0]
        say("    shares of ndcloverrat_force at rat_batch %d: sw_spinor_eo %.1f %%, deriv_Sb_batch %.1f %%, sw_all %.1f %%"
            % (np_, 100 * r["%d x sw_spinor_eo" % (4 * np_)][0] / tot, 100 * r["2 x deriv_Sb_batch (%d pairs)" % (2 * np_)][0] / tot, 100 * r["sw_all"][0] / tot))
        # (f)
        lat.set_option("rat_batch", np_)
        its = []
        v = interleaved(lat, {"x": (None, lambda: its.append(lat.ndcloverrat_derivative(ks, kc, mu, rmu, inv, kappa, c_sw, 1, 5000, 1e-16, 1)))}, 3, 1)["x"]
        say("(f) ndcloverrat_derivative, np = %d         : %s   (%d iterations)" % (np_, fmt(v), its[-1]))
        lat.set_option("nd_fused", 1)
        lat.close()
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "ndsw_" in l or "sw_invert_nd" in l or "sw_deriv_nd" in l:
                if ", true>" in l:
                    continue
                say("(g) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
