"""Speed of the non-degenerate doublet on one MI355X, at 16^4 and 32^4 ("Doublet").

For each lattice, interleaved in one process, `rounds` times:
  * us per Qtm_pm_ndpsi with the doublet stencil (option nd_fused 1, the default) -- 4 launches;
  * the same operator from two single-flavour stencils per hop plus a mixing pass (nd_fused 0) -- 12 launches;
  * 2 x Qtm_pm_psi, the single-flavour operator applied to both flavours (the yardstick);
and then cg_her_nd iterations per second (both forms; 300 iterations with eps_sq = 0) next to cg_her on Qtm_pm_psi, which
iterates ONE flavour (the doublet's yardstick is half its rate).  Medians are printed as a table and written as JSON to --out.

    python tools/nd_speed.py [--sizes 16 32] [--reps 200] [--rounds 5] [--out nd_speed.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(lat, fn, reps):
    fn()
    lat.sync()
    lat.event_record(0)
    for _ in range(reps):
        fn()
    lat.event_record(1)
    lat.sync()
    return 1e3 * lat.event_elapsed_ms(0, 1) / reps   # us per call


def cg_rate(lat, fn, iters):
    """iterations per second of a solve with eps_sq = 0 (it runs max_iter iterations unless the iterated residual reaches exactly
    zero); the rate is taken over the iterations the solver reports, so an early stop cannot inflate it"""
    fn(iters)   # warm-up (allocations, first launches)
    lat.sync()
    t0 = time.perf_counter()
    it = fn(iters)
    lat.sync()
    return (it if it > 0 else iters) / (time.perf_counter() - t0)


def one_size(L, reps, rounds):
    from tests.util import random_gauge, random_spinor
    from tmlqcd_amd import Lattice
    lat = Lattice(L, L, L, L, kappa=0.1373, mu=0.0035, theta=(1.0, 0.0, 0.0, 0.0))
    lat.set_gauge(random_gauge(11, L ** 4))
    lat.set_nd(0.1375, 0.1175, 0.83)
    N = lat.Vh
    ks, kc = lat.field(random_spinor(1, N)), lat.field(random_spinor(2, N))
    ls, lc = lat.field(), lat.field()

    def nd(fused):
        def f():
            lat.Qtm_pm_ndpsi(ls, lc, ks, kc)
        return lambda: (lat.set_option("nd_fused", fused), timed(lat, f, reps))[1]

    def two_single():
        def f():
            lat.Qtm_pm_psi(ls, ks)
            lat.Qtm_pm_psi(lc, kc)
        return timed(lat, f, reps)

    rows = {"doublet": [], "two_stencils": [], "2x_Qtm_pm_psi": []}
    for _ in range(rounds):
        rows["doublet"].append(nd(1)())
        rows["two_stencils"].append(nd(0)())
        rows["2x_Qtm_pm_psi"].append(two_single())
    res = {"L": L, "us_per_call": {k: float(np.median(v)) for k, v in rows.items()}, "samples": rows}
    pu, pd = lat.field(), lat.field()

    def her_nd(fused):
        def run(iters):
            lat.set_option("nd_fused", fused)
            pu.zero(); pd.zero()
            return lat.cg_her_nd(pu, pd, ks, kc, iters, 0.0, 0, N)
        return run

    def her(iters):
        pu.zero()
        return lat.cg_her(pu, ks, iters, 0.0, 0, N)[0]

    res["cg_iters_per_s"] = {"cg_her_nd_doublet": cg_rate(lat, her_nd(1), 300), "cg_her_nd_two_stencils": cg_rate(lat, her_nd(0), 300),
                             "cg_her_Qtm_pm_psi": cg_rate(lat, her, 300)}
    lat.set_option("nd_fused", 1)
    lat.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="JSON file for the full results (default: table only)")
    a = ap.parse_args()
    out = [one_size(L, a.reps, a.rounds) for L in a.sizes]
    print("%5s %14s %14s %16s %14s %14s %12s" % ("L", "doublet us", "2-stencil us", "2xQtm_pm_psi us", "her_nd it/s", "her_nd(2st)", "cg_her it/s"))
    for r in out:
        u, c = r["us_per_call"], r["cg_iters_per_s"]
        print("%5d %14.1f %14.1f %16.1f %14.0f %14.0f %12.0f" % (r["L"], u["doublet"], u["two_stencils"], u["2x_Qtm_pm_psi"],
                                                               c["cg_her_nd_doublet"], c["cg_her_nd_two_stencils"], c["cg_her_Qtm_pm_psi"]))
    if a.out:
        d = os.path.dirname(os.path.abspath(a.out))
        os.makedirs(d, exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
