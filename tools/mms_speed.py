"""Speed of the single-flavour multi-shift CG (tmhip_cg_mms_tm, mms.hip) on one MI355X, in one process, interleaved.

    python tools/mms_speed.py [--sizes 16 32] [--shifts 1 4 12 24] [--iters 100] [--reps 3] [--out profiles/r06_mms_speed.json]

For every L^4 and shift count: microseconds per iteration of cg_mms_tm on Qtm_pm_psi (eps_sq = 0, a fixed iteration count, so
no shift is dropped and nothing converges), cg_her on the same operator as the yardstick, and the per-shift share of the vector
pass -- (t(n shifts) - t(1 shift)) / (n - 1), 768 B/site per shift -- against the bandwidth of a linalg stream kernel
(assign_add_mul_r: 576 B/site) measured in the same process.  Every row is the median of --reps interleaved repetitions.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import random_gauge, random_spinor   # noqa: E402
from tmlqcd_amd import Lattice                        # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--shifts", type=int, nargs="+", default=[1, 4, 12, 24])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.13, mu=0.01)
        lat.set_gauge(random_gauge(1, lat.VPR))
        q = lat.field(random_spinor(2, lat.Vh))
        x, y = lat.field(random_spinor(3, lat.Vh)), lat.field(random_spinor(4, lat.Vh))
        pools = {n: [lat.field() for _ in range(n)] for n in a.shifts}
        shifts = {n: [0.01 + 0.1 * k for k in range(n)] for n in a.shifts}
        K = a.iters
        # warm-up of every kernel involved
        lat.cg_mms_tm(q, shifts[max(a.shifts)], 5, 0.0, 0, P=pools[max(a.shifts)])
        lat.cg_her(lat.field(), q, 5, 0.0, 0, lat.Vh)
        meas = {("mms", n): [] for n in a.shifts}
        meas["her"], meas["stream"] = [], []
        for _ in range(a.reps):
            for n in a.shifts:
                meas[("mms", n)].append(timed(lambda: lat.cg_mms_tm(q, shifts[n], K, 0.0, 0, P=pools[n])) / K)
            p = lat.field()
            meas["her"].append(timed(lambda: (lat.cg_her(p, q, K, 0.0, 0, lat.Vh))) / K)
            lat.sync()

            def stream():
                for _ in range(50):
                    lat.assign_add_mul_r(x, y, 1e-9, lat.Vh)
                lat.sync()
            meas["stream"].append(timed(stream) / 50)
        med = {k: float(np.median(v)) for k, v in meas.items()}
        bw_stream = 576.0 * lat.Vh / med["stream"] / 1e12
        base = med[("mms", a.shifts[0])]
        for n in a.shifts:
            t = med[("mms", n)]
            per_shift = (t - base) / (n - a.shifts[0]) if n > a.shifts[0] else None
            bw_shift = 768.0 * lat.Vh / per_shift / 1e12 if per_shift else None
            row = {"L": L, "shifts": n, "us_per_iter": t * 1e6, "cg_her_us_per_iter": med["her"] * 1e6,
                   "ratio_to_cg_her": t / med["her"], "per_shift_us": per_shift * 1e6 if per_shift else None,
                   "per_shift_TBps": bw_shift, "stream_TBps": bw_stream,
                   "per_shift_vs_stream": bw_shift / bw_stream if bw_shift else None}
            rows.append(row)
            print("L=%2d shifts=%2d  %8.1f us/iter  cg_her %7.1f us/iter  x%.2f   per shift %s   stream %.2f TB/s" % (
                L, n, row["us_per_iter"], row["cg_her_us_per_iter"], row["ratio_to_cg_her"],
                "%.1f us = %.2f TB/s (%.0f %% of stream)" % (row["per_shift_us"], bw_shift, 100 * row["per_shift_vs_stream"]) if per_shift else "-",
                bw_stream), flush=True)
        lat.close()
    if a.out:
        json.dump({"iters": a.iters, "reps": a.reps, "rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
