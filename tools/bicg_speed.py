"""Timing of BiCGstab on the device (writes profiles/r16_bicg_speed.log when given --out).

    python tools/bicg_speed.py [--sizes 16 32] [--ops Mtm_plus_sym_psi D_psi] [--reps 7] [--out profiles/r16_bicg_speed.log]

Per size L^4 and operator, on the synthetic gauge field: (a) the whole solve (relative 1e-18) with bicg_fused 1 and 0 and its
iteration count, (b) K iterations cut by max_iter = K (K below the count of (a), so no stopping test fires) with bicg_fused 1 and 0,
per iteration -- the set-up of a solve (one operator application, four stream kernels, three sums) is in the figure, K times
diluted --, (c) 2 K operator applications alone, per pair, and what (b) leaves for the vector part, (d) the kernels' lines of the
build's resource table.  Every figure: warm-up call first, then the median of `reps` timings with the min .. max spread, taken with
HIP events around the call (the stream's time, host round trips included) and, in brackets, the host clock around the synchronised
call."""
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
    ap.add_argument("--ops", nargs="+", default=["Mtm_plus_sym_psi", "D_psi"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    fmt = lambda r, k=1: "%9.3f ms  (%.3f .. %.3f) [host %.3f]" % tuple(x / k for x in r)
    slower = []
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.125, mu=0.01)
        lat.set_gauge(syn.gauge_field(5, L, L, L, L))
        say("== %d^4, median of %d (min .. max), HIP events [host clock]" % (L, a.reps))
        for op in a.ops:
            full = op == "D_psi"
            N = lat.V if full else lat.Vh
            if full:
                import numpy as np
                src = np.concatenate([syn.spinor_field_eo(10, 1, L, L, L, L), syn.spinor_field_eo(11, 1, L, L, L, L)])
                q, x, y = lat.full_field(src), lat.full_field(), lat.full_field()
            else:
                q, x, y = lat.field(syn.spinor_field_eo(10, 1, L, L, L, L)), lat.field(), lat.field()
            its, whole, cut = {}, {}, {}
            for fused in (1, 0):
                lat.set_option("bicg_fused", fused)
                whole[fused] = timed(lat, lambda: its.__setitem__(fused, lat.bicgstab_complex(x, q, 5000, 1e-18, 1, N, op=op)[0]), a.reps, lambda: x.zero())
            K = max(1, min(20, its[1] - 1))
            for fused in (1, 0):
                lat.set_option("bicg_fused", fused)
                cut[fused] = timed(lat, lambda: lat.bicgstab_complex(x, q, K, 1e-18, 1, N, op=op), a.reps, lambda: x.zero())
            lat.set_option("bicg_fused", 1)

            def pairs():
                for _ in range(K):
                    lat.D_psi(y, q) if full else lat.op(op, y, q)
                    lat.D_psi(x, y) if full else lat.op(op, x, y)
            ops = timed(lat, pairs, a.reps)
            say("(a) %-17s solve, bicg_fused 1 : %s   %d iterations" % (op, fmt(whole[1]), its[1]))
            say("    %-17s solve, bicg_fused 0 : %s   %d iterations; singles / fused %.2f" % (op, fmt(whole[0]), its[0], whole[0][0] / whole[1][0]))
            say("(b) %-17s iteration, fused 1  : %s   (%d iterations / %d)" % (op, fmt(cut[1], K), K, K))
            say("    %-17s iteration, fused 0  : %s   singles / fused %.2f" % (op, fmt(cut[0], K), cut[0][0] / cut[1][0]))
            say("(c) %-17s two applications    : %s   vector part: fused %.3f ms, singles %.3f ms, ratio %.2f" %
                (op, fmt(ops, K), (cut[1][0] - ops[0]) / K, (cut[0][0] - ops[0]) / K, (cut[0][0] - ops[0]) / max(cut[1][0] - ops[0], 1e-9)))
            if whole[1][0] > whole[0][0] or cut[1][0] > cut[0][0]:
                slower.append((L, op))
        lat.close()
    say("fused path slower than the singles at: %s" % (slower if slower else "no measured point"))
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "bicghip::" in l or "cplx3_kernel" in l:
                say("(d) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
