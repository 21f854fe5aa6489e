"""Timing of the batched sw_spinor_eo, the clover rational forces and the tr-log energies on the device (writes
profiles/r10_cloverrat_speed.log when given --out).

    python tools/cloverrat_speed.py [--sizes 16 32] [--np 12] [--reps 9] [--out profiles/r10_cloverrat_speed.log]

Device events around a batch of `calls` calls on the context's stream; all variants of a group are timed INTERLEAVED in one process:
every repetition runs one warm-up call and one timed batch of each variant in turn, and the figure is the median over the repetitions
with the min .. max spread.  The two calls that end in a host read (sw_trace, get_clover + numpy) are timed with the host clock
around the synchronised call instead, and say so.
Per size L^4:
 (i)   sw_spinor_eo_batch with 2 np pairs against 2 np launches of the per-call kernel (the kernel of the parent commit, unchanged), with
       the bytes each form moves per site and the rate that makes;
 (ii)  ndcloverrat_force at np shifts with "rat_batch" 1 (the per-call path) and np;
 (iii) cloverrat_force with "rat_batch" 1 and np, and cloverrat_derivative (solve + force);
 (iv)  sw_trace and sw_trace_nd against get_clover + the host evaluation (numpy.linalg.slogdet on the even sites' blocks);
 (v)   the new kernels' lines of the build's resource table.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def interleaved(lat, variants, reps, calls, host_clock=False):
    """variants: {name: (prepare or None, fn)} -> {name: (median, min, max)} in us per call"""
    ts = {k: [] for k in variants}
    for rep in range(reps + 1):                    # repetition 0 is the warm-up of every variant
        for k, (prep, fn) in variants.items():
            if prep:
                prep()
            fn(); lat.sync()                       # first call after a switch of options is not timed
            if host_clock:
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                lat.sync()
                us = (time.perf_counter() - t0) * 1e6 / calls
            else:
                lat.event_record(0)
                for _ in range(calls):
                    fn()
                lat.event_record(1)
                lat.sync()
                us = lat.event_elapsed_ms(0, 1) * 1e3 / calls
            if rep:
                ts[k].append(us)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def host_trlog(lat, even, mu, shift):
    """what a host program does today: the clover term over PCIe, then the 6x6 determinants of the even sites in numpy"""
    swh, _ = lat.get_clover(True, False)
    b = (swh[..., 0] + 1j * swh[..., 1])[even]
    tot = 0.0
    for i in range(2):
        a = np.zeros((b.shape[0], 6, 6), dtype=complex)
        a[:, :3, :3] = b[:, 0, i]; a[:, :3, 3:] = b[:, 1, i]
        a[:, 3:, :3] = np.conj(np.transpose(b[:, 1, i], (0, 2, 1))); a[:, 3:, 3:] = b[:, 2, i]
        m = a + 1j * mu * np.eye(6) if shift is None else a @ a + shift * np.eye(6)
        tot += (2.0 if shift is None else 1.0) * np.linalg.slogdet(m)[1].sum()
    return tot


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
        lat = Lattice(L, L, L, L, kappa=kappa, mu=0.0)
        g = syn.gauge_field(5, L, L, L, L)
        lat.set_gauge(g)
        lat.set_nd(mb, eb, inv)
        lat.sw_term(g, kappa, c_sw)
        lat.sw_invert(0, 0.0)
        lat.sw_invert_nd(mb * mb - eb * eb)
        assert lat.sw_invert_failures() == 0
        say("== %d^4, np = %d, median of %d interleaved repetitions (min .. max), device events unless stated" % (L, np_, a.reps))
        chi = [(lat.field(syn.spinor_field_eo(20 + j, 1, L, L, L, L)), lat.field(syn.spinor_field_eo(60 + j, 1, L, L, L, L))) for j in range(np_)]
        fl = [c[0] for c in chi] + [c[1] for c in chi]
        fk = fl[1:] + fl[:1]
        fac = rmu + rmu
        n = 2 * np_
        lat.swpm_zero()
        calls = 10 if L <= 16 else 4
        # (i)
        r = interleaved(lat, {
            "sw_spinor_eo_batch, %d pairs" % n: (None, lambda: lat.sw_spinor_eo_batch(0, fl, fk, fac)),
            "%d x sw_spinor_eo" % n: (None, lambda: [lat.sw_spinor_eo(0, fl[j], fk[j], fac[j]) for j in range(n)]),
        }, a.reps, calls)
        sites = lat.Vh
        byt = {"sw_spinor_eo_batch, %d pairs" % n: n * 384 + 2304, "%d x sw_spinor_eo" % n: n * (384 + 2304)}   # every word once / per call
        for k, v in r.items():
            say("(i)   %-30s : %s   %6.1f kB per site if every word moves once, %.2f TB/s at that count"
                % (k, fmt(v), byt[k] / 1e3, byt[k] * sites / v[0] / 1e6))
        say("      per-call / batched %.2f" % (r["%d x sw_spinor_eo" % n][0] / r["sw_spinor_eo_batch, %d pairs" % n][0]))
        # (ii), (iii)
        lat.derivative_zero()
        batch = lambda v: (lambda: lat.set_option("rat_batch", v))
        single = [c[0] for c in chi]
        r = interleaved(lat, {
            "ndcloverrat_force rat_batch 1": (batch(1), lambda: lat.ndcloverrat_force(chi, mu, rmu, inv, kappa, c_sw, 1)),
            "ndcloverrat_force rat_batch %d" % np_: (batch(np_), lambda: lat.ndcloverrat_force(chi, mu, rmu, inv, kappa, c_sw, 1)),
            "cloverrat_force rat_batch 1": (batch(1), lambda: lat.cloverrat_force(single, rmu, kappa, c_sw, 1)),
            "cloverrat_force rat_batch %d" % np_: (batch(np_), lambda: lat.cloverrat_force(single, rmu, kappa, c_sw, 1)),
        }, max(3, a.reps // 2), 2)
        for k, v in r.items():
            say("(%s) %-32s : %s" % ("ii" if k.startswith("nd") else "iii", k, fmt(v)))
        say("      rat_batch 1 / %d: ndcloverrat_force %.3f, cloverrat_force %.3f"
            % (np_, r["ndcloverrat_force rat_batch 1"][0] / r["ndcloverrat_force rat_batch %d" % np_][0],
               r["cloverrat_force rat_batch 1"][0] / r["cloverrat_force rat_batch %d" % np_][0]))
        lat.set_option("rat_batch", np_)
        its = []
        pf = lat.field(syn.spinor_field_eo(10, 1, L, L, L, L))
        v = interleaved(lat, {"x": (None, lambda: its.append(lat.cloverrat_derivative(pf, mu, rmu, kappa, c_sw, 1, 5000, 1e-16, 1)))}, 3, 1, host_clock=True)["x"]
        say("(iii) cloverrat_derivative, np = %d, host clock : %s   (%d iterations)" % (np_, fmt(v), its[-1]))
        # (iv): both sides end in a host value, so the host clock around the whole call
        c = np.indices((L, L, L, L)).sum(axis=0).reshape(-1)
        even = (c & 1) == 0
        shift = mb * mb - eb * eb
        r = interleaved(lat, {
            "sw_trace(EE, mu)": (None, lambda: lat.sw_trace(0, mb)),
            "sw_trace_nd(EE, mubar, epsbar)": (None, lambda: lat.sw_trace_nd(0, mb, eb)),
            "get_clover + slogdet, sw_trace": (None, lambda: host_trlog(lat, even, mb, None)),
            "get_clover + slogdet, sw_trace_nd": (None, lambda: host_trlog(lat, even, mb, shift)),
        }, 3, 1, host_clock=True)
        for k, v in r.items():
            say("(iv)  %-34s : %s   host clock" % (k, fmt(v)))
        d, h = lat.sw_trace(0, mb), host_trlog(lat, even, mb, None)
        dn, hn = lat.sw_trace_nd(0, mb, eb), host_trlog(lat, even, mb, shift)
        say("      values: sw_trace %.15e (host %.15e), sw_trace_nd %.15e (host %.15e), failures %d" % (d, h, dn, hn, lat.sw_trace_failures()))
        lat.close()
    ru = os.path.join(ROOT, "tmlqcd_amd", "lib", "resource_usage.txt")
    if os.path.exists(ru):
        for l in open(ru):
            if l.startswith("kernel") or "sw_spinor_eo" in l or "sw_trace_kernel" in l:
                say("(v) " + " ".join(l.split()))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
