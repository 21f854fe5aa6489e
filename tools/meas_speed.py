"""Speed of the online measurements on the device (meas.hip) on one MI355X (writes profiles/r13_meas_speed.log when given --out).

    python tools/meas_speed.py [--sizes 16 32] [--reps 7] [--out profiles/r13_meas_speed.log]

One child process per size, each under its own `timeout`; a size that fails ends the run.  Per L^4, warm-up call first, then the
median of `reps` timings with HIP events around the call (min .. max in brackets).  Every call includes its final pass, the copy of
its results and its one synchronisation.  No pass/fail threshold: the numbers are recorded.
  slice_correlators   dir 0 with pp, pa, p4 and dir 3 with pp alone, beside square_norm(even) + square_norm(odd) from the same run:
                      the same 192 B/site read (the slice sums do three times the accumulation and synchronise once instead of twice)
  oriented plaquettes beside measure_plaquette: the same loads and products, six sums instead of one
  polyakov_loop       dir 0 and dir 3: V / L threads of serial work over all 576 B/site of links, of which it uses a quarter"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBPS = 5.5


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


def child(L, reps):
    from tests.util import random_gauge, random_spinor
    from tmlqcd_amd import Lattice
    lat = Lattice(L, L, L, L, kappa=0.13, mu=0.01)
    V, Vh = lat.V, lat.Vh
    lat.set_gauge(random_gauge(1, V))
    fe, fo = lat.field(random_spinor(2, Vh)), lat.field(random_spinor(3, Vh))
    print("L=%d  V=%d  propagator %.0f MB, links %.0f MB" % (L, V, V * 192 / 1e6, V * 576 / 1e6), flush=True)
    rows = [("slice dir 0 pp pa p4", lambda: lat.slice_correlators(fe, fo, 0), 192),
            ("slice dir 0 pp", lambda: lat.slice_correlators(fe, fo, 0, pa_p4=False), 192),
            ("slice dir 3 pp", lambda: lat.slice_correlators(fe, fo, 3, pa_p4=False), 192),
            ("slice dir 3 pp pa p4", lambda: lat.slice_correlators(fe, fo, 3), 192),
            ("two square_norm", lambda: (lat.square_norm(fe, Vh), lat.square_norm(fo, Vh)), 192),
            ("oriented plaquettes", lat.measure_oriented_plaquettes, 576),
            ("measure_plaquette", lat.measure_plaquette, 576),
            ("polyakov_loop dir 0", lambda: lat.polyakov_loop(0), 144),
            ("polyakov_loop dir 3", lambda: lat.polyakov_loop(3), 144)]
    res = {}
    for name, fn, nbytes in rows:
        ms, lo, hi = timed(lat, fn, reps)
        res[name] = ms
        tb = nbytes * V / (ms * 1e-3) / 1e12
        print("  %-22s %9.4f ms  (%.4f .. %.4f)   unique %4d B/site -> %5.2f TB/s = %4.1f %% of the %.1f TB/s copy" % (
            name, ms, lo, hi, nbytes, tb, 100 * tb / COPY_TBPS, COPY_TBPS), flush=True)
    two = res["two square_norm"]
    for name in ("slice dir 0 pp pa p4", "slice dir 3 pp"):
        ratio = res[name] / two
        print("  %s / two square_norm = %.2f%s" % (name, ratio, "   ABOVE the expected 1.5" if ratio > 1.5 else ""), flush=True)
    print("  oriented plaquettes / measure_plaquette = %.2f" % (res["oriented plaquettes"] / res["measure_plaquette"]), flush=True)
    lat.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per size")
    ap.add_argument("--note", action="append", default=[], help="a line for the log's header")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return 0
    lines = ["# tools/meas_speed.py: HIP events around each call, warm, median of %d (min .. max); one process per size." % a.reps,
             "# Every call includes its final pass, the copy of its results and its one synchronisation.  unique = bytes a call must move at least once."]
    lines += ["# " + n for n in a.note]
    print("\n".join(lines), flush=True)
    rc = 0
    for L in a.sizes:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(L), "--reps", str(a.reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        lines.append(r.stdout.rstrip("\n"))
        if r.returncode != 0:
            lines.append("L=%d: exit status %d, stopping" % (L, r.returncode))
            print(lines[-1])
            rc = 1
            break
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
