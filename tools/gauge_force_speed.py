"""Speed of the gauge monomial on the device (gauge.hip) on one MI355X: device events, warm, one process.

    python tools/gauge_force_speed.py [--sizes 16 32] [--reps 20] [--bench-json BENCH.json]

Per L^4: the plaquette force, the plaquette + rectangle force, measure_plaquette / measure_gauge_action / measure_rectangles (each
includes its final reduction and the 8-byte result copy), and in the same run tmhip_update_gauge, tmhip_sw_all (a plaquette-leaf
kernel of comparable shape) and tmhip_gauge_download of the full field -- the transfer a host-side gauge monomial pays before any
CPU work, which is the yardstick.  Next to every kernel: its unique bytes (576 B/site of links + 512 B/site of derivative read and
written for a force, 576 B/site for a measure) over the measured time, against a linalg stream kernel measured here
(assign_add_mul_r, 576 B/site) and, with --bench-json, the copy rate of roofline.measured_stream in that bench.py record.
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import random_gauge, random_spinor   # noqa: E402
from tmlqcd_amd import Lattice                        # noqa: E402

C1 = -0.331
IWASAKI = dict(c0=1.0 - 8.0 * C1, c1=C1, use_rectangles=True)


def device_ms(lat, fn, reps):
    fn()
    lat.sync()
    lat.event_record(0)
    for _ in range(reps):
        fn()
    lat.event_record(1)
    lat.sync()
    return lat.event_elapsed_ms(0, 1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bench-json")
    a = ap.parse_args()
    copy = None
    if a.bench_json:
        m = re.findall(r'copy_GBps\\?":\s*([0-9.eE+-]+)', open(a.bench_json).read())   # (also inside a quoted log line of the record)
        copy = float(m[-1]) if m else None
    print("# tools/gauge_force_speed.py: device events, warm, %d calls per figure; gauge_download by the host clock, best of 3." % a.reps)
    print("# Yardstick: what a host-side gauge monomial pays per call before any CPU work -- the download of the links.")
    print("# unique = bytes a call must move at least once (links in; derivative read and written).  The gathered re-reads of the links")
    print("# are expected to be served by L2 / Infinity Cache; no counter run in this log measures that.")
    if a.bench_json:
        print("# bench.py copy = copy_GBps of roofline.measured_stream in %s%s" % (os.path.basename(a.bench_json), "" if copy else ": NOT FOUND"))
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.13, mu=0.01)
        V = lat.V
        lat.set_gauge(random_gauge(1, V))
        lat.momenta_upload(np.random.default_rng(2).standard_normal((V, 4, 8)) * 1e-3)
        x, y = lat.field(random_spinor(3, lat.Vh)), lat.field(random_spinor(4, lat.Vh))
        lat.derivative_zero()
        lat.sw_term(None, 0.13, 1.5)
        lat.swpm_zero()
        rows = [("plaquette force", lambda: lat.gauge_derivative(5.6), 1088),
                ("plaquette + rectangle force", lambda: lat.gauge_derivative(5.6, **IWASAKI), 1088),
                ("measure_plaquette", lat.measure_plaquette, 576),
                ("measure_gauge_action", lambda: lat.measure_gauge_action(0.3), 576),
                ("measure_rectangles", lat.measure_rectangles, 576),
                ("update_gauge", lambda: lat.update_gauge(1e-6), None),
                ("sw_all", lambda: lat.sw_all(0.13, 1.5), None)]
        stream = device_ms(lat, lambda: lat.assign_add_mul_r(x, y, 1e-9, lat.Vh), 50)
        bw_stream = 576.0 * lat.Vh / (stream * 1e-3) / 1e9
        print("L=%d  V=%d  linalg stream %.0f GB/s%s" % (L, V, bw_stream, "  bench.py copy %.0f GB/s" % copy if copy else ""), flush=True)
        res = {}
        for name, fn, bytes_per_site in rows:
            ms = device_ms(lat, fn, a.reps)
            res[name] = ms
            if bytes_per_site:
                bw = bytes_per_site * V / (ms * 1e-3) / 1e9
                print("  %-28s %9.3f ms   unique %4d B/site -> %7.0f GB/s = %4.1f %% of the linalg stream%s" % (
                    name, ms, bytes_per_site, bw, 100 * bw / bw_stream, ", %4.1f %% of the bench.py copy" % (100 * bw / copy) if copy else ""), flush=True)
            else:
                print("  %-28s %9.3f ms" % (name, ms), flush=True)
        lat.gauge_download()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            lat.gauge_download()
            t.append(time.perf_counter() - t0)
        dl = 1e3 * min(t)
        print("  %-28s %9.3f ms   (%.0f MB device -> host, best of 3, host clock)" % ("gauge_download", dl, V * 576 / 1e6), flush=True)
        for name in ("plaquette force", "plaquette + rectangle force"):
            print("  %s / gauge_download = %.3f  -> %s" % (name, res[name] / dl, "faster than the download alone" if res[name] < dl else "SLOWER than the download"), flush=True)
        lat.close()


if __name__ == "__main__":
    main()
