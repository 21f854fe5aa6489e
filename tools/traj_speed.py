"""Speed of the trajectory frame on the device (md_update.hip, trajectory.hip) on one MI355X: HIP events, warm, median of 7, one process.

    python tools/traj_speed.py [--sizes 16 32]

Per L^4, in one run:
 (a) each of the seven core calls (gauge_snapshot, gauge_restore, gauge_reunitarize, gauge_snapshot_diff, moment_energy,
     derivative_norms, gauge_snapshot_free by the host clock);
 (b) the two forms of the reject pass (device-to-device copy + re-sort against the re-sort that reads the snapshot) and of the accept
     pass (restoresu3 pass + re-sort against the fused LINKS_REUNIT form), through tmhip_bench_trajectory_forms;
 (c) the three reductions beside square_norm: bytes read per call over the time, and the ratio of the rates (a square_norm call reads
     192 bytes per site of ONE parity, so its fixed cost -- two launches and a synchronisation, as theirs -- weighs more);
 (d) what a linked program paid for the same step before: gauge_download + momenta_download + set_gauge (host clock, best of 3), and --
     where oracle/_ref/libtmtraj.so is present (tools/make_golden_traj.py --keep-lib) -- the reference's moment_energy and the three
     host loops of tools/traj_harness.c at 16^4.
The last lines compare the device's end-of-trajectory sequence (snapshot + 2 moment_energy + accept, or + reject) with (d)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import random_gauge, random_spinor   # noqa: E402
from tmlqcd_amd import Lattice                        # noqa: E402

REPS = 7


def device_ms(lat, fn):
    fn()
    t = []
    for _ in range(REPS):
        lat.sync()
        lat.event_record(0)
        fn()
        lat.event_record(1)
        lat.sync()
        t.append(lat.event_elapsed_ms(0, 1))
    return statistics.median(t)


def host_ms(fn, n=3):
    fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * min(t)


def reference_leg(L):
    """the reference's moment_energy and the harness's loops on host arrays, ms each; None if the libraries are not on this machine"""
    so = os.path.join(ROOT, "oracle", "_ref", "libtmtraj.so")
    if not os.path.exists(so):
        return None
    from oracle.refbind import RefLattice
    r = RefLattice(L, L, L, L, kappa=0.125, mu=0.0)
    tl = C.CDLL(so)
    vp = C.c_void_p
    tl.tmtraj_moment_energy.argtypes = [vp]
    tl.tmtraj_moment_energy.restype = C.c_double
    tl.tmtraj_gauge_diff.argtypes = [vp, vp]
    tl.tmtraj_gauge_diff.restype = C.c_double
    tl.tmtraj_snapshot.argtypes = [vp, vp]
    tl.tmtraj_restore.argtypes = [vp, vp]
    tl.tmtraj_reunitarize.argtypes = [vp]
    V = r.V
    g, tmp = random_gauge(1, V), np.zeros((V, 4, 3, 3, 2))
    mom = np.random.default_rng(2).standard_normal((V, 4, 8))
    hp = lambda a: a.ctypes.data_as(vp)
    return {"moment_energy": host_ms(lambda: tl.tmtraj_moment_energy(hp(mom))), "snapshot loop": host_ms(lambda: tl.tmtraj_snapshot(hp(tmp), hp(g))),
            "restore loop": host_ms(lambda: tl.tmtraj_restore(hp(g), hp(tmp))), "restoresu3 loop": host_ms(lambda: tl.tmtraj_reunitarize(hp(g))),
            "ddU loop": host_ms(lambda: tl.tmtraj_gauge_diff(hp(g), hp(tmp)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    a = ap.parse_args()
    print("# tools/traj_speed.py: HIP events around one call, warm, median of %d; host-clock figures best of 3." % REPS)
    for L in a.sizes:
        lat = Lattice(L, L, L, L, kappa=0.13, mu=0.01)
        V = lat.V
        g = random_gauge(1, V)
        mom = np.random.default_rng(2).standard_normal((V, 4, 8))
        lat.set_gauge(g)
        lat.momenta_upload(mom)
        lat.derivative_upload(np.random.default_rng(3).standard_normal((V, 4, 8)))
        x = lat.field(random_spinor(4, lat.Vh))
        print("L=%d  V=%d  links %.0f MB, momenta %.0f MB" % (L, V, V * 576 / 1e6, V * 256 / 1e6), flush=True)
        # (a)
        res = {}
        t0 = time.perf_counter()
        lat.gauge_snapshot()
        lat.sync()
        print("  (a) %-26s %9.3f ms   (first call: allocates %.0f MB; host clock)" % ("gauge_snapshot, first", 1e3 * (time.perf_counter() - t0), V * 576 / 1e6))
        lat.update_gauge(1e-3)
        rows = [("gauge_snapshot", lat.gauge_snapshot, 1152), ("gauge_restore", lat.gauge_restore, 2304), ("gauge_reunitarize", lat.gauge_reunitarize, 2304),
                ("gauge_snapshot_diff", lat.gauge_snapshot_diff, 1152), ("moment_energy", lat.moment_energy, 256), ("derivative_norms", lat.derivative_norms, 256)]
        for name, fn, bps in rows:
            res[name] = device_ms(lat, fn)
            print("  (a) %-26s %9.3f ms   %4d B/site -> %6.0f GB/s" % (name, res[name], bps, bps * V / (res[name] * 1e-3) / 1e9), flush=True)
        # (b)
        lat.gauge_snapshot()
        forms = {}
        for form, name in ((0, "restore: copy + re-sort"), (1, "restore: one pass"), (2, "accept: restoresu3 + re-sort"), (3, "accept: one pass")):
            forms[form] = statistics.median(lat.bench_trajectory_forms(form, 1) for _ in range(REPS))
            print("  (b) %-30s %9.3f ms" % (name, forms[form]), flush=True)
        print("  (b) restore one pass / two launches = %.3f   accept one pass / two launches = %.3f" % (forms[1] / forms[0], forms[3] / forms[2]), flush=True)
        # (c)
        sq = device_ms(lat, lambda: lat.square_norm(x, lat.Vh, 0))
        rate_sq = 192.0 * lat.Vh / (sq * 1e-3) / 1e9
        print("  (c) %-26s %9.3f ms   %.1f MB -> %6.0f GB/s" % ("square_norm (one parity)", sq, 192.0 * lat.Vh / 1e6, rate_sq), flush=True)
        for name, bps in (("moment_energy", 256), ("gauge_snapshot_diff", 1152), ("derivative_norms", 256)):
            rate = bps * V / (res[name] * 1e-3) / 1e9
            print("  (c) %-26s %9.3f ms   %.1f MB -> %6.0f GB/s = %.2f x square_norm's rate" % (name, res[name], bps * V / 1e6, rate, rate / rate_sq), flush=True)
        # (d)
        before = {"gauge_download": host_ms(lat.gauge_download), "momenta_download": host_ms(lat.momenta_download), "set_gauge": host_ms(lambda: lat.set_gauge(g))}
        for name, ms in before.items():
            print("  (d) %-26s %9.3f ms   (host clock)" % (name, ms), flush=True)
        ref = None
        if L == 16:
            try:
                ref = reference_leg(L)
            except Exception as e:   # noqa: BLE001 (a missing or unloadable reference build is not this tool's failure)
                print("  (d) reference host loops: skipped (%s)" % e)
            else:
                if ref is None:
                    print("  (d) reference host loops: skipped (oracle/_ref/libtmtraj.so is not on this machine)")
                else:
                    for name, ms in ref.items():
                        print("  (d) reference %-16s %9.3f ms   (one thread, as the reference's moment_energy; host clock)" % (name, ms), flush=True)
        lat.gauge_snapshot_free()
        paid = sum(before.values())
        for end in ("gauge_reunitarize", "gauge_restore"):
            dev = res["gauge_snapshot"] + 2 * res["moment_energy"] + res[end]
            print("  end of trajectory: snapshot + 2 moment_energy + %-17s = %8.3f ms  against  downloads + upload = %9.3f ms  -> %s" % (
                end, dev, paid, "%.1f x less" % (paid / dev) if dev < paid else "NOT less"), flush=True)
        lat.close()


if __name__ == "__main__":
    main()
