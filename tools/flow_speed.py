"""Speed of the Wilson gradient flow on the device (flow.hip) on one MI355X (writes profiles/r12_flow_speed.log when given --out).

    python tools/flow_speed.py [--sizes 16 32] [--reps 7] [--out profiles/r12_flow_speed.log]        on a machine with the GPU
    python tools/flow_speed.py --reference /path/to/tmLQCD [--threads 16] [--out ...]                 on a CPU machine, appends
    (--reference TREE --keep-lib LIB.so builds the harness library only; --reference-lib LIB.so times it where the tree is absent)

GPU part: one child process per size, each under its own `timeout`; a size that fails ends the run.  Per L^4, warm-up call first, then
the median of `reps` timings with HIP events around the call (min .. max in brackets):
  flow step            three stage kernels; "stage" is a third of it (stage 0 reads no Z, stage 2 writes none)
  field strength       the clover-leaf kernel, its final reduction and the 16-byte result copy
  flow_observables     measure_plaquette on the flowed links + the field strength
  plaquette force      gauge_derivative without rectangles, the yardstick a stage is held against: a stage reads what it reads
                       and additionally writes a link and Z
Next to every kernel its unique bytes per site over the measured time, against the 5.5 TB/s copy rate of README (roofline.measured_stream).
At the largest size the whole gradient_flow(0.01, 1.0) -- 51 rows = 102 steps, 103 measurements -- by the host clock, and gauge_download, the
transfer a host-side measurement pays first.
Reference part: meas/gradient_flow.c and its measures compiled in place with OpenMP as tools/make_golden_flow.py does (harness build),
timed at 16^4 on the given number of threads: seconds per (step + measurement), and the 102 steps of gradient_flow(0.01, 1.0) scaled
by the volume to 32^4."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBPS = 5.5
# unique bytes per site: links 576 B; Z 288 B.  A stage reads and writes the links; Z is read by stages 1, 2 and written by stages 0, 1.
BYTES = {"flow step": 3 * (576 + 576) + 2 * 288 + 2 * 288, "field strength": 576, "flow_observables": 2 * 576, "plaquette force": 576 + 2 * 256}


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


def child(L, reps, whole):
    import numpy as np
    from tests.util import random_gauge
    from tmlqcd_amd import Lattice
    lat = Lattice(L, L, L, L, kappa=0.13, mu=0.01)
    V = lat.V
    lat.set_gauge(random_gauge(1, V))
    lat.derivative_zero()
    lat.flow_begin()
    print("L=%d  V=%d  flow buffers %.0f MB (two link copies + Z = 1440 B/site)" % (L, V, V * 1440 / 1e6), flush=True)
    rows = [("flow step", lambda: lat.flow_step(0.01)), ("field strength", lat.measure_field_strength),
            ("flow_observables", lat.flow_observables), ("plaquette force", lambda: lat.gauge_derivative(5.6))]
    res = {}
    for name, fn in rows:
        ms, lo, hi = timed(lat, fn, reps)
        res[name] = ms
        tb = BYTES[name] * V / (ms * 1e-3) / 1e12
        print("  %-18s %9.3f ms  (%.3f .. %.3f)   unique %4d B/site -> %5.2f TB/s = %4.1f %% of the %.1f TB/s copy" % (
            name, ms, lo, hi, BYTES[name], tb, 100 * tb / COPY_TBPS, COPY_TBPS), flush=True)
        if name == "flow step":
            print("  %-18s %9.3f ms   (a third of the step; unique %d B/site on average)" % ("stage", ms / 3, BYTES[name] // 3), flush=True)
    print("  stage / plaquette force = %.2f" % (res["flow step"] / 3 / res["plaquette force"]), flush=True)
    lat.flow_end()
    if whole:
        lat.gradient_flow(0.01, 0.02)
        t0 = time.perf_counter()
        rws = lat.gradient_flow(0.01, 1.0)
        gf = time.perf_counter() - t0
        lat.gauge_download()
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            lat.gauge_download()
            t.append(time.perf_counter() - t0)
        print("  gradient_flow(0.01, 1.0): %d rows, %.3f s by the host clock (%d steps + %d measurements: %.2f ms per step + measurement)" % (
            len(rws), gf, 2 * len(rws), 2 * len(rws) + 1, 1e3 * gf / (2 * len(rws))), flush=True)
        print("  gauge_download %.1f ms (best of 3, host clock): what a host-side measurement pays before its first step" % (1e3 * min(t)), flush=True)
        print("  last row: t %.2f  P %.12f  Esym %.12f  t^2 Esym %.12f  Wsym %.12f  Qsym %.12f" % tuple(np.array(rws[-1])[[0, 1, 3, 5, 6, 7]]), flush=True)
    lat.close()


def reference(ref, threads, lib=None, L=16, nsteps=4):
    from oracle.refbind import RefLattice
    from tests.util import random_gauge
    from tools.make_golden_flow import bind, build_lib
    with tempfile.TemporaryDirectory() as tmp:
        so = lib or build_lib(ref, tmp, omp=True)       # lib: a harness build made earlier (--keep-lib), for a machine without the tree
        r = RefLattice(L, L, L, L, kappa=0.13, mu=0.01, omp=True, threads=threads)
        r.gauge()[:] = random_gauge(1, r.V)
        r.mark_gauge_dirty()
        fl = bind(so)
        fl.tmflow_time(0.01, 1)
        sec = min(fl.tmflow_time(0.01, nsteps) for _ in range(3)) / nsteps
    out = ["reference (meas/gradient_flow.c: step_gradient_flow + measure_clover_field_strength_observables + measure_plaquette; harness build,",
           "  gcc -O3 -march=x86-64-v3 -fopenmp, %d OpenMP threads) at %d^4: %.4f s per step + measurement" % (threads, L, sec),
           "  -> the 102 steps of gradient_flow(0.01, 1.0): %.1f s at %d^4; scaled by the volume (x16) to 32^4: %.0f s, after the download of the links" % (
               102 * sec, L, 102 * 16 * sec)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per size")
    ap.add_argument("--note", action="append", default=[], help="a line for the log's header")
    ap.add_argument("--reference", help="time the reference from this tmLQCD tree on the CPU and append the result")
    ap.add_argument("--reference-lib", help="... from a harness build made earlier with --keep-lib")
    ap.add_argument("--keep-lib", help="with --reference: only build the harness library and keep it under this name")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--child", type=int)
    ap.add_argument("--whole", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.whole)
        return 0
    if a.reference and a.keep_lib:
        import shutil
        from tools.make_golden_flow import build_lib
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copy(build_lib(a.reference, tmp, omp=True), a.keep_lib)
        return 0
    if a.reference or a.reference_lib:
        lines = reference(a.reference, a.threads, a.reference_lib)
        print("\n".join(lines))
        if a.out:
            open(a.out, "a").write("\n".join(lines) + "\n")
        return 0
    lines = ["# tools/flow_speed.py: HIP events around each call, warm, median of %d (min .. max); one process per size." % a.reps,
             "# unique = bytes a call must move at least once; the gathered re-reads of the links are expected to be served by L2 / Infinity Cache."]
    lines += ["# " + n for n in a.note]
    print("\n".join(lines), flush=True)
    rc = 0
    for L in a.sizes:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(L), "--reps", str(a.reps)]
        if L == max(a.sizes):
            cmd.append("--whole")
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
