"""Propagator / source records on the device against the host loop they replace, at 16^4 and 32^4, 64 and 32 bit
(-> profiles/r18_spinor_io_speed.log).  Every figure is the median of 7.

  (a) kernel     pack and unpack kernel alone (tmhip_bench_spinor_io: HIP events over 10 launches), with the bytes moved,
                 VOLUME x (192 + file bytes per site)
  (b) copy       the copy rate of this run -- assign() over four pairs of one-parity fields in turn, HIP events over 40 calls, as
                 bench.py's roofline.measured_stream -- and the time a copy of the same number of bytes takes at that rate
  (c) host       what the device path replaces: two tmhip_field_download calls (two uploads when reading) and the single-threaded site
                 loop of tools/spinor_io_harness.c (compiled here) around the reference's DML_checksum_accum from
                 oracle/_ref/libtmref_dml.so
  (d) whole call tmhip_write_spinor / tmhip_read_spinor by the host clock, to a file in the temporary directory

At 16^4 the fields and the record (25 MB together) stay in the Infinity Cache between launches; 32^4 (403 MB) is the HBM figure."""
import ctypes as C
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tmlqcd_amd import Lattice, hip  # noqa: E402

REPS = 7


def med(fn):
    return statistics.median(fn() for _ in range(REPS))


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def harness(tmp):
    so = os.path.join(tmp, "libspioharness.so")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "spinor_io_harness.c")])
    lib = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    for f in (lib.spio_host_write, lib.spio_host_read):
        f.argtypes = [vp, vp, i, i, i, i, i, vp, vp, vp]
        f.restype = None
    dml = os.path.join(ROOT, "oracle", "_ref", "libtmref_dml.so")
    if not os.path.exists(dml):
        return lib, None
    accum = C.cast(C.CDLL(dml).DML_checksum_accum, vp)
    return lib, accum


def run(L, tmp, hl, accum):
    lat = Lattice(L, L, L, L)
    V, Vh = lat.V, lat.Vh
    rng = np.random.default_rng(L)
    even, odd = rng.standard_normal((Vh, 4, 3, 2)), rng.standard_normal((Vh, 4, 3, 2))
    fe, fo = lat.field(even), lat.field(odd)
    # (b) the copy rate of this run
    fs = [lat.field() for _ in range(8)]

    def copy_rate():
        for k in range(4):
            lat.assign(fs[2 * (k & 3)], fs[2 * (k & 3) + 1], Vh)
        lat.event_record(12)
        for k in range(40):
            lat.assign(fs[2 * (k & 3)], fs[2 * (k & 3) + 1], Vh)
        lat.event_record(13)
        return 2 * 192.0 * Vh * 40 / (lat.event_elapsed_ms(12, 13) * 1e-3) / 1e9
    copy = med(copy_rate)
    for f in fs:
        f.free()
    print("%d^4 (b) copy yardstick: %.0f GB/s (assign over four pairs of one-parity fields, %.0f MB each)" % (L, copy, 192.0 * Vh / 1e6), flush=True)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    he, ho = np.zeros_like(even), np.zeros_like(odd)
    for prec in (64, 32):
        sb = 192 if prec == 64 else 96
        nbytes = V * (192.0 + sb)
        rec = np.zeros(V * sb, dtype=np.uint8)
        _, sums = lat.spinor_pack(fe, fo, prec, out=rec)
        # (a)
        for name, pack in (("pack", True), ("unpack", False)):
            ms = med(lambda: lat.bench_spinor_io(fe, fo, prec, pack, 10) / 10)
            print("%d^4 prec %d (a) %-6s kernel %8.3f ms  %6.0f GB/s over %.1f MB = %.2f of the copy rate (a copy of these bytes: %.3f ms)"
                  % (L, prec, name, ms, nbytes / ms / 1e6, nbytes / 1e6, nbytes / ms / 1e6 / copy, nbytes / copy / 1e6), flush=True)
        fe.upload(even); fo.upload(odd)              # (the 32-bit unpack rounded the fields)
        # (c)
        down = med(lambda: clock(lambda: (fe.download(out=he), fo.download(out=ho))))
        up = med(lambda: clock(lambda: (fe.upload(even), fo.upload(odd))))
        if accum is not None:
            hs = (C.c_uint32 * 2)()
            hrec = np.zeros(V * sb, dtype=np.uint8)
            wloop = med(lambda: clock(lambda: hl.spio_host_write(hp(even), hp(odd), L, L, L, L, prec, hp(hrec), accum, hs)))
            assert (hs[0], hs[1]) == sums and np.array_equal(hrec, rec), "host loop and device disagree"
            rloop = med(lambda: clock(lambda: hl.spio_host_read(hp(he), hp(ho), L, L, L, L, prec, hp(hrec), accum, hs)))
            assert (hs[0], hs[1]) == sums
            print("%d^4 prec %d (c) host path   write: 2 downloads %.1f ms + site loop %.1f ms = %.1f ms;  read: site loop %.1f ms + 2 uploads %.1f ms = %.1f ms"
                  % (L, prec, down, wloop, down + wloop, rloop, up, rloop + up), flush=True)
        else:
            print("%d^4 prec %d (c) host path   2 downloads %.1f ms, 2 uploads %.1f ms; oracle/_ref/libtmref_dml.so is not built: no site loop" % (L, prec, down, up), flush=True)
        # (d)
        path = os.path.join(tmp, "prop_%d_%d.lime" % (L, prec))
        def write():
            hip.write_lime_message(path, "propagator-type", "DiracFermion_Sink", 1, 1, append=False)
            lat.write_spinor(path, fe, fo, prec, append=True)
        wr = med(lambda: clock(write))
        ge, go = lat.field(), lat.field()
        rd = med(lambda: clock(lambda: lat.read_spinor(ge, go, path, 0)))
        rc, info = lat.read_spinor(ge, go, path, 0)
        assert rc == 0 and (info.suma, info.sumb) == (info.suma_stored, info.sumb_stored) == sums
        print("%d^4 prec %d (d) whole call  tmhip_write_spinor %.1f ms, tmhip_read_spinor %.1f ms (file of %.1f MB in the temporary directory)"
              % (L, prec, wr, rd, os.path.getsize(path) / 1e6), flush=True)
        os.unlink(path)
        ge.free(); go.free()
    lat.close()


if __name__ == "__main__":
    sizes = [int(x) for x in sys.argv[1:]] or [16, 32]
    with tempfile.TemporaryDirectory() as tmp:
        hl, accum = harness(tmp)
        for L in sizes:
            run(L, tmp, hl, accum)
