"""TEST INFRASTRUCTURE ONLY: fixtures of the propagator / source I/O (tests/golden/ref_spinor_io_<shape>.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so and libtmref_dml.so from the reference tree):

    python tools/make_golden_spinor_io.py

Nothing is compiled and nothing is written under oracle/.  What comes from the reference's object code:
  site order, parity   g_ipt and g_lexic2eosub of libtmref.so, walked as io/spinor_write_binary.c:145-169 walks them
  checksums            DML_checksum_accum of libtmref_dml.so over the sites of the record (oracle/ildgbind.ref_checksum)
  point sources        source_spinor_field of libtmref.so (site 0); for another site the selection rule of
                       source_spinor_field_point_from_file on the reference's g_ipt, g_lexic2eo, g_lexic2eosub
The input fields come from tests/spinor_io_restate.py (seeded), so a fixture holds results only: per precision the checksum pair and
the SHA-256 of the record, and the non-zero entries of the point sources.  The generator refuses to write a fixture that the NumPy
restatement does not reproduce exactly.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def gen(tag):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle import ildgbind as ib
    from oracle.refbind import RefLattice
    from tests import spinor_io_restate as sr
    dims = sr.SHAPES[tag]
    T, LX, LY, LZ = dims
    ref = RefLattice(*dims, kappa=0.125, mu=0.0)   # sets VOLUME, g_ipt, g_lexic2eosub and the other globals of libtmref.so
    lib, V = ref.lib, ref.V
    ipt = C.POINTER(C.POINTER(C.POINTER(C.POINTER(C.c_int)))).in_dll(lib, "g_ipt")
    l2s = C.POINTER(C.c_int).in_dll(lib, "g_lexic2eosub")
    par, idx = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
    f = 0
    for t in range(T):                              # the loop nest of write_binary_spinor_data on one rank
        for z in range(LZ):
            for y in range(LY):
                for x in range(LX):
                    idx[f] = l2s[ipt[t][x][y][z]]
                    par[f] = (t + x + y + z) % 2
                    f += 1
    even, odd = sr.fields(dims)
    sites = np.where((par == 0)[:, None], even.reshape(-1, 24)[idx], odd.reshape(-1, 24)[idx])
    out = {"dims": list(dims), "seed": sr.FIELD_SEED}
    for prec in (64, 32):
        with np.errstate(over="ignore"):
            rec = np.frombuffer(sites.astype(">f8" if prec == 64 else ">f4").tobytes(), dtype=np.uint8)
        sums = ib.ref_checksum(rec, 192 if prec == 64 else 96)
        mine, msums = sr.pack(even, odd, dims, prec)
        if not np.array_equal(mine, rec) or tuple(msums) != tuple(sums):
            sys.exit("%s prec %d: the restatement does not reproduce the reference (sums %s vs %s)" % (tag, prec, msums, sums))
        e2, o2, s2 = sr.unpack(rec, dims, prec)
        with np.errstate(over="ignore"):
            want = (even, odd) if prec == 64 else (even.astype(np.float32).astype(np.float64), odd.astype(np.float32).astype(np.float64))
        if not (np.array_equal(e2, want[0]) and np.array_equal(o2, want[1]) and tuple(s2) == tuple(sums)):
            sys.exit("%s prec %d: unpack of the restatement does not invert the record" % (tag, prec))
        out["prec%d" % prec] = {"suma": "%08x" % sums[0], "sumb": "%08x" % sums[1], "sha256": hashlib.sha256(rec.tobytes()).hexdigest()}
    # point sources.  Site 0: P, Q as the reference's source_spinor_field fills them (on the reference's own, aligned fields).
    # Any other site: source_spinor_field_point_from_file cannot be called in libtmref.so (it reads index_start, a global of
    # read_input.c that the library does not define), so its selection rule (start.c:793, 808-811) is walked here on the
    # reference's g_ipt, g_lexic2eo and g_lexic2eosub.
    vp = C.c_void_p
    lib.source_spinor_field.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.source_spinor_field.restype = None
    P, Q = ref.spinor(0, V // 2), ref.spinor(1, V // 2)
    l2e = C.POINTER(C.c_int).in_dll(lib, "g_lexic2eo")

    def nonzero():
        both = np.stack([P, Q]).reshape(2, V // 2, 12, 2)
        nz = np.argwhere(both != 0.0)
        return [[int(a), int(b), int(c), int(d), float(both[a, b, c, d])] for a, b, c, d in nz]

    g = sr.odd_site(dims)
    gz, gy, gx, gt = g % LZ, g // LZ % LY, g // (LZ * LY) % LX, g // (LZ * LY * LX)      # start.c:763-769, one rank
    loc = ipt[gt][gx][gy][gz]
    where = [0, int(l2e[loc])] if l2e[loc] < V // 2 else [1, int(l2s[loc])]
    src = {"site0": [], "odd_site": [], "odd_site_index": g}
    for is_ in range(4):
        for ic in range(3):
            P[:] = 1.0; Q[:] = 1.0
            lib.source_spinor_field(ref.sp(0), ref.sp(1), is_, ic)
            nz = nonzero()
            want = sr.source_point(dims, is_, ic, 0)
            if nz != [[want[0], want[1], want[2], 0, 1.0]]:
                sys.exit("%s: source_spinor_field(%d, %d) gives %s, the restatement %s" % (tag, is_, ic, nz, want))
            src["site0"].append(nz[0])
            want = sr.source_point(dims, is_, ic, g)
            if [want[0], want[1]] != where or want[0] != 1:
                sys.exit("%s: the reference's tables put site %d at %s, the restatement at %s" % (tag, g, where, want))
            src["odd_site"].append(where + [3 * is_ + ic, 0, 1.0])
    out["point_sources"] = src
    out["point_source_entry"] = "[field 0 = P (even) | 1 = Q (odd), e/o entry, component 3 spin + colour, 0 = re | 1 = im, value], in the order is, ic"
    json.dump(out, open(os.path.join(GOLD, "ref_spinor_io_%s.json" % tag), "w"), indent=1)
    print("%s: 64-bit %s %s  32-bit %s %s" % (tag, out["prec64"]["suma"], out["prec64"]["sumb"], out["prec32"]["suma"], out["prec32"]["sumb"]), file=sys.stderr)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", metavar="SHAPE")
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        gen(a.child)
        sys.exit(0)
    for so in ("libtmref.so", "libtmref_dml.so"):
        if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", so)):
            sys.exit("oracle/_ref/%s missing: run build() first" % so)
    sys.path.insert(0, ROOT)
    from tests import spinor_io_restate as sr
    for tag in sr.SHAPES:
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", tag])
