"""Child process of tests/test_gpu_spinor_io_dropin.py.

A host program in miniature, as tests/csg_dropin_child.py: the stub globals of tests/host_stub/globals.c are loaded first, then
libtmlqcd_dropin.so.  In the residency mode given on the command line it runs the five stages of an `invert` on one source, by
name and with host arrays:
  tmlqcd_hip_source_spinor_field -> cg_her(Qtm_pm_psi) -> tmlqcd_hip_write_lime_message + tmlqcd_hip_write_spinor -> read_spinor
into fresh arrays, then the lexicographic forms (r == NULL) and tmlqcd_hip_source_spinor_field_point_from_file, and prints what it
found as one JSON line."""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests import spinor_io_restate as sr  # noqa: E402
from tmlqcd_amd import synthetic as syn  # noqa: E402

VP = C.c_void_p
DIMS = (4, 4, 4, 6)
SENTINEL = -7.25


def main(mode, tmp):
    stub, _, d = hostprog.load()
    V = sr.volume(DIMS)
    N = V // 2
    hostprog.init_lattice(stub, *DIMS, syn.gauge_field(31, *DIMS)[:V], 0.125)
    stub.stub_set_mu(0.05)
    hf = hostprog.HostFields(stub, d, mode, modes=("coherent", "resident"))
    d.tmlqcd_hip_set_residency(hostprog.MODES[mode])   # (no way back at the end: tmlqcd_hip_finalize() ends this program)
    arr = lambda fill=0.0: hf.arr(V, fill)

    def counts():
        n = (C.c_ulong * 4)()
        d.tmlqcd_hip_transfer_counts(n)
        return list(n)

    out = {"mode": mode}
    # 1. source (spin 1, colour 2 at site 0) into arrays full of something else
    se, so = arr(SENTINEL), arr(SENTINEL)
    d.tmlqcd_hip_source_spinor_field(se[1], so[1], 1, 2)
    # 2. solve Q+Q- x = source on the even sites
    xe, xo = arr(SENTINEL), arr(SENTINEL)
    d.tmlqcd_hip_source_spinor_field_point_from_file(xe[1], xo[1], 0, 0, 0)        # (a starting guess; any would do)
    out["iters"] = d.cg_her(xe[1], se[1], 2000, 1e-20, 1, N, C.cast(d.Qtm_pm_psi, VP))
    junk = arr(SENTINEL)
    d.tmlqcd_hip_source_spinor_field_point_from_file(junk[1], xo[1], 2, 1, sr.odd_site(DIMS))   # the odd half (Q): a point source of its own
    before = counts()
    host_before = (xe[0][:N].copy(), xo[0][:N].copy())     # what the program's pages hold now (resident: not the solution)
    # 3. write: the records an op_write_prop writes around the data, then the propagator at 64 and at 32 bit
    path = os.path.join(tmp, "prop.lime").encode()
    assert d.tmlqcd_hip_write_lime_message(path, 0, b"propagator-type", b"DiracFermion_Sink", 1, 1) == 0
    assert d.tmlqcd_hip_write_lime_message(path, 1, b"inversion-info", b"solver = CG\n", 1, 1) == 0
    ps, pr = (VP * 1)(xe[1]), (VP * 1)(xo[1])
    assert d.tmlqcd_hip_write_spinor(path, 1, ps, pr, 1, 64) == 0
    assert d.tmlqcd_hip_write_spinor(path, 1, ps, pr, 1, 32) == 0
    out["transfers_unchanged"] = counts() == before
    out["host_pages_untouched_by_write"] = bool(np.array_equal(xe[0][:N], host_before[0]) and np.array_equal(xo[0][:N], host_before[1]))
    # 4. read back into fresh arrays
    ye, yo = arr(SENTINEL), arr(SENTINEL)
    out["rc_read"] = d.read_spinor(ye[1], yo[1], path, 0)
    ze, zo = arr(SENTINEL), arr(SENTINEL)
    out["rc_read32"] = d.read_spinor(ze[1], zo[1], path, 1)
    out["rc_missing"] = d.read_spinor(ze[1], zo[1], path, 2)
    if mode == "resident":
        out["host_before_sync_is_sentinel"] = bool(np.all(ye[0][:N] == SENTINEL))
        for a in (se, so, xe, xo, ye, yo, ze, zo):
            d.tmlqcd_hip_sync_to_host(a[1])
    sol_e, sol_o = xe[0][:N].copy(), xo[0][:N].copy()
    out["source_ok"] = bool(np.count_nonzero(se[0][:N]) == 1 and se[0][0, 1, 2, 0] == 1.0 and np.count_nonzero(so[0][:N]) == 0)
    out["solution_nonzero"] = int(np.count_nonzero(sol_e))
    want_o = sr.source_point(DIMS, 2, 1, sr.odd_site(DIMS))
    out["odd_point_ok"] = bool(np.count_nonzero(sol_o) == 1 and sol_o.reshape(N, 12, 2)[want_o[1], want_o[2], 0] == 1.0 and want_o[0] == 1)
    out["read_equals_solution"] = bool(np.array_equal(ye[0][:N], sol_e) and np.array_equal(yo[0][:N], sol_o))
    with np.errstate(over="ignore"):
        out["read32_equals_rounded"] = bool(np.array_equal(ze[0][:N], sol_e.astype(np.float32).astype(np.float64)) and
                                            np.array_equal(zo[0][:N], sol_o.astype(np.float32).astype(np.float64)))
    # the file is the restatement's, byte for byte
    want = (sr.lime_record(1, 1, "propagator-type", "DiracFermion_Sink") + sr.lime_record(1, 1, "inversion-info", "solver = CG\n") +
            sr.spinor_records([(sol_e, sol_o)], DIMS, 64) + sr.spinor_records([(sol_e, sol_o)], DIMS, 32))
    out["file_ok"] = open(path, "rb").read() == want
    # 5. r == NULL: lexicographic fields, written and read
    lex = arr()
    lex[0][:] = np.random.default_rng(5).standard_normal((V, 4, 3, 2))
    lpath = os.path.join(tmp, "lex.lime").encode()
    assert d.tmlqcd_hip_write_spinor(lpath, 0, (VP * 1)(lex[1]), None, 1, 64) == 0
    T, LX, LY, LZ = DIMS
    ix = np.arange(V)
    par = (ix % LZ + ix // LZ % LY + ix // (LZ * LY) % LX + ix // (LZ * LY * LX)) & 1
    ev, od = np.zeros((N, 4, 3, 2)), np.zeros((N, 4, 3, 2))
    ev[ix[par == 0] >> 1] = lex[0][par == 0]
    od[ix[par == 1] >> 1] = lex[0][par == 1]
    out["lex_file_ok"] = open(lpath, "rb").read() == sr.spinor_records([(ev, od)], DIMS, 64)
    back = arr(SENTINEL)
    out["rc_read_lex"] = d.read_spinor(back[1], None, lpath, 0)
    if mode == "resident":
        d.tmlqcd_hip_sync_to_host(back[1])
    out["lex_read_ok"] = bool(np.array_equal(back[0], lex[0]))
    d.tmlqcd_hip_finalize()
    hostprog.emit(out)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp_dir:      # prop.lime and lex.lime
        main(sys.argv[1], tmp_dir)
