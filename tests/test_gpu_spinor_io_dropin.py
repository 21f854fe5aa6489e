"""GPU: the drop-in's propagator / source I/O in a process of its own (tests/spinor_io_dropin_child.py): point source, cg_her,
tmlqcd_hip_write_spinor, read_spinor into fresh arrays -- in coherent and in resident mode, e/o pairs and lexicographic fields."""
import json

import pytest

from tests.hostprog import run_child

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["coherent", "resident"])
def test_source_solve_write_read(mode):
    r = run_child("spinor_io_dropin_child.py", mode, check=False)      # (the library's prints are read too, and end up after the JSON line)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(out)
    assert out["source_ok"] and out["odd_point_ok"]
    assert 0 < out["iters"] < 2000 and out["solution_nonzero"] > 12 * 16
    assert out["file_ok"] and out["lex_file_ok"]
    assert (out["rc_read"], out["rc_read32"], out["rc_missing"], out["rc_read_lex"]) == (0, 0, -5, 0)
    assert out["read_equals_solution"] and out["read32_equals_rounded"] and out["lex_read_ok"]
    # nothing came down between the solve and the end of the write: the bus counters stand still and the program's pages are as before
    assert out["transfers_unchanged"] and out["host_pages_untouched_by_write"]
    if mode == "resident":
        assert out["host_before_sync_is_sentinel"]          # a read field stays in HBM until it is synchronised
    # the reference's prints (spinor_read.c:97-99, 140-144) and the -5 message
    assert "# Double precision read (64 bits)." in r.stdout and "# Single precision read (32 bits)." in r.stdout
    assert "# Scidac checksums for DiracFermion field" in r.stdout and "#   Read from LIME headers: A = 0x" in r.stdout
    assert "Unable to find requested LIME record scidac-binary-data" in r.stderr
