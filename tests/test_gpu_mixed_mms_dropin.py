"""GPU: the reference-named mixed_cg_mms_tm_nd of the drop-in library, with a solver_params_t, against the core call.

The host program in miniature of tests/hostprog.py runs in a child process (tests/mixed_mms_dropin_child.py) in both residency modes."""
import pytest

from tests.hostprog import run_child

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["lazy", "resident"])
def test_dropin_symbol_equals_the_core_call(mode):
    r = run_child("mixed_mms_dropin_child.py", mode)
    assert r["iters"] == r["iters_core"] and r["iters"] > 0, r
    assert abs(r["iters"] - r["reference_iters"]) <= max(3, r["reference_iters"] // 8), r     # the count rule, on the reference's own run
    assert r["updates_core"] > 0 and r["removed_core"] > 0, r
    assert r["solutions_bit_equal"] and r["source_untouched"], r
