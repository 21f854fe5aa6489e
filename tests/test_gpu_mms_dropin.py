"""GPU: the drop-in cg_mms_tm (include/tmlqcd_dropin.h) with the solver parameters the rat monomial and invert_eo.c build, in
every residency mode (one child process each, tests/mms_dropin_child.py), and the generic path for an M_psi the library does
not know, against tests/golden/ref_mms_4x4.npz; cg_her's generic path in the same modes against tests/golden/ref_fields_4x4.npz."""
import pytest

from tests.hostprog import run_child

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["coherent", "lazy", "resident"])
def test_dropin_cg_mms_tm_in_every_residency_mode(mode):
    out = run_child("mms_dropin_child.py", mode)
    for name in ("qtm", "qpm_full", "qtm_generic"):
        assert out[name] < 1e-9, (name, out[name])
        assert out[name + "_iters"] <= 1, (name, out)
        assert 0.5 <= out[name + "_reached"] <= 2.0, (name, out)   # *cgmms_reached_prec is written
        assert out[name + "_sloppy"] == 0, (name, out)             # g_sloppy_precision is reset (cg_mms_tm.c:192)
    # cg_her with an f the library does not know, in this mode: the bounds of tests/test_gpu_operators.py for the same fixture
    assert out["cg_her_generic_iters"] <= 1, out
    assert out["cg_her_generic"] < 1e-9, out
    # ... and it left the mode as it found it: the next operator call is correct (without a sync in coherent mode, after one in
    # resident mode) and its result reached the host the way that mode brings it there
    assert out["cg_her_generic_then_Qtm_pm_psi"] < 1e-13, out
    assert out["cg_her_generic_mode_kept"] is True, out
