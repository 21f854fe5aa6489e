"""GPU: bicgstab_complex and its two linalg symbols through the drop-in, in a process of their own (tests/bicg_dropin_child.py): host
arrays, coherent and lazy residency, the device-resident path for the operators the library knows and the host loop for a foreign f."""
import numpy as np
import pytest

from tests.hostprog import run_child

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["coherent", "lazy"])
def test_dropin_symbols(mode):
    out = run_child("bicg_dropin_child.py", mode)
    print(out)
    for k, v in out["linalg"].items():
        assert v is True or v <= 8, (k, v)                     # eps times the sum of the magnitudes of an element's terms, as tests/test_gpu_bicg.py
    assert out["linalg"]["N0_unchanged"] is True
    for name in ("mtm_plus_sym", "mtm_plus_sym_guess", "d_psi"):
        s = out["solves"][name]
        assert s["iters"] == s["ref_iters"] and s["q_unchanged"], (name, s)
        assert s["calls"] == 1, (name, s)                      # the resident path: one entry point served, no linalg call came back to the library
        assert s["true"] <= s["bound"] * out["margin"], (name, s)
        assert s["dist"] <= 2.0 * np.sqrt(s["bound"]) / s["sigma_min"], (name, s)
    g = out["solves"]["foreign"]
    assert 0 < g["iters"] <= 10 * g["restated_iters"] and g["q_unchanged"], g   # (no count is pinned for an operator the fixtures do not cover)
    assert g["calls"] > 10 * g["iters"], g                      # the host loop: every statement of every iteration is a call of its own
    assert g["true"] <= g["bound"] * out["margin"], g
    # an operator of the library outside the solver's set takes the host loop as well: more than one entry-point call served
    assert set(out["routing"]) == {"cg_her_mtm_plus_sym", "bicgstab_qtm_pm"}
    for name, calls in out["routing"].items():
        assert calls > 1, (name, calls)
