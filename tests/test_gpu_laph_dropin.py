"""GPU: the LapH entry points of the drop-in (libtmlqcd_dropin.so): Jacobi under its reference name on host vectors, and
tmlqcd_hip_laph_eigensystem with the files of eigenvalues_Jacobi.c:176-209, called by tests/laph_dropin_child.py in a fresh
process on 4x2x6x2.

Jacobi goes through the same kernel as tmhip_laph_apply on the same links: equal bit for bit, and within tests.util.TOL of the NumPy
statement.  The eigensystem is deterministic, so the files hold the bytes of the vectors the core library returns for the same
links: SPACEVOLUME x 3 complex doubles in host order, no header; an eigenvalue line is "%e" of the value and parses back to it
within the six digits written."""
import numpy as np
import pytest

from tests.hostprog import run_child
from tests.util import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def out():
    return run_child("laph_dropin_child.py")


def test_jacobi_on_host_pointers_is_laph_apply(out):
    assert out["jacobi_vs_core"] == 0.0
    assert out["jacobi_vs_numpy"] < TOL


def test_the_files_hold_the_vectors_and_the_values(out):
    T, nev, nstore = 4, 3, 17
    want = sorted(["eigenvalues.%.3d.%.4d" % (t, nstore) for t in range(T)] +
                  ["eigenvector.%.3d.%.3d.%.4d" % (i, t, nstore) for i in range(nev) for t in range(T)])
    assert out["files"] == want
    assert out["slices_done"] == T and out["core_converged"] == [nev] * T
    assert out["vector_bytes_equal"] and out["lines_equal"]
    parsed, evals = np.array(out["parsed"]), np.array(out["evals"])
    assert parsed.shape == (T, nev) and np.all(np.abs(parsed - evals) <= 5e-7 * np.abs(evals))
