"""GPU: the eigenvalue measurement under the reference's names (libtmlqcd_dropin.so): eigenvalues_bi with &Qtm_pm_ndbipsi,
tmlqcd_hip_phmc_compute_ev and tmlqcd_hip_eigenvalues, called by tests/eig_dropin_child.py (a fresh process: the drop-in's
weak references bind to the host program's globals when it is loaded) on 4x2x6x2 in lazy and resident modes.

The reference is the dense spectrum of the CPU oracle's operators, computed by the child.  Bound on a converged value: the
residual is at most prec = 1e-9 there, so |theta - lambda| <= prec + 1e-12 lambda_max (the bound of tests/test_gpu_eig.py with
the residual replaced by its own bound, because these entry points return no residual).
"""
import pytest

from tests.hostprog import last_json, run_child

pytestmark = pytest.mark.gpu

PREC = 1e-9
WARN_MAX = "Warning: largest eigenvalue for monomial ndpoly_heavy larger than upper bound!"
WARN_MIN = "Warning: smallest eigenvalue for monomial ndpoly_heavy smaller than lower bound!"


def _child(mode):
    return run_child("eig_dropin_child.py", mode, check=False)      # (the tests read its stderr too)


@pytest.fixture(scope="module", params=["lazy", "resident"])
def run(request):
    r = _child(request.param)
    assert r.returncode == 0, r.stderr[-3000:]
    return last_json(r), r.stderr


def test_eigenvalues_bi_returns_the_first_eigenvalue_and_the_number_converged(run):
    out, _ = run
    tol = PREC + 1e-12 * out["lam_nd_max"]
    assert abs(out["bi_min"] - out["lam_nd_min"]) <= tol and out["bi_min_nev"] == 1
    assert abs(out["bi_max"] - out["lam_nd_max"]) <= tol and out["bi_max_nev"] == 1
    assert out["bi_capped_nev"] == 0                       # max_iterations = 1: not converged, and *nev says so


def test_phmc_compute_ev_writes_the_line_and_the_warnings(run):
    out, err = run
    inside = err.split("--- inside")[1].split("--- outside")[0]
    outside = err.split("--- outside")[1].split("--- end")[0]
    assert WARN_MAX not in inside and WARN_MIN not in inside
    assert WARN_MAX in outside and WARN_MIN in outside
    lines = out["file"]
    assert len(lines) == 2
    for line, key, traj, lmin, lmax in ((lines[0], "ev_in", 7, out["lam_nd_min"], out["lam_nd_max"]),
                                        (lines[1], "ev_out", 8, out["lam_nd_min_out"], out["lam_nd_max_out"])):
        lo, hi, evmin = out[key]
        tol = PREC + 1e-12 * lmax
        assert abs(lo - lmin) <= tol and abs(hi - lmax) <= tol
        assert line == "%.8d %1.5e %1.5e %1.5e %1.5e" % (traj, lo, hi, evmin, 1.)
        f = line.split()
        assert int(f[0]) == traj and float(f[1]) == float("%1.5e" % lo) and float(f[2]) == float("%1.5e" % hi) and float(f[4]) == 1.0


def test_single_flavour_vectors_come_back_in_the_host_layout(run):
    out, _ = run
    lmax = out["lam_one_max"]
    assert out["one_nev"] == 2 and out["one_first"] == out["one_evals"][0]
    for i in range(2):
        assert abs(out["one_evals"][i] - out["lam_one"][i]) <= PREC + 1e-12 * lmax
        assert abs(out["one_norms"][i] - 1.0) <= 1e-12
        assert out["one_resid"][i] <= PREC + 1e-12 * lmax


def test_another_operator_pointer_ends_the_program_with_the_message():
    r = _child("other_pointer")
    assert r.returncode != 0 and "returned for a pointer" not in r.stdout
    assert "eigenvalues_bi: only Qsq = Qtm_pm_ndbipsi / Qsw_pm_ndbipsi runs on the device" in r.stderr
