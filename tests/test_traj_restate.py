"""CPU: the NumPy restatement of the trajectory frame (tests/traj_restate.py) against the reference's values
(tests/golden/ref_traj_*, made by tools/make_golden_traj.py from moment_energy.c, expo.c and the loops of update_tm.c and
monitor_forces.c).  The GPU tests measure the device against both; this file ties the two together without a GPU.

Bounds: the reference's moment_energy and its ddU loop are Kahan sums of float64 per-link values, which the restatement forms in the
same order of operations: within 4 x 2^-53 of math.fsum over them.  monitor_forces.c adds its per-link norms in a plain serial loop:
recursive summation of n non-negative terms is within (n - 1) x 2^-53 of their exact sum.  The maximum is one of the per-link values:
equal bits.  restoresu3 is about forty operations per entry on numbers of size one, 1e-15 absolute."""
import json
import os

import numpy as np
import pytest

from tests import traj_restate as tj

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ["4x4", "8x6x4x12"]
U = tj.U53


def scalars(tag):
    return json.load(open(os.path.join(GOLD, "ref_traj_scalars_%s.json" % tag)))


@pytest.fixture(scope="module")
def moved():
    """the links after update_gauge(momenta, 1e-3) by the CPU oracle, per shape (made once)"""
    from oracle.oraclebind import Oracle
    out = {}
    for tag in TAGS:
        dims = tuple(scalars(tag)["dims"])
        g = tj.gauge(dims)
        Oracle(*dims, kappa=0.125, mu=0.0).update_gauge(g, tj.momenta(dims), tj.DIFF_STEP)
        out[tag] = g
    return out


@pytest.mark.parametrize("tag", TAGS)
def test_inputs_are_the_fixture_s(tag):
    s = scalars(tag)
    assert s["seeds"] == {"gauge": tj.GAUGE_SEED, "noise": tj.NOISE_SEED, "momenta": tj.MOM_SEED, "derivative": tj.DERIV_SEED}
    assert s["noise"] == tj.NOISE and s["diff_step"] == tj.DIFF_STEP
    dims = tuple(s["dims"])
    assert tj.row_norm_deviation(tj.noisy_gauge(dims)) == s["noisy_row_deviation"] > 1e-4
    assert tj.row_norm_deviation(tj.gauge(dims)) < 1e-14


@pytest.mark.parametrize("tag", TAGS)
def test_moment_energy(tag):
    s = scalars(tag)
    plain, exact = tj.moment_energy(tj.momenta(tuple(s["dims"])))
    assert abs(s["moment_energy"] - exact) <= 4 * U * exact
    assert abs(plain - exact) <= 64 * U * exact          # NumPy's pairwise sum: log2(terms) + 8 levels at most


@pytest.mark.parametrize("tag", TAGS)
def test_gauge_diff(tag, moved):
    s = scalars(tag)
    g = tj.gauge(tuple(s["dims"]))
    plain, exact = tj.snapshot_diff(moved[tag], g)
    assert exact > 1e-4 * g.shape[0]                      # the step moved every link
    assert abs(s["gauge_diff"] - exact) <= 4 * U * exact
    assert tj.snapshot_diff(g, g.copy()) == (0.0, 0.0) and s["gauge_diff_equal_fields"] == 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_force_norms(tag):
    s = scalars(tag)
    df = tj.derivative(tuple(s["dims"]))
    plain, exact, mx = tj.derivative_norms(df)
    assert mx == s["force_max"]
    assert abs(s["force_sum"] - exact) <= (df.shape[0] * 4 - 1) * U * exact


def test_reunitarize():
    ref = np.load(os.path.join(GOLD, "ref_traj_4x4.npz"))["reunitarized"]
    noisy = tj.noisy_gauge((4, 4, 4, 4))
    got = tj.restoresu3(noisy)
    assert np.abs(got - ref).max() < 1e-15
    assert np.abs(got - noisy).max() > 1e-4               # the input really was off the group
    assert tj.row_norm_deviation(got) < 1e-14
    u = tj.cplx(got)
    assert np.abs(np.linalg.det(u) - 1.0).max() < 1e-3    # rows 0 and 1 are normalised, not orthogonalised: the noise's overlap stays
    again = tj.restoresu3(got)
    assert np.abs(again - got).max() <= 4 * 2.0 ** -52 and scalars("4x4")["reunitarize_twice_max_change"] <= 4 * 2.0 ** -52
