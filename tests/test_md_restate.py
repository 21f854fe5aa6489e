"""CPU: tests/md_restate.py pinned on its own -- the long-double exponential against its inverse and against an independent
eigen-decomposition, the generator against the properties _make_su3 has, the row-2 measure on links that are SU(3) by
construction, and (where the oracle is built) the oracle's update_gauge against exp(step P) U inside the regime of its series."""
import numpy as np

from tests import md_restate as md
from tests.util import random_gauge

assert np.finfo(np.longdouble).eps < 2e-19, "long double is not extended precision here: md_restate's bounds do not hold"


def _momenta(seed, n, scale=1.0):
    return scale * np.random.default_rng(seed).standard_normal((n, 4, 8))


def test_su3_of_is_antihermitian_traceless_with_the_gell_mann_norm():
    p = _momenta(1, 50)
    v = md.su3_of(p)
    assert np.abs(v + np.conj(np.swapaxes(v, -1, -2))).max() == 0
    assert np.abs(np.trace(v, axis1=-2, axis2=-1)).max() < 4e-19 * np.abs(v).max()
    fro = np.sqrt((np.abs(v) ** 2).sum(axis=(-1, -2))).astype(np.float64)
    assert np.abs(fro - np.sqrt(2.0) * md.adj_norm(p)).max() < 1e-14
    # one generator at a time: lambda_3 and lambda_8 on the diagonal, lambda_1 / lambda_2 in the (0, 1) corner
    e = np.eye(8)
    l = md.su3_of(e).astype(np.complex128)
    assert np.allclose(l[2], 1j * np.diag([1, -1, 0])) and np.allclose(l[7], 1j * np.diag([1, 1, -2]) / np.sqrt(3))
    assert np.allclose(l[0][:2, :2], 1j * np.array([[0, 1], [1, 0]])) and np.allclose(l[1][:2, :2], np.array([[0, 1], [-1, 0]]))


def test_expm_ld_times_its_inverse_is_the_identity():
    for scale in (0.05, 1.0, 3.0):                      # |v| up to about 20: scaling and squaring at work
        v = md.su3_of(_momenta(2, 60, scale))
        d = md._mm(md.expm_ld(v), md.expm_ld(-v))
        d[..., range(3), range(3)] -= 1
        assert np.abs(d).max() < 1e-17, scale


def test_expm_ld_agrees_with_the_eigen_decomposition():
    for scale in (0.05, 1.0, 3.0):
        v = md.su3_of(_momenta(3, 60, scale))
        h = (-1j * v).astype(np.complex128)             # Hermitian
        w, q = np.linalg.eigh(h)
        e = np.einsum("...ij,...j,...kj->...ik", q, np.exp(1j * w), np.conj(q))
        assert np.abs(md.expm_ld(v).astype(np.complex128) - e).max() < 1e-14, scale


def test_expm_ld_is_unitary_with_unit_determinant():
    u = md.expm_ld(md.su3_of(_momenta(4, 60, 2.0)))
    d = md._mm(u, np.conj(np.swapaxes(u, -1, -2)))
    d[..., range(3), range(3)] -= 1
    assert np.abs(d).max() < 1e-17
    assert np.abs(np.linalg.det(u.astype(np.complex128)) - 1).max() < 1e-14


def test_row2_deviation_of_su3_links_and_of_a_scaled_link():
    g = random_gauge(5, 48)
    assert md.row2_deviation(g) < 1e-14
    g[7, 2] *= 1.0 + 1e-6                               # row2 scales by (1 + 1e-6), conj(row0 x row1) by its square
    dev = md.row2_deviation(g)
    assert 1e-7 < dev < 1e-6


def test_update_momenta_is_one_multiply_and_one_subtract():
    mom, d = _momenta(6, 48), _momenta(7, 48)
    out = md.update_momenta(mom, d, 0.05)
    assert np.array_equal(out, mom - 0.05 * d) and not np.shares_memory(out, mom)


def test_oracle_update_gauge_is_the_exponential_inside_its_regime():
    """The reference's series (the oracle is pinned to it bit for bit, tests/test_oracle_vs_ref.py) against exp(step P) U at
    (2, 2, 2, 6): within 2e-15 up to |step P| = 0.55, and visibly not at twice that -- the premise of
    tests/test_gpu_md_update.py::test_against_the_true_exponential."""
    from oracle.oraclebind import Oracle
    orc = Oracle(2, 2, 2, 6)
    g0, mom = random_gauge(3, 48), _momenta(4, 48)
    assert 4.5 < md.adj_norm(mom).max() <= 5.5
    dist = {}
    for step in (0.01, 0.1, 0.2):
        g = g0.copy()
        orc.update_gauge(g, mom, step)
        dist[step] = float(np.abs(md.cld(g) - md.update_gauge_ld(g0, mom, step)).max())
    print("oracle - exp(step P) U, max norm:", dist)
    assert dist[0.01] < 2e-15 and dist[0.1] < 2e-15
    assert dist[0.2] > 1e-14
