"""CPU: the NumPy statement of the 3D Laplacian (tests/laph_restate.py) is the reference's Jacobi().

The fixtures tests/golden/ref_laph_*.npz hold what the reference's own object code (jacobi.c, geometry_eo.c and
init/init_geometry_indices.c compiled with -DWITHLAPH, tools/make_golden_laph.py) returned for one colour-vector field on every
time-slice, and the neighbour tables its geometry() built.  The restatement matches them to tests.util.TOL; its dense matrix is that
operator, Hermitian, with a spectrum inside [0, 12] (6 minus six unitary hops), and a random gauge transformation leaves the
eigenvalues alone to 1e-12 -- which is what allows eigenvalues to be pinned to numpy.linalg.eigvalsh of that matrix where the
reference's own eigen-driver cannot be built."""
import os

import numpy as np
import pytest

from tests import laph_restate as lr
from tests.util import TOL, random_gauge, random_su3, rel_err

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = {"4x4": (4, 4, 4, 4), "8x6x4x12": (8, 6, 4, 12)}


def _case(tag):
    z = np.load(os.path.join(GOLD, "ref_laph_%s.npz" % tag))
    dims = tuple(int(d) for d in z["dims"])
    V = int(np.prod(dims))
    g = np.load(os.path.join(GOLD, "ref_mms_4x4.npz"))["gauge"][:V] if tag == "4x4" else random_gauge(123456, V)
    return z, dims, g


@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_restatement_matches_the_reference_object_code(tag):
    z, dims, g = _case(tag)
    assert dims == SHAPES[tag]
    up, dn = lr.neighbours(*dims[1:])
    assert np.array_equal(up.T, z["iup3d"][:, 1:]) and np.array_equal(dn.T, z["idn3d"][:, 1:])     # the reference's geometry()
    assert rel_err(lr.apply_field(g, dims, z["k"]), z["l"]) < TOL
    t0, nt = 1, 2
    part = lr.apply_field(g, dims, z["k"], t0, nt)
    assert rel_err(part[t0:t0 + nt], z["l"][t0:t0 + nt]) < TOL and not part[:t0].any() and not part[t0 + nt:].any()


@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_dense_matrix_is_the_operator_hermitian_and_bounded(tag):
    z, dims, g = _case(tag)
    for t in (0, dims[0] - 1):
        A = lr.dense(g, dims, t)
        assert np.abs(A - A.conj().T).max() <= 1e-15
        l = A @ lr.cplx(z["k"][t]).reshape(-1)
        assert rel_err(lr.reals(l.reshape(-1, 3)), z["l"][t]) < TOL
        ev = np.linalg.eigvalsh(A)
        assert ev[0] >= -1e-12 and ev[-1] <= 12.0 + 1e-12, (ev[0], ev[-1])


def test_extent_two_counts_both_terms():
    """x + mu and x - mu are one site: the matrix element between the two sites is the sum of both hops"""
    dims = (2, 2, 2, 2)
    g = random_gauge(3, 16)
    A = lr.dense(g, dims, 1).reshape(8, 3, 8, 3)
    U = lr.cplx(g[8:16, 1:4])                                   # [site][mu][3][3]
    # sites 0 = (0,0,0) and 1 = (0,0,1) are neighbours along z (mu = 3) both ways
    assert np.abs(A[0, :, 1, :] + U[0, 2] + np.conj(U[1, 2]).T).max() <= 1e-15
    k = np.random.default_rng(1).standard_normal((8, 3)) + 0j
    assert np.abs(A.reshape(24, 24) @ k.reshape(-1) - lr.jacobi(g, dims, k, 1).reshape(-1)).max() <= 1e-13


def test_gauge_transformation_leaves_the_spectrum_alone():
    dims = (4, 2, 6, 2)
    V = int(np.prod(dims))
    g = random_gauge(8, V)
    omega = random_su3(np.random.default_rng(9), V)
    g2 = lr.gauge_transform(g, dims, omega)
    assert np.abs(g2 - g).max() > 0.1
    for t in range(dims[0]):
        a, b = np.linalg.eigvalsh(lr.dense(g, dims, t)), np.linalg.eigvalsh(lr.dense(g2, dims, t))
        assert np.abs(a - b).max() <= 1e-12


def test_smoothed_slice_is_another_problem_with_separated_low_end():
    dims = (4, 4, 4, 16)
    g = random_gauge(13, int(np.prod(dims)))
    g2 = lr.scale_slice_toward_unity(g, dims, 2, 0.25)
    S3 = 256
    assert np.array_equal(g2[:2 * S3], g[:2 * S3]) and np.array_equal(g2[3 * S3:], g[3 * S3:]) and np.array_equal(g2[:, 0], g[:, 0])
    d = np.linalg.eigvalsh(lr.dense(g2, dims, 2))
    assert np.all(np.diff(d[:9]) > 1e-6)
