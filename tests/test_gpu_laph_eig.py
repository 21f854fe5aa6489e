"""GPU: tmhip_laph_eigensystem, the nev lowest eigenpairs of the 3D Laplacian on every time-slice in lock-step
(tmlqcd_amd/csrc/laph.hip), on tests.util.random_gauge links.

The reference's own eigen-driver cannot be built, so eigenvalues are held against numpy.linalg.eigvalsh of the dense matrix of
tests/laph_restate.py (pinned to the reference's object code by tests/test_laph_restate.py), and the run itself -- applications and
converged pairs per slice -- against tests/eig_restate.py, the NumPy statement of the per-slice algorithm, from the same start vector.

Bounds.  resid <= prec = 1e-8.  Orthonormality per slice within 1e-12.  |evals - dense| <= resid + 1e-12: for a Hermitian matrix an
exact eigenvalue lies within the residual of a Ritz value, 1e-12 covers the rounding of a spectrum bounded by 12.  No eigenvalue is
skipped: exactly nev dense eigenvalues lie below evals[nev - 1] + 1e-7.  Premise, asserted: consecutive dense eigenvalues among the
lowest nev + 1 of every slice differ by more than 1e-6.
"""
import numpy as np
import pytest

from tests import eig_restate as er
from tests import laph_restate as lr
from tests.util import random_gauge

pytestmark = pytest.mark.gpu

PREC = 1e-8
SHAPES = [(2, 2, 2, 2), (4, 2, 6, 2), (6, 10, 2, 4), (4, 4, 4, 16), (10, 10, 6, 14)]
IDS = ["x".join(str(d) for d in s) for s in SHAPES]


@pytest.fixture(scope="module")
def lats():
    from tmlqcd_amd import Lattice
    made = {}

    def get(shape, seed=11):
        if shape not in made:
            lat = Lattice(*shape)
            g = random_gauge(seed, lat.V)
            lat.set_gauge(g)
            made[shape] = (lat, g, {})
        return made[shape]
    yield get
    for lat, _, _ in made.values():
        lat.close()


def _dense_evals(cache, g, shape, t):
    if t not in cache:
        cache[t] = np.linalg.eigvalsh(lr.dense(g, shape, t))
    return cache[t]


def _check(lat, g, shape, cache, r, nev, slices, t0=0):
    T, N = lat.T, 3 * (lat.V // lat.T)
    assert np.all(r["converged"] == nev), r["converged"]
    assert np.all(r["resid"] <= PREC), r["resid"].max()
    assert np.all(np.diff(r["evals"], axis=1) >= 0.0)
    vec = np.stack([lr.cplx(f.download()).reshape(T, N) for f in r["vectors"]], axis=1)      # [T][nev][N]
    for t in slices:
        ev, rs, v = r["evals"][t - t0], r["resid"][t - t0], vec[t]
        d = _dense_evals(cache, g, shape, t)
        assert np.all(np.diff(d[:nev + 1]) > 1e-6), (t, np.diff(d[:nev + 1]).min())              # the premise
        assert np.abs(np.conj(v) @ v.T - np.eye(nev)).max() <= 1e-12
        assert np.all(np.abs(ev - d[:nev]) <= rs + 1e-12), (t, np.abs(ev - d[:nev]).max())
        assert int(np.sum(d < ev[nev - 1] + 1e-7)) == nev
        # the values returned are the Rayleigh quotients and residuals of the vectors returned
        A = lr.dense(g, shape, t) if N <= 800 else None
        if A is not None:
            Av = v @ A.T
            theta = np.einsum("in,in->i", np.conj(v), Av).real
            assert np.abs(theta - ev).max() <= 1e-12
            assert np.abs(np.linalg.norm(Av - theta[:, None] * v, axis=1) - rs).max() <= 1e-12


@pytest.mark.parametrize("nev", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_lowest_eigenpairs_of_every_slice(lats, shape, nev):
    lat, g, cache = lats(shape)
    if 3 * (lat.V // lat.T) < nev + 2:
        pytest.fail("the shape has fewer than nev + 2 unknowns per slice")
    r = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000, vectors=True)
    try:
        print("apps per slice", r["apps"])
        slices = range(lat.T) if shape != (10, 10, 6, 14) else (0, 7)     # a dense problem there is 2520 x 2520: two slices only
        _check(lat, g, shape, cache, r, nev, slices)
    finally:
        for f in r["vectors"]:
            f.free()


def _restated(g, shape, t, start, nev, m, cheb, max_apps=20000):
    A = lr.dense(g, shape, t)
    return er.eigenvalues(lambda x: A @ x, lr.cplx(start[t]).reshape(-1), nev, which=0, prec=PREC, max_apps=max_apps, m=m, cheb=cheb)


@pytest.mark.parametrize("cheb", [0, 8])
@pytest.mark.parametrize("shape", [(4, 2, 6, 2), (4, 4, 4, 16)], ids=["4x2x6x2", "4x4x4x16"])
def test_run_for_run_against_the_numpy_statement(lats, shape, cheb):
    lat, g, _ = lats(shape)
    nev, m = 4, 14
    start = np.random.default_rng(31).standard_normal((lat.T, lat.V // lat.T, 3, 2))
    old = lat.get_option("laph_cheb")
    lat.set_option("laph_basis", m)
    lat.set_option("laph_cheb", cheb)
    try:
        r = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000, start=start)
        # a sub-range sees the same slices
        r1 = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000, start=start, t0=1, nt=2)
    finally:
        lat.set_option("laph_basis", 0)
        lat.set_option("laph_cheb", old)
    for t in range(lat.T):
        want = _restated(g, shape, t, start, nev, m, cheb)
        print(t, "apps", r["apps"][t], want["apps"], "converged", r["converged"][t], want["converged"])
        assert r["apps"][t] == want["apps"] and r["converged"][t] == want["converged"]
        assert np.abs(r["evals"][t] - want["evals"]).max() <= 1e-10
    assert np.array_equal(r1["evals"], r["evals"][1:3]) and np.array_equal(r1["apps"], r["apps"][1:3]) and np.array_equal(r1["resid"], r["resid"][1:3])


def _two_speeds(shape, seed, easy):
    """links whose slices `easy` are pulled toward unity: their lowest eigenvalues separate and they converge in fewer cycles"""
    from tmlqcd_amd import Lattice
    lat = Lattice(*shape)
    g = random_gauge(seed, lat.V)
    for t in easy:
        g = lr.scale_slice_toward_unity(g, shape, t, 0.25)
    lat.set_gauge(g)
    lat.set_option("laph_basis", 20)      # a short cycle and a low degree: the slices part ways after a few cycles
    lat.set_option("laph_cheb", 8)
    return lat, g


def test_slices_of_different_difficulty_freeze_on_their_own():
    shape, nev, easy = (4, 4, 4, 16), 4, 2
    lat, g = _two_speeds(shape, 13, [easy])
    try:
        r = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000, vectors=True)
        print("apps per slice", r["apps"])
        assert np.all(r["apps"][[t for t in range(lat.T) if t != easy]] != r["apps"][easy])     # it ends at another cycle than the rest
        _check(lat, g, shape, {}, r, nev, range(lat.T))
        # alone, the slice gives the bits it gave while the others went on
        solo = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000, vectors=True, t0=easy, nt=1)
        assert solo["apps"][0] == r["apps"][easy]
        assert np.array_equal(solo["evals"][0], r["evals"][easy]) and np.array_equal(solo["resid"][0], r["resid"][easy])
        for a, b in zip(solo["vectors"], r["vectors"]):
            assert np.array_equal(a.download()[easy], b.download()[easy])
        for f in solo["vectors"] + r["vectors"]:
            f.free()
    finally:
        lat.close()


def test_the_cap_ends_one_slice_and_not_the_others():
    shape, nev, hard = (4, 4, 4, 16), 4, 1
    lat, g = _two_speeds(shape, 13, [0, 2, 3])
    try:
        free = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000)
        others = [t for t in range(lat.T) if t != hard]
        cost = lat.get_option("laph_cheb")
        cap = int(free["apps"][others].max()) + cost + nev
        print("apps per slice", free["apps"], "cap", cap)
        assert cap < free["apps"][hard]                                   # the premise: only the raw slice needs more
        r = lat.laph_eigensystem(nev, prec=PREC, max_apps=cap)            # returns: reaching the cap is no error
        assert r["converged"][hard] < nev and r["apps"][hard] <= cap
        assert np.all(r["converged"][others] == nev) and np.all(r["resid"][others] <= PREC)
        assert np.array_equal(r["evals"][others], free["evals"][others]) and np.array_equal(r["apps"][others], free["apps"][others])
    finally:
        lat.close()


def test_the_default_start_vector_and_a_given_interval(lats):
    """no start vector: the fixed fill, the same run twice; an interval from the caller gives the same eigenvalues"""
    shape, nev = (4, 2, 6, 2), 4
    lat, g, cache = lats(shape)
    a = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000)
    b = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000)
    assert np.array_equal(a["evals"], b["evals"]) and np.array_equal(a["apps"], b["apps"])
    d = np.stack([_dense_evals(cache, g, shape, t) for t in range(lat.T)])
    lat.laph_set_interval(float(d[:, nev + 3].max()), 12.5)
    try:
        c = lat.laph_eigensystem(nev, prec=PREC, max_apps=20000)
    finally:
        lat.laph_set_interval(0.0, 0.0)
    assert np.all(c["converged"] == nev)
    assert np.all(np.abs(c["evals"] - d[:, :nev]) <= c["resid"] + 1e-12) and np.all(np.abs(a["evals"] - d[:, :nev]) <= a["resid"] + 1e-12)
