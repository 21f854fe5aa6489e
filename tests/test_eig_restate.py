"""CPU: tests/eig_restate.py (the NumPy restatement of the device eigensolver) against numpy.linalg.eigvalsh of the dense
matrix of oracle.nd_restate.Qtm_pm_ndpsi, built column by column through the CPU oracle's Hopping_Matrix.

Shapes 2^4 (dimension 192) and 4x2x6x2 (dimension 1152), the set-up of tests/test_gpu_nd_shapes.py (KAPPA, THETA, FIXTURE),
nev 1 and 4, both ends, prec 1e-10, unfiltered and with the Chebyshev filter.  Bound: |theta_i - lambda_i| <= resid_i +
1e-12 lambda_max; the 1e-12 covers the backward error n eps |A| of the dense solve at n <= 3072.  Premise, asserted: the
compared eigenvalues are separated by more than 100 prec.
"""
import numpy as np
import pytest

from oracle import nd_restate as nd
from tests import eig_restate as er
from tests.util import random_gauge, random_spinor

KAPPA = 0.13
THETA = (1.0, 0.3, -0.2, 0.5)
FIXTURE = (0.1375, 0.1175, 0.6931)
SHAPES = [(2, 2, 2, 2), (4, 2, 6, 2)]
PREC = 1e-10


class _Dense:
    def __init__(self, shape):
        from oracle.oraclebind import Oracle
        orc = Oracle(*shape, kappa=KAPPA, mu=0.0, theta=THETA, threads=1)
        seed = 1000 + sum(shape) * 7 + shape[0]
        orc.set_gauge(random_gauge(seed, orc.VPR))
        self.orc, self.N = orc, orc.Vh
        H = nd.hop_over(orc.Hopping_Matrix, self.N)
        n = 12 * self.N
        mb, eb, c = FIXTURE

        def A(x):
            u, d = nd.Qtm_pm_ndpsi(H, x[:n].reshape(self.N, 4, 3), x[n:].reshape(self.N, 4, 3), mb, eb, c)
            return np.concatenate([u.reshape(-1), d.reshape(-1)])
        self.A = A
        M = np.zeros((2 * n, 2 * n), dtype=np.complex128)
        e = np.zeros(2 * n, dtype=np.complex128)
        for j in range(2 * n):
            e[j] = 1.0
            M[:, j] = A(e)
            e[j] = 0.0
        assert np.abs(M - M.conj().T).max() <= 1e-13 * np.abs(M).max()
        self.lam = np.linalg.eigvalsh(0.5 * (M + M.conj().T))
        self.start = nd.cplx(np.concatenate([random_spinor(seed + 5, self.N), random_spinor(seed + 6, self.N)])).reshape(-1)


@pytest.fixture(scope="module")
def dense():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _Dense(shape)
        return made[shape]
    return get


def _want(lam, nev, which):
    return lam[:nev] if which == 0 else lam[::-1][:nev]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_premise_the_compared_eigenvalues_are_separated(dense, shape):
    lam = dense(shape).lam
    assert lam[0] > 0
    for end in (lam[:10], lam[-10:]):
        assert np.diff(end).min() > 100 * PREC, np.diff(end).min() / lam[-1]


# (which, cheb): the highest end runs unfiltered whatever "eig_cheb" says, so it has no filtered case of its own
ENDS = [(0, 0), (1, 0), (0, 8)]


@pytest.mark.parametrize("which,cheb", ENDS, ids=["lowest", "highest", "lowest-cheb8"])
@pytest.mark.parametrize("nev", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_finds_the_dense_eigenvalues(dense, shape, nev, which, cheb):
    st = dense(shape)
    r = er.eigenvalues(st.A, st.start, nev, which=which, prec=PREC, max_apps=4000, m=24, cheb=cheb)
    want = _want(st.lam, nev, which)
    print(shape, nev, which, cheb, "apps", r["apps"], "err", np.abs(r["evals"] - want).max(), "resid", r["resid"].max())
    assert r["converged"] == nev
    assert np.all(r["resid"] <= PREC)
    assert np.all(np.abs(r["evals"] - want) <= r["resid"] + 1e-12 * st.lam[-1]), (r["evals"], want)
    V = r["vectors"]
    assert np.abs(V.conj() @ V.T - np.eye(nev)).max() <= 1e-12


def test_the_cap_on_operator_applications_is_not_an_error(dense):
    st = dense(SHAPES[0])
    r = er.eigenvalues(st.A, st.start, 4, which=0, prec=PREC, max_apps=30, m=24)
    assert r["apps"] <= 30 and r["converged"] < 4
    assert np.all(np.isfinite(r["evals"])) and r["resid"].max() > PREC


@pytest.mark.parametrize("max_apps", [5, 26, 27, 28, 29, 40, 60])
@pytest.mark.parametrize("cheb", [0, 8])
def test_the_cap_includes_the_residuals_and_never_fails(dense, max_apps, cheb):
    """a loose prec makes the estimate check fire at the first restart, right at the cap for some of these values; with the filter and
    a cap too small for its probe cycle the run falls back to the unfiltered path"""
    st = dense(SHAPES[0])
    r = er.eigenvalues(st.A, st.start, 2, which=0, prec=0.5, max_apps=max_apps, m=24, cheb=cheb)
    assert r["apps"] <= max_apps
    assert np.all(np.isfinite(r["evals"]))


def test_an_interval_from_the_caller_is_used(dense):
    st = dense(SHAPES[0])
    lam = st.lam
    r = er.eigenvalues(st.A, st.start, 1, which=0, prec=PREC, max_apps=4000, m=24, cheb=8, interval=(lam[12], 1.05 * lam[-1]))
    assert r["converged"] == 1 and abs(r["evals"][0] - lam[0]) <= r["resid"][0] + 1e-12 * lam[-1]
