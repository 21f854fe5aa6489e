"""GPU: tmhip_eigenvalues / tmhip_eigenvalues_nd against the dense spectrum of the CPU oracle's operator with the device's own
gauge field, kappa, theta and parameters (the pattern of _Setup in tests/test_gpu_nd_shapes.py), on 2^4 and 4x2x6x2.

Operators: Qtm_pm_ndpsi at FIXTURE and at epsbar = 0 (nev = 1 there: every eigenvalue is double and one start vector finds
one vector per distinct eigenvalue), Qtm_pm_psi at mu = 0.01, Qsw_pm_psi on the synthetic clover term of
tests.util.random_clover, Q_pm_psi on FULL fields at 2^4.  Both ends, nev 1 and 4, "eig_fused" 1 and 0, "eig_cheb" 0 and 8,
prec 1e-9, max_apps 2000 (the NumPy runs of tests/test_eig_restate.py stay under 600).

Checks: converged == nev; |theta_i - lambda_i| <= resid_i + 1e-12 lambda_max (the bound of the CPU test: the residual norm
bounds the distance to the spectrum, 1e-12 covers the dense solve); resid_i <= prec, and resid_i equal to |A v - theta v|
recomputed through the public operator call to 1e-12 lambda_max; |V^H V - 1|_max <= 1e-12; the same bits of evals on a second
call.  The dense matrices are built once per module.
"""
import numpy as np
import pytest

from oracle import nd_restate as nd
from tests.util import random_clover, random_gauge, random_spinor

pytestmark = pytest.mark.gpu

KAPPA, MU = 0.13, 0.01
THETA = (1.0, 0.3, -0.2, 0.5)
FIXTURE = (0.1375, 0.1175, 0.6931)
EPS0 = (0.1375, 0.0, 0.6931)
SHAPES = [(2, 2, 2, 2), (4, 2, 6, 2)]
PREC, MAX_APPS = 1e-9, 2000
# (which, cheb): the highest end runs unfiltered whatever "eig_cheb" says
ENDS = [(0, 0), (1, 0), (0, 8)]
END_IDS = ["lowest", "highest", "lowest-cheb8"]


def _g5(z):
    out = z.copy()
    out[:, 2:] *= -1
    return out


class _Setup:
    """One lattice on both sides and the dense matrix of every operator, made on first use."""

    def __init__(self, shape):
        from oracle.oraclebind import Oracle
        from tmlqcd_amd import Lattice
        self.shape = shape
        self.orc = Oracle(*shape, kappa=KAPPA, mu=MU, theta=THETA, threads=8)
        self.lat = Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA)
        seed = 3000 + sum(shape) * 7 + shape[0]
        g = random_gauge(seed, self.orc.VPR)
        self.orc.set_gauge(g)
        self.lat.set_gauge(g)
        sw, swi = random_clover(seed + 1, self.orc, MU, scale=0.05)
        self.orc.set_clover(sw, swi)
        self.lat.set_clover(sw, swi)
        self.N, self.V = self.orc.Vh, self.orc.V
        self.H = nd.hop_over(self.orc.Hopping_Matrix, self.N)
        self.dense = {}

    # ---- the oracle's operators on flat complex vectors
    def _eo(self, name):
        def A(x):
            out = self.orc.new_field()
            self.orc.op(name, out, nd.real(x.reshape(self.N, 4, 3)))
            return nd.cplx(out[:self.N]).reshape(-1)
        return A

    def _q_pm_full(self, x):
        """tm_operators.c:380-388: g5 D(+mu) g5 D(-mu) on the lexicographic field"""
        k = nd.real(x.reshape(self.V, 4, 3))
        t = np.zeros_like(k)
        self.orc.set_mu(-MU)
        self.orc.D_psi(t, k)
        self.orc.set_mu(MU)
        t = nd.real(_g5(nd.cplx(t)))
        out = np.zeros_like(k)
        self.orc.D_psi(out, t)
        return _g5(nd.cplx(out)).reshape(-1)

    def _nd(self, prm):
        n = 12 * self.N
        mb, eb, c = prm

        def A(x):
            u, d = nd.Qtm_pm_ndpsi(self.H, x[:n].reshape(self.N, 4, 3), x[n:].reshape(self.N, 4, 3), mb, eb, c)
            return np.concatenate([u.reshape(-1), d.reshape(-1)])
        return A

    def operator(self, case):
        if case == "nd_fixture":
            return self._nd(FIXTURE), 24 * self.N
        if case == "nd_eps0":
            return self._nd(EPS0), 24 * self.N
        if case == "Q_pm_psi":
            return self._q_pm_full, 12 * self.V
        return self._eo(case), 12 * self.N

    def spectrum(self, case):
        if case not in self.dense:
            A, dim = self.operator(case)
            M = np.zeros((dim, dim), dtype=np.complex128)
            e = np.zeros(dim, dtype=np.complex128)
            for j in range(dim):
                e[j] = 1.0
                M[:, j] = A(e)
                e[j] = 0.0
            assert np.abs(M - M.conj().T).max() <= 1e-12 * np.abs(M).max(), case
            self.dense[case] = np.linalg.eigvalsh(0.5 * (M + M.conj().T))
        return self.dense[case]

    # ---- the device
    def run(self, case, nev, which, cheb, **kw):
        lat = self.lat
        if case.startswith("nd_"):
            lat.set_nd(*(FIXTURE if case == "nd_fixture" else EPS0))
            return lat.eigenvalues_nd(nev, which=which, prec=PREC, max_apps=MAX_APPS, cheb=cheb, **kw)
        return lat.eigenvalues(nev, which=which, prec=PREC, max_apps=MAX_APPS, op=case, cheb=cheb, **kw)

    def apply_device(self, case, v):
        """A v through the public operator call -> flat complex; v: a field or an (up, dn) pair"""
        lat = self.lat
        if case.startswith("nd_"):
            lu, ld = lat.field(), lat.field()
            lat.Qtm_pm_ndpsi(lu, ld, v[0], v[1])
            out = np.concatenate([nd.cplx(lu.download()).reshape(-1), nd.cplx(ld.download()).reshape(-1)])
            lu.free(), ld.free()
            return out
        l = lat.field()
        lat.op(case, l, v)
        out = nd.cplx(l.download()).reshape(-1)
        l.free()
        return out


def _flat(case, v):
    if case.startswith("nd_"):
        return np.concatenate([nd.cplx(v[0].download()).reshape(-1), nd.cplx(v[1].download()).reshape(-1)])
    return nd.cplx(v.download()).reshape(-1)


@pytest.fixture(scope="module")
def setup():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _Setup(shape)
        return made[shape]
    yield get
    for st in made.values():
        st.lat.close()


CASES = [(s, c, n) for s in SHAPES for c, nevs in (("nd_fixture", (1, 4)), ("nd_eps0", (1,)), ("Qtm_pm_psi", (1, 4)), ("Qsw_pm_psi", (1, 4)))
         for n in nevs] + [(SHAPES[0], "Q_pm_psi", n) for n in (1, 4)]


def _free(vectors):
    for v in vectors:
        for f in (v if isinstance(v, tuple) else (v,)):
            f.free()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("which,cheb", ENDS, ids=END_IDS)
@pytest.mark.parametrize("shape,case,nev", CASES, ids=["%s-%s-nev%d" % ("x".join(map(str, s)), c, n) for s, c, n in CASES])
def test_eigenpairs_against_the_dense_spectrum(setup, shape, case, nev, which, cheb, fused):
    st = setup(shape)
    lam = st.spectrum(case)
    lmax = lam[-1]
    st.lat.set_option("eig_fused", fused)
    try:
        r = st.run(case, nev, which, cheb, vectors=True)
        again = st.run(case, nev, which, cheb)
    finally:
        st.lat.set_option("eig_fused", 1)
    vectors = r["vectors"]
    try:
        # the i-th distinct eigenvalue from the wanted end (epsbar = 0: every eigenvalue is double)
        want = lam[:nev] if which == 0 else lam[::-1][:nev]
        print(shape, case, nev, which, cheb, fused, "apps", r["apps"], "err", np.abs(r["evals"] - want).max(), "resid", r["resid"].max())
        assert r["converged"] == nev
        assert np.all(r["resid"] <= PREC)
        assert np.all(np.abs(r["evals"] - want) <= r["resid"] + 1e-12 * lmax), (r["evals"], want)
        assert np.array_equal(r["evals"], again["evals"]) and r["apps"] == again["apps"]
        V = np.stack([_flat(case, v) for v in vectors])
        assert np.abs(V.conj() @ V.T - np.eye(nev)).max() <= 1e-12
        if case != "Q_pm_psi":
            for i, v in enumerate(vectors):
                y = st.apply_device(case, v)
                assert abs(np.linalg.norm(y - r["evals"][i] * V[i]) - r["resid"][i]) <= 1e-12 * lmax, i
        else:   # Q_pm_psi has no public entry point of its own (the solvers reach it by id): the oracle's composition recomputes
            A, _ = st.operator(case)
            for i in range(nev):
                assert abs(np.linalg.norm(A(V[i]) - r["evals"][i] * V[i]) - r["resid"][i]) <= 1e-12 * lmax, i
    finally:
        _free(vectors)


def test_the_cap_on_operator_applications_is_not_an_error(setup):
    st = setup(SHAPES[1])
    st.lat.set_nd(*FIXTURE)
    r = st.lat.eigenvalues_nd(4, which="lowest", prec=PREC, max_apps=30)
    assert r["converged"] == 0 and r["apps"] <= 30
    assert np.all(np.isfinite(r["evals"])) and r["resid"].max() > PREC


@pytest.mark.parametrize("cheb", [0, 8])
@pytest.mark.parametrize("max_apps", [5, 26, 27, 28, 29, 40, 60])
def test_the_cap_includes_the_residuals_and_never_fails(setup, max_apps, cheb):
    """A loose prec makes the estimate check fire at the first restart, right at the cap for some of these values: the residuals'
    applications are inside max_apps.  With the filter and a cap too small for its probe cycle the run falls back to the unfiltered
    path instead of failing.  The option "eig_cheb" is the context's own again after a call with cheb=."""
    st = setup(SHAPES[0])
    st.lat.set_nd(*FIXTURE)
    default = st.lat.get_option("eig_cheb")
    r = st.lat.eigenvalues_nd(2, which="lowest", prec=0.5, max_apps=max_apps, cheb=cheb)
    assert r["apps"] <= max_apps, r
    assert np.all(np.isfinite(r["evals"]))
    assert st.lat.get_option("eig_cheb") == default


def test_a_start_vector_and_an_interval_from_the_caller(setup):
    st = setup(SHAPES[1])
    lam = st.spectrum("Qtm_pm_psi")
    lat = st.lat
    start = random_spinor(77, st.N)
    try:
        lat.eig_set_interval(lam[12], 1.05 * lam[-1])
        a = lat.eigenvalues(1, which="lowest", prec=PREC, max_apps=MAX_APPS, start=start, cheb=8)
    finally:
        lat.eig_set_interval(0.0, 0.0)
    b = lat.eigenvalues(1, which="lowest", prec=PREC, max_apps=MAX_APPS, start=start)
    c = lat.eigenvalues(1, which="lowest", prec=PREC, max_apps=MAX_APPS)
    for r in (a, b, c):
        assert r["converged"] == 1 and abs(r["evals"][0] - lam[0]) <= r["resid"][0] + 1e-12 * lam[-1]
    assert b["apps"] != c["apps"] or b["evals"][0] != c["evals"][0]      # another start vector, another run


def test_refusals_carry_a_message(setup, capfd):
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    st = setup(SHAPES[0])
    lat = st.lat
    with pytest.raises(TmHipError):
        lat.eigenvalues(1, op="Qtm_plus_psi")
    assert "eigenvalues does not take Qtm_plus_psi" in capfd.readouterr().err
    bare = Lattice(*SHAPES[0], kappa=KAPPA, mu=MU, theta=THETA)
    try:
        bare.set_gauge(random_gauge(1, bare.VPR))
        with pytest.raises(TmHipError):
            bare.eigenvalues(1, op="Qsw_pm_psi")
        assert "without a valid clover term" in capfd.readouterr().err
    finally:
        bare.close()
    try:
        lat.set_option("eig_basis", 5)
        with pytest.raises(TmHipError):
            lat.eigenvalues(4)
        assert "eig_basis" in capfd.readouterr().err
        with pytest.raises(TmHipError):
            lat.set_option("eig_basis", 65)
        assert "eig_basis" in capfd.readouterr().err
    finally:
        lat.set_option("eig_basis", 24)
    with pytest.raises(TmHipError):
        lat.eigenvalues(1, N=st.N - 1)
    assert "VOLUME/2" in capfd.readouterr().err
