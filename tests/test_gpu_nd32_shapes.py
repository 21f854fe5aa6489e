"""GPU: the fp32 doublet (nd32.hip) against oracle/nd_restate.py in fp64 over the CPU oracle's Hopping_Matrix, on fp32-rounded
inputs, on the shapes and launch forms where the kernel can go wrong (the set-up of tests/test_gpu_nd_shapes.py: kappa 0.13,
theta = (1, 0.3, -0.2, 0.5)).

* operators: (2,2,2,2) where the +mu and -mu neighbours coincide, (4,2,6,2) with LZ/2 = 1, two ragged shapes, and the two padded
  XCD grids (partial last wave, padding blocks, odd LZ/2); three (mubar, epsbar) points; both forms ("nd_fused" 1 / 0), every "xcd"
  and "gauge_cache" form on the padded shapes, and l == k.  Bounds: the project's fp32 bounds in the max-norm, TOL32 for the
  site-local calls and 4 TOL32 for the four-hop operator.  The point with 1 + mubar^2 - epsbar^2 = 0.05 of the fp64 tests is left
  out: it multiplies fp32 rounding by 20 per M_ee_inv.
* rg_mixed_cg_her_nd against the restated cg_her_nd: true residual, solution, and the same result for polling intervals 1 and 4.
* refusals: the clover doublet by the operator table, a loopback context before any launch.
"""
import numpy as np
import pytest

from oracle import nd_restate as nd
from tests.util import random_gauge, random_spinor

pytestmark = pytest.mark.gpu

KAPPA = 0.13
THETA = (1.0, 0.3, -0.2, 0.5)
FIXTURE = (0.1375, 0.1175, 0.6931)                                    # (mubar, epsbar, invmaxev) of tests/golden/ref_nd_*
PARAMS = [FIXTURE, (0.1375, 0.0, 0.6931), (0.0, 0.1175, 0.6931)]      # the first three of tests/test_gpu_nd_shapes.py
SMALL = [(2, 2, 2, 2), (4, 2, 6, 2), (6, 10, 2, 4), (4, 4, 4, 16)]
XCD = [((10, 10, 6, 14), 0), ((18, 12, 12, 14), 256)]                 # (shape, "block"): the padded XCD grid of nd_launch_hop
SHAPES = [(s, 0) for s in SMALL] + XCD
TOL32 = 2e-6                                                          # tests/test_gpu_mixed.py
BOUND = {"Qtm_pm_ndpsi_32": 4 * TOL32, "M_ee_inv_ndpsi_32": TOL32, "M_oo_sub_g5_ndpsi_32": TOL32}


def rel(a, b):
    """max |a - b| / max |b| over both flavours of a pair"""
    a, b = np.concatenate([np.ravel(x) for x in a]).astype(np.float64), np.concatenate([np.ravel(x) for x in b]).astype(np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_xcd_shapes_take_the_padded_grid():
    """The premise of the XCD cases (the grid rule of nd_launch_hop, kept by the fp32 stencil)."""
    for (T, LX, LY, LZ), block in XCD:
        Vh = T * LX * LY * LZ // 2
        bs = block or (64 if Vh < 131072 else 256)
        nb = (Vh + bs - 1) // bs
        assert nb >= 64 and nb % 8 != 0 and Vh % 64 != 0, (T, LX, LY, LZ, nb)


class _Setup:
    """One lattice on both sides: the same gauge, kappa and theta for the oracle and the device; fp32-rounded spinors."""

    def __init__(self, shape, block):
        from oracle.oraclebind import Oracle
        from tmlqcd_amd import Lattice
        self.shape, self.block = shape, block
        self.orc = Oracle(*shape, kappa=KAPPA, mu=0.0, theta=THETA, threads=8)
        self.lat = Lattice(*shape, kappa=KAPPA, mu=0.0, theta=THETA)
        seed = 2000 + sum(shape) * 7 + shape[0]
        g = random_gauge(seed, self.orc.VPR)
        self.orc.set_gauge(g)
        self.lat.set_gauge(g)
        if block:
            self.lat.set_option("block", block)
        self.N = self.orc.Vh
        self.H = nd.hop_over(self.orc.Hopping_Matrix, self.N)
        self.k32 = [random_spinor(seed + i, self.N).astype(np.float32) for i in range(1, 5)]   # k_s, k_c, j_s, j_c
        self.q = [random_spinor(seed + i, self.N) for i in (5, 6)]                              # the sources of the solver
        self.refs = {}

    def operators(self, prm):
        """The restated outputs (float64 pairs) in fp64 on the fp32-rounded inputs."""
        if prm not in self.refs:
            mb, eb, c = prm
            ks, kc, js, jc = (nd.cplx(a.astype(np.float64)) for a in self.k32)
            out = {"Qtm_pm_ndpsi_32": nd.Qtm_pm_ndpsi(self.H, ks, kc, mb, eb, c), "M_ee_inv_ndpsi_32": nd.m_ee_inv(ks, kc, mb, eb),
                   "M_oo_sub_g5_ndpsi_32": nd.m_oo_sub_g5(ks, kc, js, jc, mb, eb)}
            self.refs[prm] = {k: (nd.real(a), nd.real(b)) for k, (a, b) in out.items()}
        return self.refs[prm]

    def device_operators(self, prm):
        lat = self.lat
        mb, eb, c = prm
        lat.set_nd(mb, eb, c)
        ks, kc, js, jc = (lat.field32(a) for a in self.k32)
        ls, lc = lat.field32(), lat.field32()
        out = {}
        lat.Qtm_pm_ndpsi_32(ls, lc, ks, kc)
        out["Qtm_pm_ndpsi_32"] = (ls.download(), lc.download())
        lat.M_ee_inv_ndpsi_32(ls, lc, ks, kc, mb, eb)
        out["M_ee_inv_ndpsi_32"] = (ls.download(), lc.download())
        lat.M_oo_sub_g5_ndpsi_32(ls, lc, ks, kc, js, jc, mb, eb)
        out["M_oo_sub_g5_ndpsi_32"] = (ls.download(), lc.download())
        for f in (ks, kc, js, jc, ls, lc):
            f.free()
        return out


@pytest.fixture(scope="module")
def setup():
    made = {}

    def get(shape, block=0):
        if (shape, block) not in made:
            made[(shape, block)] = _Setup(shape, block)
        return made[(shape, block)]
    yield get
    for st in made.values():
        st.lat.close()


def _check_operators(st, prm, tag):
    ref, got = st.operators(prm), st.device_operators(prm)
    errs = {k: rel(got[k], ref[k]) for k in BOUND}
    bad = {k: v for k, v in errs.items() if not v < BOUND[k]}
    assert not bad, (st.shape, tag, prm, errs)


_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "b%d" % v


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("prm", PARAMS, ids=["fixture", "epsbar0", "mubar0"])
@pytest.mark.parametrize("shape,block", SHAPES, ids=_ids)
def test_operators_match_restatement(setup, shape, block, prm, fused):
    st = setup(shape, block)
    st.lat.set_option("nd_fused", fused)
    try:
        _check_operators(st, prm, {"nd_fused": fused})
    finally:
        st.lat.set_option("nd_fused", 1)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("shape,block", XCD, ids=["10x10x6x14", "18x12x12x14_b256"])
def test_operators_in_every_xcd_and_gauge_cache_form(setup, shape, block, fused):
    st = setup(shape, block)
    lat = st.lat
    lat.set_option("nd_fused", fused)
    try:
        for xcd in (0, 1, 3, 4):
            for gc in (0, 1):
                lat.set_option("xcd", xcd)
                lat.set_option("gauge_cache", gc)
                _check_operators(st, FIXTURE, {"nd_fused": fused, "xcd": xcd, "gauge_cache": gc})
    finally:
        lat.set_option("xcd", 2)
        lat.set_option("gauge_cache", -1)
        lat.set_option("nd_fused", 1)


@pytest.mark.parametrize("fused", [1, 0])
def test_output_may_alias_input(setup, fused):
    """l == k: the reference's Qtm_pm_ndpsi_32 reads k for the last time in its second stage."""
    st = setup((6, 10, 2, 4))
    lat = st.lat
    lat.set_nd(*FIXTURE)
    lat.set_option("nd_fused", fused)
    ref = st.operators(FIXTURE)
    try:
        ks, kc = lat.field32(st.k32[0]), lat.field32(st.k32[1])
        lat.Qtm_pm_ndpsi_32(ks, kc, ks, kc)
        assert rel((ks.download(), kc.download()), ref["Qtm_pm_ndpsi_32"]) < 4 * TOL32
        ks.free(); kc.free()
    finally:
        lat.set_option("nd_fused", 1)


# ---------------------------------------------------------------- solver
SOLVE = [((6, 10, 2, 4), 0), XCD[0]]
MAX_ITER, EPS_SQ = 5000, 1e-20


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("shape,block", SOLVE, ids=["6x10x2x4", "10x10x6x14"])
def test_rg_mixed_cg_her_nd_matches_restated_cg_her_nd(setup, shape, block, fused):
    st = setup(shape, block)
    mb, eb, c = FIXTURE
    f = lambda u, d: nd.Qtm_pm_ndpsi(st.H, u, d, mb, eb, c)
    qu, qd = nd.cplx(st.q[0]), nd.cplx(st.q[1])
    if "her" not in st.refs:
        z = np.zeros_like(qu)
        st.refs["her"] = nd.cg_her_nd(f, z, z, qu, qd, MAX_ITER, EPS_SQ, 1)
    it_ref, ru, rd = st.refs["her"]
    assert it_ref > 0
    lat = st.lat
    lat.set_nd(*FIXTURE)
    lat.set_option("nd_fused", fused)
    dq = lat.field(st.q[0]), lat.field(st.q[1])
    runs = {}
    try:
        for batch in (1, 4):
            lat.set_option("cg_batch", batch)
            for delta in (0.1, 1e-3):
                pu, pd = lat.field(), lat.field()
                it, counts = lat.rg_mixed_cg_her_nd(pu, pd, dq[0], dq[1], MAX_ITER, EPS_SQ, 1, lat.Vh, delta=delta)
                runs[(batch, delta)] = (it, counts, pu.download(), pd.download())
                pu.free(); pd.free()
    finally:
        dq[0].free(); dq[1].free()
        lat.set_option("cg_batch", 4)
        lat.set_option("nd_fused", 1)
    squarenorm = np.vdot(qu, qu).real + np.vdot(qd, qd).real
    for delta in (0.1, 1e-3):
        it, (n_out, n_sp, n_dp), u, d = runs[(4, delta)]
        assert it > 0 and it == n_out + n_sp + n_dp and n_out >= 2, (delta, it, n_out, n_sp, n_dp)
        e = rel((u, d), (nd.real(ru), nd.real(rd)))
        au, ad = f(nd.cplx(u), nd.cplx(d))
        res = (np.vdot(au - qu, au - qu).real + np.vdot(ad - qd, ad - qd).real) / squarenorm
        print("%s delta %g nd_fused %d: %d = %d + %d + %d (cg_her_nd %d), solution %.3e, residual^2/|Q|^2 %.3e"
              % (shape, delta, fused, it, n_out, n_sp, n_dp, it_ref, e, res))
        assert e < 1e-8, (delta, e)
        assert res <= EPS_SQ, (delta, res)
        it1, counts1, u1, d1 = runs[(1, delta)]              # what is enqueued after `done` must change nothing
        assert (it1, counts1) == (it, (n_out, n_sp, n_dp)), (delta, it1, counts1, it)
        assert np.array_equal(u1, u) and np.array_equal(d1, d), delta


# ---------------------------------------------------------------- refusals
def test_clover_doublet_is_refused_by_the_operator_table(setup, capfd):
    from tmlqcd_amd.hip import TmHipError
    st = setup((6, 10, 2, 4))
    lat = st.lat
    qu, qd = lat.field(st.q[0]), lat.field(st.q[1])
    sentinel = np.full_like(st.q[0], 7.0)
    pu, pd = lat.field(sentinel), lat.field(sentinel)
    capfd.readouterr()
    with pytest.raises(TmHipError):
        lat.rg_mixed_cg_her_nd(pu, pd, qu, qd, 100, 1e-20, 1, lat.Vh, delta=0.1, op="Qsw_pm_ndpsi")
    assert "rg_mixed_cg_her_nd does not take Qsw_pm_ndpsi" in capfd.readouterr().err
    assert np.array_equal(pu.download(), sentinel) and np.array_equal(pd.download(), sentinel)   # nothing was written
    for f in (qu, qd, pu, pd):
        f.free()


def test_loopback_context_is_refused_before_any_launch(capfd):
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    lat = Lattice(4, 4, 4, 4, kappa=KAPPA, mu=0.0)
    lat.set_gauge(random_gauge(5, lat.V))
    lat.set_nd(*FIXTURE)
    N = lat.Vh
    k32 = random_spinor(1, N).astype(np.float32)
    s32 = np.full((N, 4, 3, 2), 7.0, dtype=np.float32)
    s64 = np.full((N, 4, 3, 2), 7.0)
    ks, kc, ls, lc = lat.field32(k32), lat.field32(k32), lat.field32(s32), lat.field32(s32)
    qu, qd, pu, pd = lat.field(random_spinor(2, N)), lat.field(random_spinor(3, N)), lat.field(s64), lat.field(s64)
    lat.set_loopback(1)
    try:
        calls = {"Qtm_pm_ndpsi_32": lambda: lat.Qtm_pm_ndpsi_32(ls, lc, ks, kc),
                 "M_ee_inv_ndpsi_32": lambda: lat.M_ee_inv_ndpsi_32(ls, lc, ks, kc, 0.1, 0.1),
                 "M_oo_sub_g5_ndpsi_32": lambda: lat.M_oo_sub_g5_ndpsi_32(ls, lc, ks, kc, ks, kc, 0.1, 0.1),
                 "rg_mixed_cg_her_nd": lambda: lat.rg_mixed_cg_her_nd(pu, pd, qu, qd, 100, 1e-20, 1, N, delta=0.1)}
        for name, call in calls.items():
            capfd.readouterr()
            with pytest.raises(TmHipError):
                call()
            assert "%s: the fp32 doublet runs on unsplit lattices only" % name in capfd.readouterr().err, name
    finally:
        lat.set_loopback(0)
    assert np.array_equal(ls.download(), s32) and np.array_equal(lc.download(), s32)
    assert np.array_equal(pu.download(), s64) and np.array_equal(pd.download(), s64)
    lat.close()
