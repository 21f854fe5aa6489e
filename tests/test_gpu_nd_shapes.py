"""GPU: the non-degenerate doublet (nd.hip) against oracle/nd_restate.py over the CPU oracle's Hopping_Matrix, on
non-hypercubic lattices with twisted boundary phases, at the parameters and launch forms where the doublet kernels can go
wrong.  tests/test_nd_restate.py pins the restatement to the reference's own outputs.

* operators: every doublet entry point on small, ragged and padded-XCD-grid shapes, theta = (1, 0.3, -0.2, 0.5), four
  (mubar, epsbar) points, both forms ("nd_fused" 1 / 0), every "xcd" and "gauge_cache" form on the padded shapes, and l == k;
* solvers: cg_mms_tm_nd (1, 5 and 32 shifts, an unsorted set, rel_prec 0 / 1 / -1, a run to max_iter) and cg_her_nd (zero
  and non-zero start, rel_prec 0 / 1 / 2) against the restated solvers, and the same results for every polling interval.
"""
import numpy as np
import pytest

from oracle import nd_restate as nd
from tests.util import TOL, random_gauge, random_spinor

pytestmark = pytest.mark.gpu

KAPPA = 0.13
THETA = (1.0, 0.3, -0.2, 0.5)
FIXTURE = (0.1375, 0.1175, 0.6931)                                    # (mubar, epsbar, invmaxev) of tests/golden/ref_nd_*
PARAMS = [FIXTURE, (0.1375, 0.0, 0.6931), (0.0, 0.1175, 0.6931),
          (0.1375, float(np.sqrt(0.95 + 0.1375 ** 2)), 0.6931)]        # the last: 1 + mubar^2 - epsbar^2 = 0.05
SMALL = [(2, 2, 2, 2), (4, 2, 6, 2), (6, 10, 2, 4), (24, 4, 4, 4), (4, 4, 4, 16)]
XCD = [((10, 10, 6, 14), 0), ((18, 12, 12, 14), 256)]                 # (shape, "block"): the padded XCD grid of nd_launch_hop
SHAPES = [(s, 0) for s in SMALL] + XCD
OPS = ("Qtm_ndpsi", "Qtm_dagger_ndpsi", "Qtm_pm_ndpsi")
OUTS = OPS + ("M_ee_inv_ndpsi", "M_oo_sub_g5_ndpsi", "H_eo_tm_ndpsi_0", "H_eo_tm_ndpsi_1")


def _pair_err(a, b, ra, rb):
    num = np.sqrt(np.sum((a - ra) ** 2) + np.sum((b - rb) ** 2))
    return num / np.sqrt(np.sum(ra ** 2) + np.sum(rb ** 2))


def _grid(Vh, block):
    """nd_launch_hop: block size (tmhip_hop_block), blocks, blocks of the XCD-remapped grid (padded to a multiple of 8)."""
    bs = block or (64 if Vh < 131072 else 256)
    nb = (Vh + bs - 1) // bs
    return bs, nb, (8 * ((nb + 7) // 8) if nb >= 64 else nb)


def test_xcd_shapes_take_the_padded_grid():
    """The premise of the XCD cases: a remapped grid with padding blocks and a partial last wave."""
    for (T, LX, LY, LZ), block in XCD:
        Vh = T * LX * LY * LZ // 2
        bs, nb, padded = _grid(Vh, block)
        assert nb >= 64 and nb % 8 != 0 and padded > nb, (T, LX, LY, LZ, nb)
        assert Vh % 64 != 0, Vh
    assert (10 * 10 * 6 * 14 // 2, (14 // 2) % 2) == (4200, 1)        # odd LZh
    assert _grid(4200, 0)[1:] == (66, 72) and _grid(18144, 256)[1:] == (71, 72)


class _Setup:
    """One lattice on both sides: the same gauge, kappa and theta for the oracle and the device."""

    def __init__(self, shape, block):
        from oracle.oraclebind import Oracle
        from tmlqcd_amd import Lattice
        self.shape, self.block = shape, block
        self.orc = Oracle(*shape, kappa=KAPPA, mu=0.0, theta=THETA, threads=8)
        self.lat = Lattice(*shape, kappa=KAPPA, mu=0.0, theta=THETA)
        seed = 1000 + sum(shape) * 7 + shape[0]
        g = random_gauge(seed, self.orc.VPR)
        self.orc.set_gauge(g)
        self.lat.set_gauge(g)
        if block:
            self.lat.set_option("block", block)
        self.N = self.orc.Vh
        self.H = nd.hop_over(self.orc.Hopping_Matrix, self.N)
        self.k = [random_spinor(seed + i, self.N) for i in range(1, 6)]   # k_s, k_c, j_s, j_c, a start vector
        self.refs = {}

    def qpm(self, prm):
        mb, eb, c = prm
        return lambda u, d: nd.Qtm_pm_ndpsi(self.H, u, d, mb, eb, c)

    def operators(self, prm):
        """The restated outputs (float64 pairs) of every entry point on (k_s, k_c) (and j_s, j_c)."""
        if prm not in self.refs:
            mb, eb, c = prm
            H = self.H
            ks, kc, js, jc = (nd.cplx(a) for a in self.k[:4])
            out = {"Qtm_ndpsi": nd.Qtm_ndpsi(H, ks, kc, mb, eb, c), "Qtm_dagger_ndpsi": nd.Qtm_dagger_ndpsi(H, ks, kc, mb, eb, c),
                   "Qtm_pm_ndpsi": nd.Qtm_pm_ndpsi(H, ks, kc, mb, eb, c), "M_ee_inv_ndpsi": nd.m_ee_inv(ks, kc, mb, eb),
                   "M_oo_sub_g5_ndpsi": nd.m_oo_sub_g5(ks, kc, js, jc, mb, eb),
                   "H_eo_tm_ndpsi_0": nd.H_eo_tm_ndpsi(H, ks, kc, 0, mb, eb), "H_eo_tm_ndpsi_1": nd.H_eo_tm_ndpsi(H, ks, kc, 1, mb, eb)}
            self.refs[prm] = {k: (nd.real(a), nd.real(b)) for k, (a, b) in out.items()}
        return self.refs[prm]

    def device_operators(self, prm):
        lat = self.lat
        mb, eb, c = prm
        lat.set_nd(mb, eb, c)
        ks, kc, js, jc = (lat.field(a) for a in self.k[:4])
        ls, lc = lat.field(), lat.field()
        out = {}
        for name in OPS:
            getattr(lat, name)(ls, lc, ks, kc)
            out[name] = (ls.download(), lc.download())
        lat.M_ee_inv_ndpsi(ls, lc, ks, kc, mb, eb)
        out["M_ee_inv_ndpsi"] = (ls.download(), lc.download())
        lat.M_oo_sub_g5_ndpsi(ls, lc, ks, kc, js, jc, mb, eb)
        out["M_oo_sub_g5_ndpsi"] = (ls.download(), lc.download())
        for ieo in (0, 1):
            lat.H_eo_tm_ndpsi(ls, lc, ks, kc, ieo)
            out["H_eo_tm_ndpsi_%d" % ieo] = (ls.download(), lc.download())
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
    errs = {k: _pair_err(*got[k], *ref[k]) for k in OUTS}
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, (st.shape, tag, prm, errs)


# ---------------------------------------------------------------- operators
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("prm", PARAMS, ids=["fixture", "epsbar0", "mubar0", "nrm20"])
@pytest.mark.parametrize("shape,block", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "b%d" % v)
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
    """l == k: allowed by tm_operators_nd.c:190 for Qtm_pm_ndpsi; H_eo_tm_ndpsi hops into scratch first as well."""
    st = setup((6, 10, 2, 4))
    lat = st.lat
    lat.set_nd(*FIXTURE)
    lat.set_option("nd_fused", fused)
    ref = st.operators(FIXTURE)
    try:
        for name in ("Qtm_pm_ndpsi", "H_eo_tm_ndpsi_0", "H_eo_tm_ndpsi_1"):
            ks, kc = lat.field(st.k[0]), lat.field(st.k[1])
            if name == "Qtm_pm_ndpsi":
                lat.Qtm_pm_ndpsi(ks, kc, ks, kc)
            else:
                lat.H_eo_tm_ndpsi(ks, kc, ks, kc, int(name[-1]))
            assert _pair_err(ks.download(), kc.download(), *ref[name]) < TOL, name
            ks.free(); kc.free()
    finally:
        lat.set_option("nd_fused", 1)


# ---------------------------------------------------------------- solvers
SOLVE = [((6, 10, 2, 4), 0)] + XCD
SOLVE_IDS = ["6x10x2x4", "10x10x6x14", "18x12x12x14_b256"]
FIVE = [0.02, 0.15, 0.6, 2.5, 9.0]
# name: (shifts, max_iter, eps_sq, rel_prec)
MMS = {
    "one_shift": ([0.1], 1000, 1e-20, 1),
    "five_sorted": (FIVE, 1000, 1e-22, 0),
    "thirty_two": (list(np.logspace(-2, 1, 32)), 25, 1e-22, 0),
    "unsorted": ([0.15, 0.02, 0.6, 2.5], 1000, 1e-20, 1),
    "rel_prec_negative": ([0.05, 0.5], 30, 1e-10, -1),
    "max_iter": ([0.02, 0.15, 0.6], 12, 1e-22, 0),
}


def _target(eps_sq, rel_prec, squarenorm):
    return eps_sq * squarenorm if rel_prec > 0 else eps_sq


def _mms_reference(st, name):
    key = ("mms", name)
    if key not in st.refs:
        shifts, max_iter, eps_sq, rel = MMS[name]
        ks, kc = nd.cplx(st.k[0]), nd.cplx(st.k[1])
        st.refs[key] = nd.cg_mms_tm_nd(st.qpm(FIXTURE), ks, kc, shifts, max_iter, eps_sq, rel)
    return st.refs[key]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", list(MMS))
@pytest.mark.parametrize("shape,block", SOLVE, ids=SOLVE_IDS)
def test_cg_mms_tm_nd_matches_restatement(setup, shape, block, name, fused):
    st = setup(shape, block)
    shifts, max_iter, eps_sq, rel = MMS[name]
    it_ref, P_ref, drops, left = _mms_reference(st, name)
    # the premises of the cases
    if name == "five_sorted":
        assert len(drops) >= 2 and it_ref > 0, (it_ref, drops)
    if name in ("thirty_two", "rel_prec_negative", "max_iter"):
        assert it_ref == -1
    if name == "unsorted":
        assert min(shifts) < shifts[0] and it_ref > 0
    if name == "rel_prec_negative":   # with rel_prec 0 the same run stops early: a device that does so for rel_prec < 0 fails
        ks, kc = nd.cplx(st.k[0]), nd.cplx(st.k[1])
        assert 0 < nd.cg_mms_tm_nd(st.qpm(FIXTURE), ks, kc, shifts, max_iter, eps_sq, 0)[0] < max_iter
    lat = st.lat
    lat.set_nd(*FIXTURE)
    lat.set_option("nd_fused", fused)
    qs, qc = lat.field(st.k[0]), lat.field(st.k[1])
    try:
        it, P = lat.cg_mms_tm_nd(qs, qc, shifts, max_iter, eps_sq, rel)
        active = lat.nd_active_shifts()
        got = [(u.download(), d.download()) for u, d in P]
        for u, d in P:
            u.free(); d.free()
    finally:
        qs.free(); qc.free()
        lat.set_option("nd_fused", 1)
    if it_ref == -1:
        assert it == -1, it
    else:
        assert it > 0 and abs(it - it_ref) <= 1, (it, it_ref)
    assert active == left, (active, left, drops)
    tol = 1e-10 if it_ref == -1 else 1e-9
    for s, ((u, d), (ru, rd)) in enumerate(zip(got, P_ref)):
        e = _pair_err(u, d, nd.real(ru), nd.real(rd))
        assert e < tol, (s, shifts[s], e)
    if it_ref > 0:   # the true residual of the base system
        ks, kc = nd.cplx(st.k[0]), nd.cplx(st.k[1])
        xu, xd = nd.cplx(got[0][0]), nd.cplx(got[0][1])
        au, ad = st.qpm(FIXTURE)(xu, xd)
        s0 = shifts[0] ** 2
        res = np.vdot(au + s0 * xu - ks, au + s0 * xu - ks).real + np.vdot(ad + s0 * xd - kc, ad + s0 * xd - kc).real
        squarenorm = np.vdot(ks, ks).real + np.vdot(kc, kc).real
        assert res <= 10 * _target(eps_sq, rel, squarenorm), (res, _target(eps_sq, rel, squarenorm))


# name: (start, max_iter, eps_sq, rel_prec); start: a random start vector instead of zero
HER = {
    "zero_start_rel1": (False, 1000, 1e-20, 1),
    "zero_start_rel0": (False, 1000, 1e-16, 0),
    "start_rel1": (True, 1000, 1e-20, 1),
    "rel_prec2": (False, 15, 1e-20, 2),     # cg_her_nd.c:132 never converges: -1 after max_iter
}


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", list(HER))
@pytest.mark.parametrize("shape,block", SOLVE, ids=SOLVE_IDS)
def test_cg_her_nd_matches_restatement(setup, shape, block, name, fused):
    st = setup(shape, block)
    start, max_iter, eps_sq, rel = HER[name]
    ks, kc = nd.cplx(st.k[0]), nd.cplx(st.k[1])
    x0 = 0.1 * st.k[4] if start else np.zeros_like(st.k[4])
    x0u, x0d = nd.cplx(x0), nd.cplx(x0[::-1].copy())
    key = ("her", name)
    if key not in st.refs:
        st.refs[key] = nd.cg_her_nd(st.qpm(FIXTURE), x0u, x0d, ks, kc, max_iter, eps_sq, rel)
    it_ref, ru, rd = st.refs[key]
    assert (it_ref == -1) == (name == "rel_prec2"), it_ref
    lat = st.lat
    lat.set_nd(*FIXTURE)
    lat.set_option("nd_fused", fused)
    qs, qc = lat.field(st.k[0]), lat.field(st.k[1])
    pu, pd = lat.field(nd.real(x0u)), lat.field(nd.real(x0d))
    try:
        it = lat.cg_her_nd(pu, pd, qs, qc, max_iter, eps_sq, rel, lat.Vh)
        u, d = pu.download(), pd.download()
    finally:
        for f in (qs, qc, pu, pd):
            f.free()
        lat.set_option("nd_fused", 1)
    if it_ref == -1:
        assert it == -1, it
        assert _pair_err(u, d, nd.real(ru), nd.real(rd)) < 1e-10
        return
    assert it > 0 and abs(it - it_ref) <= 1, (it, it_ref)
    assert _pair_err(u, d, nd.real(ru), nd.real(rd)) < 1e-9
    xu, xd = nd.cplx(u), nd.cplx(d)
    au, ad = st.qpm(FIXTURE)(xu, xd)
    res = np.vdot(au - ks, au - ks).real + np.vdot(ad - kc, ad - kc).real
    squarenorm = np.vdot(ks, ks).real + np.vdot(kc, kc).real
    assert res <= 10 * _target(eps_sq, rel, squarenorm), res


@pytest.mark.parametrize("fused", [1, 0])
def test_polling_interval_does_not_change_the_result(setup, fused):
    """The solver engine polls `done` every cg_batch iterations; what it enqueues after `done` must change nothing."""
    st = setup(*XCD[0])
    lat = st.lat
    lat.set_nd(*FIXTURE)
    lat.set_option("nd_fused", fused)
    qs, qc = lat.field(st.k[0]), lat.field(st.k[1])
    runs = {}
    try:
        for batch in (1, 4, 7):
            lat.set_option("cg_batch", batch)
            for name in ("five_sorted", "rel_prec_negative"):
                shifts, max_iter, eps_sq, rel = MMS[name]
                it, P = lat.cg_mms_tm_nd(qs, qc, shifts, max_iter, eps_sq, rel)
                runs[(batch, name)] = (it, lat.nd_active_shifts(), [(u.download(), d.download()) for u, d in P])
                for u, d in P:
                    u.free(); d.free()
            pu, pd = lat.field().zero(), lat.field().zero()
            it = lat.cg_her_nd(pu, pd, qs, qc, 1000, 1e-20, 1, lat.Vh)
            runs[(batch, "her")] = (it, 1, [(pu.download(), pd.download())])
            pu.free(); pd.free()
    finally:
        qs.free(); qc.free()
        lat.set_option("cg_batch", 4)
        lat.set_option("nd_fused", 1)
    for name in ("five_sorted", "rel_prec_negative", "her"):
        it1, act1, x1 = runs[(1, name)]
        for batch in (4, 7):
            it, act, x = runs[(batch, name)]
            assert (it, act) == (it1, act1), (name, batch, it, it1)
            for (u, d), (u1, d1) in zip(x, x1):
                assert np.array_equal(u, u1) and np.array_equal(d, d1), (name, batch)
