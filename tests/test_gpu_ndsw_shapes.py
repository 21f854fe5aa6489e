"""GPU: the clover doublet (sw_invert_nd, the three site-local functions, the Qsw_*_ndpsi family) against tests/ndsw_restate.py
over the CPU oracle (Hopping_Matrix, sw_term), on the shapes of tests/test_gpu_nd_shapes.py -- small, ragged and the two
padded-XCD-grid shapes with their "block" settings (that file asserts their premise); none is excluded, tests/test_gpu_clover_shapes.py
runs sw_term on all of them or on smaller ones of the same kind.  theta = (1, 0.3, -0.2, 0.5); four (mubar, epsbar) points: the
fixture's, epsbar = 0, mubar = 0 and epsbar > mubar (a negative shift).  tests/test_ndsw_restate.py pins the restatement to the
reference's own outputs and asserts that every 6x6 block inverted here has a condition number below 10^3.

Both forms ("nd_fused" 1 / 0) against the restatement and against each other, l == k, the inverse against the restatement's and
times (1+T)^2 + shift on the device, and the epsbar = 0 reduction to two single-flavour Qsw_pm_psi on the device.
"""
import numpy as np
import pytest

from tests import ndsw_restate as sw
from tests.util import TOL, random_gauge, random_spinor, rel_err

pytestmark = pytest.mark.gpu

KAPPA, C_SW, THETA = sw.KAPPA, sw.C_SW, sw.THETA
Z, CPOL = 0.3 - 0.7j, 1.1
OPS = ("Qsw_ndpsi", "Qsw_dagger_ndpsi", "Qsw_pm_ndpsi", "H_eo_sw_ndpsi", "Msw_ee_inv_ndpsi")
OUTS = OPS + ("Qsw_tau1_sub_const_ndpsi", "assign_mul_one_sw_pm_imu_eps_0", "assign_mul_one_sw_pm_imu_eps_1", "clover_inv_nd",
              "clover_gamma5_nd_0", "clover_gamma5_nd_1")
SHAPE_IDS = ["x".join(map(str, s)) + ("_b%d" % b if b else "") for s, b in sw.SHAPES]


def _pair_err(a, b, ra, rb):
    num = np.sqrt(np.sum((a - ra) ** 2) + np.sum((b - rb) ** 2))
    return num / np.sqrt(np.sum(ra ** 2) + np.sum(rb ** 2))


class _Setup:
    """One lattice on both sides: the same gauge, kappa and theta; the clover term computed on each side from the links."""

    def __init__(self, shape, block):
        from oracle.oraclebind import Oracle
        from tmlqcd_amd import Lattice
        self.shape, self.block = shape, block
        self.orc = Oracle(*shape, kappa=KAPPA, mu=0.0, theta=THETA, threads=8)
        self.lat = Lattice(*shape, kappa=KAPPA, mu=0.0, theta=THETA)
        seed = sw.shape_seed(shape)
        self.gauge = random_gauge(seed, self.orc.VPR)
        self.orc.set_gauge(self.gauge)
        self.lat.set_gauge(self.gauge)
        if block:
            self.lat.set_option("block", block)
        self.lat.sw_term(self.gauge, KAPPA, C_SW)
        self.cl = sw.clover_of(self.orc, KAPPA, C_SW)
        self.N = self.orc.Vh
        self.H = sw.hop_over(self.orc.Hopping_Matrix, self.N)
        self.k = [random_spinor(seed + i, self.N) for i in range(1, 6)]   # k_s, k_c, j_s, j_c, a start vector
        self.refs = {}
        self.point = None

    def at(self, prm):
        """sw_invert_nd(mubar^2 - epsbar^2) on both sides and the doublet's parameters on the device"""
        mb, eb, c = prm
        if self.point != prm:
            self.lat.sw_invert_nd(mb * mb - eb * eb)
            assert self.lat.sw_invert_failures() == 0
            self.inv_host = self.cl.sw_invert_nd(mb * mb - eb * eb)
            assert self.cl.fails == 0
            self.point = prm
        self.lat.set_nd(mb, eb, c)

    def qpm(self, prm):
        mb, eb, c = prm
        self.at(prm)
        return lambda u, d: sw.Qsw_pm_ndpsi(self.cl, self.H, u, d, mb, eb, c)

    def operators(self, prm):
        """The restated outputs (float64 pairs (l_s, l_c)) of every entry point on (k_s, k_c) (and j_s, j_c)."""
        if prm not in self.refs:
            self.at(prm)
            mb, eb, c = prm
            cl, H = self.cl, self.H
            ks, kc, js, jc = (sw.cplx(a) for a in self.k[:4])
            out = {"Qsw_ndpsi": sw.Qsw_ndpsi(cl, H, ks, kc, mb, eb, c), "Qsw_dagger_ndpsi": sw.Qsw_dagger_ndpsi(cl, H, ks, kc, mb, eb, c),
                   "Qsw_pm_ndpsi": sw.Qsw_pm_ndpsi(cl, H, ks, kc, mb, eb, c), "H_eo_sw_ndpsi": sw.H_eo_sw_ndpsi(cl, H, ks, kc, mb, eb),
                   "Msw_ee_inv_ndpsi": sw.Msw_ee_inv_ndpsi(cl, ks, kc, mb, eb),
                   "Qsw_tau1_sub_const_ndpsi": sw.Qsw_tau1_sub_const_ndpsi(cl, H, ks, kc, Z, CPOL, c, mb, eb)}
            for ieo in (0, 1):
                out["assign_mul_one_sw_pm_imu_eps_%d" % ieo] = sw.assign_mul_one_sw_pm_imu_eps(cl, ieo, ks, kc, mb, eb)
                lc, ls = sw.clover_gamma5_nd(cl, ieo, kc, ks, jc, js, mb, -eb)
                out["clover_gamma5_nd_%d" % ieo] = (ls, lc)
            lc, ls = sw.clover_inv_nd(cl, sw.EE, kc, ks)
            out["clover_inv_nd"] = (ls, lc)
            self.refs[prm] = ({k: (sw.real(a), sw.real(b)) for k, (a, b) in out.items()}, self.inv_host.copy())
        return self.refs[prm][0]

    def device_operators(self, prm):
        lat = self.lat
        mb, eb, c = prm
        self.at(prm)
        ks, kc, js, jc = (lat.field(a) for a in self.k[:4])
        ls, lc = lat.field(), lat.field()
        out = {}
        for name in OPS:
            getattr(lat, name)(ls, lc, ks, kc)
            out[name] = (ls.download(), lc.download())
        lat.Qsw_tau1_sub_const_ndpsi(ls, lc, ks, kc, Z, CPOL, c)
        out["Qsw_tau1_sub_const_ndpsi"] = (ls.download(), lc.download())
        for ieo in (0, 1):
            lat.assign_mul_one_sw_pm_imu_eps(ieo, ls, lc, ks, kc, mb, eb)
            out["assign_mul_one_sw_pm_imu_eps_%d" % ieo] = (ls.download(), lc.download())
            lat.clover_gamma5_nd(ieo, lc, ls, kc, ks, jc, js, mb, -eb)
            out["clover_gamma5_nd_%d" % ieo] = (ls.download(), lc.download())
        lat.assign(ls, ks, self.N)
        lat.assign(lc, kc, self.N)
        lat.clover_inv_nd(0, lc, ls)
        out["clover_inv_nd"] = (ls.download(), lc.download())
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
    return got


@pytest.mark.parametrize("prm", list(sw.POINTS.values()), ids=list(sw.POINTS))
@pytest.mark.parametrize("shape,block", sw.SHAPES, ids=SHAPE_IDS)
def test_operators_match_restatement_in_both_forms(setup, shape, block, prm):
    st = setup(shape, block)
    got = {}
    try:
        for fused in (1, 0):
            st.lat.set_option("nd_fused", fused)
            got[fused] = _check_operators(st, prm, {"nd_fused": fused})
    finally:
        st.lat.set_option("nd_fused", 1)
    # the two forms against each other: the same arithmetic per site, apart from the stencil's summation order
    for k in OUTS:
        assert _pair_err(*got[1][k], *got[0][k]) < TOL, (k, shape, prm)


@pytest.mark.parametrize("prm", list(sw.POINTS.values()), ids=list(sw.POINTS))
@pytest.mark.parametrize("shape,block", sw.SHAPES, ids=SHAPE_IDS)
def test_sw_invert_nd_matches_restatement_and_inverts(setup, shape, block, prm):
    st = setup(shape, block)
    st.operators(prm)
    st.at(prm)
    mb, eb, c = prm
    lat = st.lat
    assert lat.sw_invert_failures() == 0
    assert rel_err(lat.get_clover_nd(), st.refs[prm][1]) < TOL
    # ((1+T)^2 + shift) sw_inv_nd x = x on the device: clover_inv_nd, two assign_mul_one_sw_pm_imu_eps at mu = eps = 0, the shift
    xs, xc = lat.field(st.k[0]), lat.field(st.k[1])
    ys, yc, zs, zc = lat.field(st.k[0]), lat.field(st.k[1]), lat.field(), lat.field()
    try:
        lat.clover_inv_nd(0, yc, ys)
        lat.assign_mul_one_sw_pm_imu_eps(0, zs, zc, ys, yc, 0.0, 0.0)
        lat.assign_mul_one_sw_pm_imu_eps(0, zs, zc, zs, zc, 0.0, 0.0)
        lat.assign_add_mul_r(zs, ys, mb * mb - eb * eb, st.N)
        lat.assign_add_mul_r(zc, yc, mb * mb - eb * eb, st.N)
        assert _pair_err(zs.download(), zc.download(), st.k[0], st.k[1]) < TOL
    finally:
        for f in (xs, xc, ys, yc, zs, zc):
            f.free()


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("shape,block", sw.XCD, ids=["10x10x6x14", "18x12x12x14_b256"])
def test_operators_in_every_xcd_and_gauge_cache_form(setup, shape, block, fused):
    st = setup(shape, block)
    lat = st.lat
    lat.set_option("nd_fused", fused)
    try:
        for xcd in (0, 1, 3, 4):
            for gc in (0, 1):
                lat.set_option("xcd", xcd)
                lat.set_option("gauge_cache", gc)
                _check_operators(st, sw.FIXTURE, {"nd_fused": fused, "xcd": xcd, "gauge_cache": gc})
    finally:
        lat.set_option("xcd", 2)
        lat.set_option("gauge_cache", -1)
        lat.set_option("nd_fused", 1)


@pytest.mark.parametrize("fused", [1, 0])
def test_output_may_alias_input(setup, fused):
    """l == k: allowed for Qsw_pm_ndpsi (tm_operators_nd.c:190); H_eo_sw_ndpsi hops into scratch first; the site-local ones run in place."""
    st = setup((6, 10, 2, 4))
    lat = st.lat
    ref = st.operators(sw.FIXTURE)
    st.at(sw.FIXTURE)
    mb, eb, c = sw.FIXTURE
    lat.set_option("nd_fused", fused)
    try:
        for name in ("Qsw_pm_ndpsi", "H_eo_sw_ndpsi", "Msw_ee_inv_ndpsi", "assign_mul_one_sw_pm_imu_eps_1"):
            ks, kc = lat.field(st.k[0]), lat.field(st.k[1])
            if name == "assign_mul_one_sw_pm_imu_eps_1":
                lat.assign_mul_one_sw_pm_imu_eps(1, ks, kc, ks, kc, mb, eb)
            else:
                getattr(lat, name)(ks, kc, ks, kc)
            assert _pair_err(ks.download(), kc.download(), *ref[name]) < TOL, name
            ks.free(); kc.free()
    finally:
        lat.set_option("nd_fused", 1)


@pytest.mark.parametrize("shape,block", [((6, 10, 2, 4), 0), sw.XCD[0]], ids=["6x10x2x4", "10x10x6x14"])
def test_epsbar_zero_is_two_single_flavour_operators(setup, shape, block):
    """epsbar = 0: Qsw_pm_ndpsi on (k, k') is Qsw_pm_psi at +mubar on k and at -mubar on k', times invmaxev^2 -- all on the device."""
    st = setup(shape, block)
    prm = sw.POINTS["epsbar0"]
    mb, eb, c = prm
    assert eb == 0.0
    lat = st.lat
    st.at(prm)
    ks, kc, ls, lc, t = lat.field(st.k[0]), lat.field(st.k[1]), lat.field(), lat.field(), lat.field()
    try:
        lat.Qsw_pm_ndpsi(ls, lc, ks, kc)
        nd_s, nd_c = ls.download(), lc.download()
        single = []
        for sign, k in ((+1, ks), (-1, kc)):
            lat.set_mu(sign * mb)
            lat.sw_invert(0, sign * mb)
            assert lat.sw_invert_failures() == 0
            lat.op("Qsw_pm_psi", t, k)
            lat.mul_r(t, c * c, t, st.N)
            single.append(t.download())
        assert _pair_err(nd_s, nd_c, single[0], single[1]) < TOL
        # cloverdet's inverse and the doublet's live side by side: the doublet still runs without inverting again
        lat.Qsw_pm_ndpsi(ls, lc, ks, kc)
        assert np.array_equal(ls.download(), nd_s) and np.array_equal(lc.download(), nd_c)
    finally:
        lat.set_mu(0.0)
        for f in (ks, kc, ls, lc, t):
            f.free()


def test_refusals(setup):
    """Not valid / not unsplit: refused with a message before any launch, the outputs untouched."""
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    st = setup((4, 2, 6, 2))
    shape = st.shape
    lat = Lattice(*shape, kappa=KAPPA, mu=0.0, theta=THETA)
    try:
        lat.set_gauge(st.gauge)
        lat.set_nd(*sw.FIXTURE)
        ks, kc = lat.field(st.k[0]), lat.field(st.k[1])
        ls, lc = lat.field(st.k[2]), lat.field(st.k[3])

        def refused(call):
            with pytest.raises(TmHipError):
                call()
            assert np.array_equal(ls.download(), st.k[2]) and np.array_equal(lc.download(), st.k[3])
        refused(lambda: lat.Qsw_pm_ndpsi(ls, lc, ks, kc))                   # no clover term at all
        with pytest.raises(TmHipError):
            lat.sw_invert_nd(sw.REFUSAL_SHIFT)                            # refused: nothing was inverted
        lat.sw_term(st.gauge, KAPPA, C_SW)
        refused(lambda: lat.Qsw_pm_ndpsi(ls, lc, ks, kc))                   # sw_inv_nd not valid
        refused(lambda: lat.H_eo_sw_ndpsi(ls, lc, ks, kc))
        refused(lambda: lat.clover_inv_nd(0, lc, ls))
        with pytest.raises(TmHipError):
            lat.get_clover_nd()
        lat.sw_invert_nd(sw.REFUSAL_SHIFT)
        assert lat.sw_invert_failures() == 0
        lat.Qsw_pm_ndpsi(ls, lc, ks, kc)
        ls.upload(st.k[2]); lc.upload(st.k[3])
        refused(lambda: lat.clover_inv_nd(1, lc, ls))                       # the inverse belongs to the even sites
        lat.sw_term(st.gauge, KAPPA, C_SW)                                  # a new clover term drops the inverse
        refused(lambda: lat.Qsw_pm_ndpsi(ls, lc, ks, kc))
        lat.sw_invert_nd(sw.REFUSAL_SHIFT)
        assert lat.sw_invert_failures() == 0
        lat.set_loopback(1)                                                  # the rehearsal of a T-split run
        try:
            refused(lambda: lat.Qsw_pm_ndpsi(ls, lc, ks, kc))
            refused(lambda: lat.cg_her_nd(ls, lc, ks, kc, 10, 1e-10, 1, lat.Vh, op="Qsw_pm_ndpsi"))
        finally:
            lat.set_loopback(0)
    finally:
        lat.close()
