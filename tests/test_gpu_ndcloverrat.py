"""GPU: the clover rational monomial (type NDCLOVERRAT of monomial/ndrat_monomial.c; rational.hip) and sw_deriv_nd against the
statements restated over the CPU oracle (tests/ndsw_restate.py: deriv_Sb, sw_spinor_eo, sw_all from oracle/tm_oracle.c), on 4^4
and a ragged shape; the refusals; one molecular-dynamics trajectory with everything resident; the drop-in symbols on host arrays.
tests/test_ndsw_restate.py pins the restatement to the reference's own outputs."""
import numpy as np
import pytest

from tests import ndsw_restate as sw
from tests.hostprog import run_child
from tests.util import TOL, random_gauge, random_spinor, rel_err
from tmlqcd_amd import synthetic as syn

pytestmark = pytest.mark.gpu

KAPPA, C_SW, THETA = sw.KAPPA, sw.C_SW, sw.THETA
MUBAR, EPSBAR, INVMAXEV = sw.FIXTURE
MSHIFT = MUBAR * MUBAR - EPSBAR * EPSBAR
SHAPES = sw.FORCE_SHAPES
MU3, RMU3 = [0.21, 0.6, 1.7], [0.05, 0.4, 1.3]
NU3, RNU3 = [0.15, 0.5, 1.4], [0.04, 0.3, 0.9]
SOLVE = (2000, 1e-24, 1)


def pair(shape, seed=None):
    """One lattice on both sides with the clover term and the doublet's inverse computed on each side from the links."""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    orc = Oracle(*shape, kappa=KAPPA, mu=0.0, theta=THETA, threads=8)
    lat = Lattice(*shape, kappa=KAPPA, mu=0.0, theta=THETA)
    g = random_gauge(seed if seed is not None else sw.shape_seed(shape), orc.VPR)
    orc.set_gauge(g)
    lat.set_gauge(g)
    lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
    lat.sw_term(g, KAPPA, C_SW)
    lat.sw_invert_nd(MSHIFT)
    assert lat.sw_invert_failures() == 0
    cl = sw.clover_of(orc, KAPPA, C_SW)
    cl.sw_invert_nd(MSHIFT)
    assert cl.fails == 0 and cl.cond(MSHIFT) < sw.COND_MAX
    return orc, lat, cl, g


@pytest.mark.parametrize("shape", SHAPES, ids=["4x4x4x4", "6x4x2x8"])
def test_sw_deriv_nd_against_the_restatement(shape):
    orc, lat, cl, g = pair(shape)
    swm, swp = np.zeros((orc.V, 4, 3, 3, 2)), np.zeros((orc.V, 4, 3, 3, 2))
    sw.sw_deriv_nd(cl, sw.EE, swm, swp)
    lat.swpm_zero()
    lat.sw_deriv_nd(0)
    gm, gp = lat.get_swpm()
    assert rel_err(gm, swm) < TOL and rel_err(gp, swp) < TOL
    lat.sw_deriv_nd(0)                                                  # it accumulates
    gm2, gp2 = lat.get_swpm()
    assert rel_err(gm2, 2 * swm) < TOL and rel_err(gp2, 2 * swp) < TOL
    lat.close()


@pytest.mark.parametrize("np_", [1, 3, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=["4x4x4x4", "6x4x2x8"])
def test_force_against_the_restatement(shape, np_):
    """ndcloverrat_force with and without the tr-log term, at "rat_batch" 1 / 2 / np; the tolerance of tests/test_gpu_rat.py's ndrat_force."""
    orc, lat, cl, g = pair(shape)
    N = lat.Vh
    rng = np.random.default_rng(5 + np_)
    mu, rmu = list(rng.uniform(0.02, 2.0, np_)), list(rng.standard_normal(np_))
    hu, hd = [random_spinor(400 + j, N) for j in range(np_)], [random_spinor(500 + j, N) for j in range(np_)]
    chi = [(lat.field(a), lat.field(b)) for a, b in zip(hu, hd)]
    m = sw.NdCloverRat(orc, cl, MUBAR, EPSBAR)
    cchi = [(sw.cplx(a), sw.cplx(b)) for a, b in zip(hu, hd)]
    for trlog in (0, 1):
        want = np.zeros((orc.VPR, 4, 8))
        m.force(cchi, mu, rmu, INVMAXEV, KAPPA, C_SW, trlog, want)
        got = {}
        for batch in (1, 2, np_):
            lat.set_option("rat_batch", batch)
            lat.derivative_zero()
            lat.ndcloverrat_force(chi, mu, rmu, INVMAXEV, KAPPA, C_SW, trlog)
            got[batch] = lat.derivative()
            assert rel_err(got[batch], want[:orc.V]) < TOL, (trlog, batch)
        for batch in (2, np_):                                          # the same force up to rounding
            assert rel_err(got[batch], got[1]) < TOL
    for (a, b), (fa, fb) in zip(zip(hu, hd), chi):
        assert np.array_equal(fa.download(), a) and np.array_equal(fb.download(), b)
    lat.close()


def test_drivers_against_the_restatement():
    orc, lat, cl, g = pair(sw.DRIVER_SHAPE)
    N = lat.Vh
    hu, hd = random_spinor(21, N), random_spinor(22, N)
    pu, pd = lat.field(hu), lat.field(hd)
    m = sw.NdCloverRat(orc, cl, MUBAR, EPSBAR)
    # derivative = solve + force
    it0, P = lat.cg_mms_tm_nd(pu, pd, MU3, *SOLVE, op="Qsw_pm_ndpsi")
    assert it0 > 0
    chi = [(sw.cplx(a.download()), sw.cplx(b.download())) for a, b in P]
    lat.derivative_zero()
    assert lat.ndcloverrat_derivative(pu, pd, MU3, RMU3, INVMAXEV, KAPPA, C_SW, 1, *SOLVE) == it0
    got = lat.derivative()
    want = np.zeros((orc.VPR, 4, 8))
    m.force(chi, MU3, RMU3, INVMAXEV, KAPPA, C_SW, 1, want)
    assert rel_err(got, want[:orc.V]) < TOL
    lat.derivative_zero()
    lat.ndcloverrat_force(P, MU3, RMU3, INVMAXEV, KAPPA, C_SW, 1)
    assert np.array_equal(lat.derivative(), got)
    # acceptance
    e1, it = lat.ndcloverrat_acc(pu, pd, MU3, RMU3, *SOLVE)
    assert it == it0
    w1 = m.acc(sw.cplx(hu), sw.cplx(hd), chi, RMU3)
    assert abs(e1 - w1) < TOL * abs(w1)
    # heatbath
    it0, P = lat.cg_mms_tm_nd(pu, pd, NU3, *SOLVE, P=P, op="Qsw_pm_ndpsi")
    chi = [(sw.cplx(a.download()), sw.cplx(b.download())) for a, b in P]
    e0, it = lat.ndcloverrat_heatbath(pu, pd, NU3, RNU3, INVMAXEV, *SOLVE)
    assert it == it0
    w0, wu, wd = m.heatbath(sw.cplx(hu), sw.cplx(hd), chi, NU3, RNU3, INVMAXEV)
    assert abs(e0 - w0) < TOL * w0
    assert rel_err(pu.download(), sw.real(wu)) < TOL and rel_err(pd.download(), sw.real(wd)) < TOL
    lat.close()


def test_refusals_leave_the_accumulator_alone():
    """T-split context, loopback rehearsal, sw_inv_nd not valid, np outside [1, 32]: refused before any launch."""
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    orc, lat, cl, g = pair((4, 4, 4, 4))
    N = lat.Vh
    a, b = lat.field(random_spinor(1, N)), lat.field(random_spinor(2, N))
    lat.derivative_zero()
    lat.deriv_Sb(1, a, b, 0.8)
    before = lat.derivative()
    lat.swpm_zero()
    lat.sw_spinor_eo(0, a, b, 0.3)
    swpm_before = lat.get_swpm()

    def refused(call, what):
        with pytest.raises(TmHipError):
            call()
        assert np.array_equal(lat.derivative(), before), what
        gm, gp = lat.get_swpm()
        assert np.array_equal(gm, swpm_before[0]) and np.array_equal(gp, swpm_before[1]), what

    force = lambda n: lat.ndcloverrat_force([(a, b)] * n, [0.1] * n, [0.5] * n, INVMAXEV, KAPPA, C_SW, 1)
    refused(lambda: force(0), "np = 0")
    refused(lambda: force(33), "np = 33")
    refused(lambda: lat.ndcloverrat_derivative(a, b, [0.1] * 33, [0.5] * 33, INVMAXEV, KAPPA, C_SW, 1, *SOLVE), "np = 33, derivative")
    refused(lambda: lat.ndcloverrat_acc(a, b, [], [], *SOLVE), "np = 0, acc")
    refused(lambda: lat.ndcloverrat_heatbath(a, b, [0.1] * 33, [0.5] * 33, INVMAXEV, *SOLVE), "np = 33, heatbath")
    lat.set_loopback(1)
    try:
        refused(lambda: force(1), "loopback")
        refused(lambda: lat.ndcloverrat_derivative(a, b, MU3, RMU3, INVMAXEV, KAPPA, C_SW, 1, *SOLVE), "loopback, derivative")
        refused(lambda: lat.Qsw_tau1_sub_const_ndpsi(lat.field(), lat.field(), a, b, 0.1j, 1.0, 1.0), "loopback, operator")
    finally:
        lat.set_loopback(0)
    lat.sw_term(g, KAPPA, C_SW)                                         # a new clover term: sw_inv_nd is no longer valid
    refused(lambda: force(1), "sw_inv_nd not valid")
    refused(lambda: lat.ndcloverrat_derivative(a, b, MU3, RMU3, INVMAXEV, KAPPA, C_SW, 1, *SOLVE), "sw_inv_nd not valid, derivative")
    refused(lambda: lat.ndcloverrat_acc(a, b, MU3, RMU3, *SOLVE), "sw_inv_nd not valid, acc")
    refused(lambda: lat.sw_deriv_nd(0), "sw_inv_nd not valid, sw_deriv_nd")
    lat.sw_invert_nd(MSHIFT)
    assert lat.sw_invert_failures() == 0
    force(1)                                                            # and a legal call goes through
    assert not np.array_equal(lat.derivative(), before)
    lat.close()
    # a T-split context
    split = Lattice(2, 4, 4, 4, nproc_t=2, proc_t=0, kappa=KAPPA)
    gs = syn.gauge_field(6, 2, 4, 4, 4, 2, 0)
    split.set_gauge(gs)                                                 # refused for the split alone, whatever the clover state
    split.derivative_zero()
    fa, fb = split.field(), split.field()
    with pytest.raises(TmHipError):
        split.ndcloverrat_force([(fa, fb)], [0.1], [0.5], INVMAXEV, KAPPA, C_SW, 1)
    with pytest.raises(TmHipError):
        split.Qsw_pm_ndpsi(split.field(), split.field(), fa, fb)
    assert not split.derivative().any()
    split.close()


# ---------------------------------------------------------------- the force is the derivative of the action
class NdCloverRatTrajectory:
    """H = p^2 / 2 + pf . (pf + sum_j rmu_j chi_j) - sum_even log det((1+T)^2 + mubar^2 - epsbar^2): ndcloverrat_acc with pf fixed, the
    tr-log on the host from tmhip_get_clover; force = ndcloverrat_derivative with trlog set; sw_term + sw_invert_nd from the moving links.
    Lattice size and step sizes of tests/test_gpu_md_trajectory.py and the rational trajectories of tests/test_gpu_rat.py."""
    MU, RMU = [0.4, 0.9, 2.0], [0.3, 0.8, 1.5]
    SOLVE = (2000, 1e-26, 1)
    MB, EB, INV = 0.12, 0.1, 0.6

    def __init__(self, L=8, kappa=0.125, c_sw=1.2, seed=5):
        from tmlqcd_amd import Lattice
        self.kappa, self.c_sw = kappa, c_sw
        self.lat = lat = Lattice(L, L, L, L, kappa=kappa, mu=0.0)
        lat.set_nd(self.MB, self.EB, self.INV)
        self.shift = self.MB ** 2 - self.EB ** 2
        self.g0 = syn.gauge_field(seed, L, L, L, L)
        self.p0 = np.random.default_rng(seed + 1).standard_normal((lat.V, 4, 8))
        self.reset()
        self.pf = [lat.field(syn.spinor_field_eo(seed + 2 + q, 1, L, L, L, L)) for q in range(2)]
        self.iters = 0
        c = np.indices((L, L, L, L)).sum(axis=0).reshape(-1)
        self.even = (c & 1) == 0
        self.worst_cond = 0.0

    def reset(self):
        self.lat.set_gauge(self.g0)
        self.lat.momenta_upload(self.p0)

    def clover(self):
        self.lat.sw_term(None, self.kappa, self.c_sw)                   # from the links resident in HBM
        self.lat.sw_invert_nd(self.shift)
        assert self.lat.sw_invert_failures() == 0

    def trlog(self):
        swh, _ = self.lat.get_clover(True, False)
        b = (swh[..., 0] + 1j * swh[..., 1])[self.even]                 # [Vh][3][2][3][3]
        tot = 0.0
        for i in range(2):
            a = np.zeros((b.shape[0], 6, 6), dtype=complex)
            a[:, :3, :3] = b[:, 0, i]; a[:, :3, 3:] = b[:, 1, i]
            a[:, 3:, :3] = np.conj(np.transpose(b[:, 1, i], (0, 2, 1))); a[:, 3:, 3:] = b[:, 2, i]
            m = a @ a + self.shift * np.eye(6)
            self.worst_cond = max(self.worst_cond, float(np.linalg.cond(m).max()))
            tot += np.linalg.slogdet(m)[1].sum()
        return -tot

    def energy(self):
        self.clover()
        s, it = self.lat.ndcloverrat_acc(self.pf[0], self.pf[1], self.MU, self.RMU, *self.SOLVE)
        assert it > 0
        p = self.lat.momenta_download()
        return 0.5 * float((p * p).sum()) + s + self.trlog()

    def force(self, step):
        lat = self.lat
        lat.derivative_zero()
        self.clover()
        it = lat.ndcloverrat_derivative(self.pf[0], self.pf[1], self.MU, self.RMU, self.INV, self.kappa, self.c_sw, 1, *self.SOLVE)
        assert it > 0
        self.iters += it
        lat.update_momenta(step)

    def leapfrog(self, nsteps, eps):
        self.force(0.5 * eps)
        for k in range(nsteps):
            self.lat.update_gauge(eps)
            self.force(eps if k < nsteps - 1 else 0.5 * eps)


def test_trajectory_conserves_its_hamiltonian_to_second_order_and_is_reversible():
    tr = NdCloverRatTrajectory()
    h0 = tr.energy()
    dh = {}
    for nsteps in (4, 8):                                               # trajectory length 0.2
        tr.reset()
        tr.leapfrog(nsteps, 0.2 / nsteps)
        dh[nsteps] = tr.energy() - h0
    p = tr.lat.momenta_download()
    tr.lat.momenta_upload(-p)
    tr.leapfrog(8, 0.2 / 8)
    back = tr.lat.gauge_download()[:tr.lat.V]
    tr.lat.close()
    print("ndcloverrat: H0 = %.6f   dH(eps = 0.05) = %.3e   dH(eps = 0.025) = %.3e   ratio %.2f   CG iterations %d   worst cond %.1f"
          % (h0, dh[4], dh[8], dh[4] / dh[8], tr.iters, tr.worst_cond))
    assert tr.worst_cond < sw.COND_MAX
    assert abs(dh[8]) < abs(dh[4])
    assert 3.0 < dh[4] / dh[8] < 5.5                                    # O(eps^2), the factor tests/test_gpu_md_trajectory.py and test_gpu_rat.py demand
    assert np.abs(back - tr.g0).max() < 1e-10


# ---------------------------------------------------------------- drop-in
@pytest.mark.parametrize("mode", ["coherent", "resident"])
def test_dropin_symbols(mode):
    errs = run_child("ndsw_dropin_child.py", mode)
    assert {"sw_invert_nd_failures", "core_sw_invert_nd_failures", "sw_invert_nd_host_copy", "Qsw_pm_ndpsi", "Qsw_pm_ndpsi_aliased", "cg_mms_tm_nd", "ndcloverrat_derivative"} <= set(errs)
    for k, v in errs.items():
        if k.endswith("_iters"):
            assert v <= 1, (k, v)
        elif k == "ndcloverrat_derivative_held_back" or k.endswith("_failures"):
            assert v == 0.0, (k, v)
        elif k.startswith("cg_"):
            assert v < 1e-9, (k, v)
        else:
            assert v < TOL, (k, v)
