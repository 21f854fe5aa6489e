"""GPU: the clover rational monomial (type CLOVERRAT of monomial/rat_monomial.c; rational.hip) against the statements restated over
the CPU oracle (tests/cloverrat_restate.py: Qsw_plus_psi, Hopping_Matrix + clover_inv, deriv_Sb, sw_spinor_eo, sw_deriv, sw_all from
oracle/tm_oracle.c), on 4^4 and a ragged shape; the refusals; one molecular-dynamics trajectory with everything resident; the drop-in
symbols on host arrays.  Mirrors tests/test_gpu_ndcloverrat.py."""
import numpy as np
import pytest

from tests import cloverrat_restate as cr
from tests import ndsw_restate as sw
from tests.hostprog import run_child
from tests.util import TOL, random_gauge, random_spinor, rel_err
from tmlqcd_amd import synthetic as syn

pytestmark = pytest.mark.gpu

KAPPA, C_SW, THETA = sw.KAPPA, sw.C_SW, sw.THETA
SHAPES = sw.FORCE_SHAPES
MU3, RMU3 = [0.21, 0.6, 1.7], [0.05, 0.4, 1.3]
NU3, RNU3 = [0.15, 0.5, 1.4], [0.04, 0.3, 0.9]
SOLVE = (2000, 1e-24, 1)
CTX_MU, CTX_MU3 = 0.17, 0.05                                           # the context's own twist: CLOVERRAT runs at 0 and puts it back


def pair(shape, seed=None):
    """One lattice on both sides with the clover term and its even-even inverse at mu = 0 computed on each side from the links."""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    orc = Oracle(*shape, kappa=KAPPA, mu=0.0, theta=THETA, threads=8)
    lat = Lattice(*shape, kappa=KAPPA, mu=CTX_MU, theta=THETA)
    lat.set_mu3(CTX_MU3)
    g = random_gauge(seed if seed is not None else sw.shape_seed(shape), orc.VPR)
    orc.set_gauge(g)
    lat.set_gauge(g)
    lat.sw_term(g, KAPPA, C_SW)
    lat.sw_invert(0, 0.0)
    assert lat.sw_invert_failures() == 0
    m = cr.CloverRat(orc, KAPPA, C_SW)
    assert m.fails == 0
    return orc, lat, m, g


def twist_probe(lat, src):
    """Qtm_plus_psi of a fixed field: depends on the context's mu, bit for bit"""
    out = lat.field()
    lat.op("Qtm_plus_psi", out, src)
    return out.download()


@pytest.mark.parametrize("np_", [1, 3, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=["4x4x4x4", "6x4x2x8"])
def test_force_against_the_restatement(shape, np_):
    """cloverrat_force with and without the tr-log term, at "rat_batch" 1 / 2 / np"""
    orc, lat, m, g = pair(shape)
    N = lat.Vh
    rng = np.random.default_rng(5 + np_)
    rmu = list(rng.standard_normal(np_))
    host = [random_spinor(400 + j, N) for j in range(np_)]
    chi = [lat.field(a) for a in host]
    cchi = [cr.cplx(a) for a in host]
    probe = lat.field(random_spinor(9, N))
    tw = twist_probe(lat, probe)
    for trlog in (0, 1):
        want = np.zeros((orc.VPR, 4, 8))
        m.force(cchi, rmu, trlog, want)
        got = {}
        for batch in (1, 2, np_):
            lat.set_option("rat_batch", batch)
            lat.derivative_zero()
            lat.cloverrat_force(chi, rmu, KAPPA, C_SW, trlog)
            got[batch] = lat.derivative()
            print("cloverrat_force %s np = %d trlog = %d rat_batch = %d: %.2e" % (shape, np_, trlog, batch, rel_err(got[batch], want[:orc.V])))
            assert rel_err(got[batch], want[:orc.V]) < TOL, (trlog, batch)
        for batch in (2, np_):                                          # the same force up to rounding
            assert rel_err(got[batch], got[1]) < TOL
    for a, fa in zip(host, chi):
        assert np.array_equal(fa.download(), a)
    assert np.array_equal(twist_probe(lat, probe), tw)                  # the context's mu is back
    lat.close()


def test_drivers_against_the_restatement():
    orc, lat, m, g = pair(sw.DRIVER_SHAPE)
    N = lat.Vh
    h = random_spinor(21, N)
    pf = lat.field(h)
    probe = lat.field(random_spinor(9, N))
    tw = twist_probe(lat, probe)
    # derivative = solve + force; the solve is cg_mms_tm on Qsw_pm_psi at twisted mass 0
    lat.set_mu(0.0); lat.set_mu3(0.0)
    it0, _, P = lat.cg_mms_tm(pf, MU3, *SOLVE, op="Qsw_pm_psi")
    lat.set_mu(CTX_MU); lat.set_mu3(CTX_MU3)
    assert it0 > 0
    chi = [cr.cplx(a.download()) for a in P]
    lat.derivative_zero()
    assert lat.cloverrat_derivative(pf, MU3, RMU3, KAPPA, C_SW, 1, *SOLVE) == it0
    got = lat.derivative()
    want = np.zeros((orc.VPR, 4, 8))
    m.force(chi, RMU3, 1, want)
    assert rel_err(got, want[:orc.V]) < TOL
    lat.derivative_zero()
    lat.cloverrat_force(P, RMU3, KAPPA, C_SW, 1)
    assert np.array_equal(lat.derivative(), got)                        # bit-equal to the force on those solutions
    assert np.array_equal(twist_probe(lat, probe), tw)
    # acceptance
    e1, it = lat.cloverrat_acc(pf, MU3, RMU3, *SOLVE)
    assert it == it0
    w1 = m.acc(cr.cplx(h), chi, RMU3)
    assert abs(e1 - w1) < TOL * abs(w1)
    assert np.array_equal(twist_probe(lat, probe), tw)
    # heatbath
    lat.set_mu(0.0); lat.set_mu3(0.0)
    it0, _, P = lat.cg_mms_tm(pf, NU3, *SOLVE, op="Qsw_pm_psi", P=P)
    lat.set_mu(CTX_MU); lat.set_mu3(CTX_MU3)
    chi = [cr.cplx(a.download()) for a in P]
    e0, it = lat.cloverrat_heatbath(pf, NU3, RNU3, *SOLVE)
    assert it == it0
    w0, wpf = m.heatbath(cr.cplx(h), chi, NU3, RNU3)
    assert abs(e0 - w0) < TOL * w0
    assert rel_err(pf.download(), cr.real(wpf)) < TOL
    assert np.array_equal(twist_probe(lat, probe), tw)
    lat.close()


def test_refusals_leave_the_accumulator_alone():
    """sw_inv not valid, made for another parity or mu, or uploaded; a stale inverse after update_gauge; np outside [1, 32]; fp32 and full
    fields; loopback rehearsal; T-split context: refused before any launch, the context's mu untouched."""
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    orc, lat, m, g = pair((4, 4, 4, 4))
    N = lat.Vh
    a, b = lat.field(random_spinor(1, N)), lat.field(random_spinor(2, N))
    tw = [twist_probe(lat, a)]
    lat.derivative_zero()
    lat.deriv_Sb(1, a, b, 0.8)
    before = lat.derivative()
    lat.swpm_zero()
    lat.sw_spinor_eo(0, a, b, 0.3)
    swpm_before = lat.get_swpm()
    pf0 = a.download()

    def refused(call, what):
        with pytest.raises(TmHipError):
            call()
        assert np.array_equal(lat.derivative(), before), what
        gm, gp = lat.get_swpm()
        assert np.array_equal(gm, swpm_before[0]) and np.array_equal(gp, swpm_before[1]), what
        assert np.array_equal(a.download(), pf0), what
        assert np.array_equal(twist_probe(lat, a), tw[0]), what

    force = lambda n, f=None: lat.cloverrat_force([f or a] * n, [0.5] * n, KAPPA, C_SW, 1)
    deriv = lambda: lat.cloverrat_derivative(a, MU3, RMU3, KAPPA, C_SW, 1, *SOLVE)

    def all_four(what):
        refused(lambda: force(1), what + ", force")
        refused(deriv, what + ", derivative")
        refused(lambda: lat.cloverrat_acc(a, MU3, RMU3, *SOLVE), what + ", acc")
        refused(lambda: lat.cloverrat_heatbath(a, NU3, RNU3, *SOLVE), what + ", heatbath")

    refused(lambda: force(0), "np = 0")
    refused(lambda: force(33), "np = 33")
    refused(lambda: lat.cloverrat_derivative(a, [0.1] * 33, [0.5] * 33, KAPPA, C_SW, 1, *SOLVE), "np = 33, derivative")
    refused(lambda: lat.cloverrat_acc(a, [], [], *SOLVE), "np = 0, acc")
    refused(lambda: lat.cloverrat_heatbath(a, [0.1] * 33, [0.5] * 33, *SOLVE), "np = 33, heatbath")
    f32, full = lat.field32(), lat.full_field()
    refused(lambda: force(1, f32), "fp32 field")
    refused(lambda: force(1, full), "full field")
    refused(lambda: lat.cloverrat_acc(f32, MU3, RMU3, *SOLVE), "fp32 field, acc")
    refused(lambda: lat.cloverrat_heatbath(full, NU3, RNU3, *SOLVE), "full field, heatbath")
    lat.set_loopback(1)
    try:
        tw[0] = twist_probe(lat, a)                                     # (the rehearsal's stencil takes another path: its own bits)
        all_four("loopback")
    finally:
        lat.set_loopback(0)
    tw[0] = twist_probe(lat, a)
    lat.sw_invert(0, 0.3)                                               # an inverse made with mu != 0
    all_four("inverse with mu != 0")
    lat.sw_invert(1, 0.0)                                               # ... or for the odd sites
    all_four("inverse for OO")
    lat.sw_invert(0, 0.0)
    swh, swih = lat.get_clover()
    lat.set_clover(swh, swih)                                           # the same blocks uploaded: nobody knows which inverse this is
    all_four("set_clover")
    lat.sw_term(g, KAPPA, C_SW)                                         # a new clover term: sw_inv is no longer valid
    all_four("sw_inv not valid")
    lat.sw_invert(0, 0.0)
    lat.momenta_upload(np.zeros((lat.V, 4, 8)))
    lat.update_gauge(0.0)                                               # the links "moved": clover term and inverse are stale
    tw[0] = twist_probe(lat, a)                                         # (reunitarised links: the probe's value may move in the last bit)
    all_four("stale inverse after update_gauge")
    lat.sw_term(None, KAPPA, C_SW)
    lat.sw_invert(0, 0.0)
    force(1)                                                            # and a legal call goes through
    assert not np.array_equal(lat.derivative(), before)
    lat.close()
    # a T-split context
    split = Lattice(2, 4, 4, 4, nproc_t=2, proc_t=0, kappa=KAPPA)
    gs = syn.gauge_field(6, 2, 4, 4, 4, 2, 0)
    split.set_gauge(gs)                                                 # refused for the split alone, whatever the clover state
    split.derivative_zero()
    fa = split.field()
    with pytest.raises(TmHipError):
        split.cloverrat_force([fa], [0.5], KAPPA, C_SW, 1)
    with pytest.raises(TmHipError):
        split.cloverrat_acc(fa, MU3, RMU3, *SOLVE)
    assert not split.derivative().any()
    split.close()


# ---------------------------------------------------------------- the force is the derivative of the action
class CloverRatTrajectory:
    """H = p^2 / 2 + pf . (pf + sum_j rmu_j chi_j): cloverrat_acc with pf fixed; force = cloverrat_derivative with trlog 0; sw_term +
    sw_invert(EE, 0.) from the moving links.  Lattice and step sizes of the NDCLOVERRAT trajectory of tests/test_gpu_ndcloverrat.py."""
    MU, RMU = [0.4, 0.9, 2.0], [0.3, 0.8, 1.5]
    SOLVE = (2000, 1e-26, 1)

    def __init__(self, shape=(4, 4, 6, 4), kappa=0.125, c_sw=1.2, seed=5):
        from tmlqcd_amd import Lattice
        self.kappa, self.c_sw = kappa, c_sw
        self.lat = lat = Lattice(*shape, kappa=kappa, mu=CTX_MU)
        self.g0 = syn.gauge_field(seed, *shape)
        self.p0 = np.random.default_rng(seed + 1).standard_normal((lat.V, 4, 8))
        self.reset()
        self.pf = lat.field(syn.spinor_field_eo(seed + 2, 1, *shape))
        self.iters = 0

    def reset(self):
        self.lat.set_gauge(self.g0)
        self.lat.momenta_upload(self.p0)

    def clover(self):
        self.lat.sw_term(None, self.kappa, self.c_sw)                   # from the links resident in HBM
        self.lat.sw_invert(0, 0.0)
        assert self.lat.sw_invert_failures() == 0

    def energy(self):
        self.clover()
        s, it = self.lat.cloverrat_acc(self.pf, self.MU, self.RMU, *self.SOLVE)
        assert it > 0
        p = self.lat.momenta_download()
        return 0.5 * float((p * p).sum()) + s

    def force(self, step):
        lat = self.lat
        lat.derivative_zero()
        self.clover()
        it = lat.cloverrat_derivative(self.pf, self.MU, self.RMU, self.kappa, self.c_sw, 0, *self.SOLVE)
        assert it > 0
        self.iters += it
        lat.update_momenta(step)

    def leapfrog(self, nsteps, eps):
        self.force(0.5 * eps)
        for k in range(nsteps):
            self.lat.update_gauge(eps)
            self.force(eps if k < nsteps - 1 else 0.5 * eps)


def test_trajectory_conserves_its_hamiltonian_to_second_order_and_is_reversible():
    tr = CloverRatTrajectory()
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
    print("cloverrat: H0 = %.6f   dH(eps = 0.05) = %.3e   dH(eps = 0.025) = %.3e   ratio %.2f   CG iterations %d"
          % (h0, dh[4], dh[8], dh[4] / dh[8], tr.iters))
    assert abs(dh[8]) < abs(dh[4])
    assert 3.0 < dh[4] / dh[8] < 5.5                                    # O(eps^2), the factor tests/test_gpu_ndcloverrat.py demands
    assert np.abs(back - tr.g0).max() < 1e-10


# ---------------------------------------------------------------- drop-in
@pytest.mark.parametrize("mode", ["coherent", "resident"])
def test_dropin_symbols(mode):
    errs = run_child("cloverrat_dropin_child.py", mode)
    print(errs)
    assert {"cloverrat_derivative", "cloverrat_derivative_iters", "cloverrat_acc", "cloverrat_heatbath", "cloverrat_heatbath_energy"} <= set(errs)
    for k, v in errs.items():
        if k.endswith("_iters"):
            assert v == 0, (k, v)
        elif k == "cloverrat_derivative_held_back" or k.endswith("_failures"):
            assert v == 0.0, (k, v)
        else:
            assert v < TOL, (k, v)
