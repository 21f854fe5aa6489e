"""GPU: the polynomial monomial NDPOLY on the device (poly.hip): the four-term combination, Ptilde_ndpsi, and the three bodies of
monomial/ndpoly_monomial.c -- against the reference's 4^4 fixture (tools/make_golden_poly.py), against the NumPy restatement over the
CPU oracle (tests/poly_restate.py) on ragged lattices, as the force of a molecular-dynamics trajectory, and through the drop-in.

Bounds against the fixture: 8 x the deviation the restatement itself has from the reference (tests/poly_restate.py::gpu_bound, never
below TOL) -- the chain of 48 factors and the Clenshaw sums amplify rounding, the GPU contracts to FMA and sums in another order."""
import json
import os

import numpy as np
import pytest

from oracle.nd_restate import cplx, hop_over, real
from tests import ndsw_restate as sw
from tests import poly_restate
from tests.hostprog import run_child
from tests.poly_restate import gpu_bound, roots_of
from tests.util import TOL, random_gauge, random_spinor, rel_err
from tmlqcd_amd import synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
THETA = (1.0, 0.5, -0.25, 0.125)
MUBAR, EPSBAR, INVMAXEV, CPOL = 0.11, 0.09, 0.71, 1.15
EVMIN, EVMAX = 0.02, 1.0


def pair(dims, kappa=0.131, seed=93):
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    orc = Oracle(*dims, kappa=kappa, mu=0.0, theta=THETA, threads=8)
    lat = Lattice(*dims, kappa=kappa, mu=0.0, theta=THETA)
    g = random_gauge(seed, orc.VPR)
    orc.set_gauge(g); lat.set_gauge(g)
    lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
    return orc, lat


def synthetic_roots(n, radius=0.8):
    """2n - 2 roots on a circle, arranged as the reference's root files are: the first n - 1 in the upper half plane (B), the second n - 1
    their conjugates in reversed order, z[2n-3-k] = conj(z[k]) (B^dagger) -- the pairing ndpoly_derivative's n - 1 terms rely on"""
    th = np.pi * (np.arange(n - 1) + 0.5) / (n - 1)
    z = radius * np.exp(1j * th)
    return list(z) + list(np.conj(z[::-1]))


@pytest.fixture(scope="module")
def fx():
    f = np.load(os.path.join(GOLD, "ref_poly_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_poly_scalars_4x4.json")))
    gauge = np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"])
    return f, s, gauge


def fixture_lattice(s, gauge):
    from tmlqcd_amd import Lattice
    lat = Lattice(s["T"], s["L"], s["L"], s["L"], kappa=s["kappa"], mu=0.0)
    lat.set_gauge(gauge)
    lat.set_nd(s["mubar"], s["epsbar"], s["invmaxev"])
    return lat


# ---------------------------------------------------------------- 1: the kernel
@pytest.mark.parametrize("dims", [(2, 2, 2, 2), (4, 2, 6, 2), (6, 6, 6, 6)])
def test_four_term_combination_against_numpy(dims):
    """Vh = 8 (less than a wave), 48 (not a multiple of 64), 648 (a partial last wave); mixed signs, one coefficient exactly 0; the output
    aliasing each input in turn; inputs that are not the output stay bit-identical"""
    from tmlqcd_amd import Lattice
    lat = Lattice(*dims)
    N = lat.Vh
    h = [random_spinor(700 + k, N) for k in range(8)]
    for cs in ((0.7, -1.3, 0.0, 2.1), (-0.4, 0.0, 1.9, -0.6), (0.0, 1.1, -2.2, 0.3)):
        # the reference's form on one field: R aliases S, U, V in turn (alias -1: four different fields)
        for alias in (-1, 1, 2, 3):
            f = [lat.field(x) for x in h[:4]]
            idx = [0, 1, 2, 3]
            if alias > 0:
                idx[alias] = 0
            lat.assign_mul_add_mul_add_mul_add_mul_r(f[0], f[idx[1]], f[idx[2]], f[idx[3]], *cs)
            want = poly_restate.comb4(h[0], h[idx[1]], h[idx[2]], h[idx[3]], *cs)
            assert rel_err(f[0].download(), want) < TOL, (cs, alias)
            for k in range(1, 4):
                assert np.array_equal(f[k].download(), h[k]), (cs, alias, k)
        # the doublet form: its output is a pair of its own, or one of the four input pairs
        for alias in (-1, 0, 1, 2, 3):
            f = [lat.field(x) for x in h]
            ins = [(f[2 * k], f[2 * k + 1]) for k in range(4)]
            out = (lat.field(), lat.field()) if alias < 0 else ins[alias]
            lat.comb4_ndpsi(out, *ins, *cs)
            for fl in range(2):
                want = poly_restate.comb4(h[fl], h[2 + fl], h[4 + fl], h[6 + fl], *cs)
                assert rel_err(out[fl].download(), want) < TOL, (cs, alias, fl)
            for k in range(4):
                if k != alias:
                    assert np.array_equal(ins[k][0].download(), h[2 * k]) and np.array_equal(ins[k][1].download(), h[2 * k + 1]), (cs, alias, k)
    lat.close()


# ---------------------------------------------------------------- 2: Ptilde_ndpsi
def test_Ptilde_against_the_fixture(fx):
    f, s, gauge = fx
    lat = fixture_lattice(s, gauge)
    Su, Sd = lat.field(np.ascontiguousarray(f["S_up"])), lat.field(np.ascontiguousarray(f["S_dn"]))
    Ru, Rd = lat.field(), lat.field()
    lat.Ptilde_ndpsi(Ru, Rd, s["PtildeCoefs"], Su, Sd, s["evmin"], s["evmax"])
    err = max(rel_err(Ru.download(), f["ptilde_up"]), rel_err(Rd.download(), f["ptilde_dn"]))
    print("Ptilde_ndpsi, degree %d, against the reference: %.3e (bound %.3e)" % (s["PtildeDegree"], err, gpu_bound(s, "ptilde")))
    assert np.array_equal(Su.download(), f["S_up"]) and np.array_equal(Sd.download(), f["S_dn"])
    assert err < gpu_bound(s, "ptilde")
    lat.Ptilde_ndpsi(Su, Sd, s["PtildeCoefs"], Su, Sd, s["evmin"], s["evmax"])            # R = S
    assert np.array_equal(Su.download(), Ru.download()) and np.array_equal(Sd.download(), Rd.download())
    lat.close()


@pytest.mark.parametrize("op", ["Qtm_pm_ndpsi", "Qsw_pm_ndpsi"])
@pytest.mark.parametrize("dims", [(4, 2, 6, 2), (8, 6, 4, 12)])
def test_Ptilde_against_the_restatement(dims, op):
    """coefficient vectors of length 1, 2, 3 (the loop that runs zero times, the last-step form alone) and 9; both operators; R = S"""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    mb, eb, c = sw.FIXTURE
    orc = Oracle(*dims, kappa=sw.KAPPA, mu=0.0, theta=sw.THETA, threads=8)
    lat = Lattice(*dims, kappa=sw.KAPPA, mu=0.0, theta=sw.THETA)
    g = random_gauge(sw.shape_seed(dims), orc.VPR)
    orc.set_gauge(g); lat.set_gauge(g)
    lat.set_nd(mb, eb, c)
    N = lat.Vh
    H = hop_over(orc.Hopping_Matrix, N)
    if op == "Qsw_pm_ndpsi":
        lat.sw_term(g, sw.KAPPA, sw.C_SW)
        lat.sw_invert_nd(mb * mb - eb * eb)
        cl = sw.clover_of(orc, sw.KAPPA, sw.C_SW)
        cl.sw_invert_nd(mb * mb - eb * eb)
        Qsq = lambda xs, xc: sw.Qsw_pm_ndpsi(cl, H, xs, xc, mb, eb, c)
    else:
        Qsq = lambda xs, xc: poly_restate.Qtm_pm_ndpsi(H, xs, xc, mb, eb, c)
    hs, hc = random_spinor(51, N), random_spinor(52, N)
    rng = np.random.default_rng(8)
    for n in (1, 2, 3, 9):
        coefs = list(rng.standard_normal(n))
        ws, wc = poly_restate.Ptilde_ndpsi(Qsq, coefs, cplx(hs), cplx(hc), EVMIN, EVMAX)
        Ss, Sc, Rs, Rc = lat.field(hs), lat.field(hc), lat.field(), lat.field()
        lat.Ptilde_ndpsi(Rs, Rc, coefs, Ss, Sc, EVMIN, EVMAX, op)
        err = max(rel_err(Rs.download(), real(ws)), rel_err(Rc.download(), real(wc)))
        print("Ptilde_ndpsi %s %s n = %d: %.3e" % (dims, op, n, err))
        assert err < TOL, n
        assert np.array_equal(Ss.download(), hs) and np.array_equal(Sc.download(), hc)
        lat.Ptilde_ndpsi(Ss, Sc, coefs, Ss, Sc, EVMIN, EVMAX, op)
        assert np.array_equal(Ss.download(), Rs.download()) and np.array_equal(Sc.download(), Rc.download()), n
    lat.close()


# ---------------------------------------------------------------- 3: the force
def _nonzero_derivative(lat, seed):
    N = lat.Vh
    a, b = lat.field(random_spinor(seed, N)), lat.field(random_spinor(seed + 1, N))
    lat.derivative_zero()
    lat.deriv_Sb(0, a, b, 0.37)
    return lat.derivative()


def test_force_against_the_fixture(fx):
    f, s, gauge = fx
    lat = fixture_lattice(s, gauge)
    pu, pd = lat.field(np.ascontiguousarray(f["phi_up"])), lat.field(np.ascontiguousarray(f["phi_dn"]))
    got = {}
    for batch in (1, 12, 32):
        lat.set_option("poly_batch", batch)
        d0 = _nonzero_derivative(lat, 60)
        lat.ndpoly_derivative(pu, pd, roots_of(s), s["Cpol"], s["invmaxev"])
        got[batch] = lat.derivative() - d0
        err = float(np.abs(got[batch] - f["force"]).max() / np.abs(f["force"]).max())
        print("ndpoly_derivative n = %d poly_batch %d against the reference: %.3e (bound %.3e)" % (s["MDPolyDegree"], batch, err, gpu_bound(s, "force")))
        assert err < gpu_bound(s, "force"), batch
    assert np.array_equal(pu.download(), f["phi_up"]) and np.array_equal(pd.download(), f["phi_dn"])
    lat.close()


@pytest.mark.parametrize("n", [3, 4, 6])
@pytest.mark.parametrize("dims", [(4, 2, 6, 2), (6, 6, 6, 6), (8, 6, 4, 12)])
def test_force_against_the_restatement(dims, n):
    """poly_batch 1 (the single-pair kernel in the reference's order), 2 (does not divide n - 1 = 3, 5) and 32 (larger than the loop), on top
    of a non-zero accumulator; batched against poly_batch 1 within TOL"""
    orc, lat = pair(dims)
    N = lat.Vh
    hu, hd = random_spinor(410 + n, N), random_spinor(510 + n, N)
    pu, pd = lat.field(hu), lat.field(hd)
    roots = synthetic_roots(n)
    po = poly_restate.Poly(orc, MUBAR, EPSBAR, INVMAXEV)
    want = po.derivative(cplx(hu), cplx(hd), roots, CPOL, np.zeros((orc.VPR, 4, 8)))[:orc.V]
    got = {}
    for batch in (1, 2, 32):
        lat.set_option("poly_batch", batch)
        d0 = _nonzero_derivative(lat, 70)
        lat.ndpoly_derivative(pu, pd, roots, CPOL, INVMAXEV)
        got[batch] = lat.derivative() - d0
        err = float(np.abs(got[batch] - want).max() / np.abs(want).max())
        print("ndpoly_derivative %s n = %d poly_batch %d: %.3e" % (dims, n, batch, err))
        assert err < TOL, batch
    scale = np.abs(got[1]).max()
    assert np.abs(got[2] - got[1]).max() < TOL * scale and np.abs(got[32] - got[1]).max() < TOL * scale
    assert np.array_equal(pu.download(), hu) and np.array_equal(pd.download(), hd)
    lat.close()


# ---------------------------------------------------------------- 4: heatbath and acceptance
def test_heatbath_and_acceptance_against_the_fixture(fx):
    f, s, gauge = fx
    lat = fixture_lattice(s, gauge)
    roots = roots_of(s)
    pu, pd = lat.field(np.ascontiguousarray(f["eta_up"])), lat.field(np.ascontiguousarray(f["eta_dn"]))
    e0 = lat.ndpoly_heatbath(pu, pd, roots, s["Cpol"], s["invmaxev"], s["PtildeCoefs"], s["evmin"], s["evmax"])
    err = max(rel_err(pu.download(), f["pf_up"]), rel_err(pd.download(), f["pf_dn"]))
    print("ndpoly_heatbath: pf %.3e (bound %.3e), energy0 %.3e (bound %.3e)" % (err, gpu_bound(s, "pf"), abs(e0 - s["energy0"]) / s["energy0"], gpu_bound(s, "energy0")))
    assert err < gpu_bound(s, "pf")
    assert abs(e0 - s["energy0"]) < gpu_bound(s, "energy0") * s["energy0"]
    # the acceptance step on the reference's pf
    pu, pd = lat.field(np.ascontiguousarray(f["pf_up"])), lat.field(np.ascontiguousarray(f["pf_dn"]))
    e1, steps, ener = lat.ndpoly_acc(pu, pd, roots, s["Cpol"], s["invmaxev"], s["MDPolyCoefs"], s["PtildeCoefs"], s["evmin"], s["evmax"], s["PrecisionHfinal"])
    d = [abs(a - b) / abs(b) for a, b in zip(ener, s["Ener"])]
    print("ndpoly_acc: corrections %d, Ener[j] %s (bounds %s)" % (steps, d, [gpu_bound(s, "Ener", j) for j in range(8)]))
    assert steps == s["corrections"]
    assert e1 == ener[steps]
    for j in range(steps + 1):
        assert d[j] < gpu_bound(s, "Ener", j), j
    assert abs(e1 - s["energy1"]) < gpu_bound(s, "Ener", steps) * abs(s["energy1"])
    assert np.array_equal(pu.download(), f["pf_up"]) and np.array_equal(pd.download(), f["pf_dn"])
    lat.close()


def test_heatbath_and_acceptance_against_the_restatement_on_a_ragged_lattice():
    """n = 6 with synthetic roots and short Chebyshev sums; precision_hfinal chosen once to stop after one correction, once to run all seven"""
    dims = (4, 2, 6, 2)
    orc, lat = pair(dims)
    N = lat.Vh
    n = 6
    roots = synthetic_roots(n)
    rng = np.random.default_rng(12)
    md, pt = [1.9] + list(0.05 * rng.standard_normal(n - 1)), [2.1] + list(0.04 * rng.standard_normal(8))
    po = poly_restate.Poly(orc, MUBAR, EPSBAR, INVMAXEV)
    hu, hd = random_spinor(81, N), random_spinor(82, N)
    w0, wu, wd = po.heatbath(cplx(hu), cplx(hd), roots, CPOL, pt, EVMIN, EVMAX)
    pu, pd = lat.field(hu), lat.field(hd)
    e0 = lat.ndpoly_heatbath(pu, pd, roots, CPOL, INVMAXEV, pt, EVMIN, EVMAX)
    assert abs(e0 - w0) < TOL * w0
    assert rel_err(pu.download(), real(wu)) < TOL and rel_err(pd.download(), real(wd)) < TOL
    pu, pd = lat.field(hu), lat.field(hd)
    for prec, steps_want in ((np.inf, 1), (0.0, 7)):
        w1, wsteps, wen = po.acc(cplx(hu), cplx(hd), roots, CPOL, md, pt, EVMIN, EVMAX, prec)
        e1, steps, ener = lat.ndpoly_acc(pu, pd, roots, CPOL, INVMAXEV, md, pt, EVMIN, EVMAX, prec)
        assert steps == wsteps == steps_want
        # Ener[0] and Ener[1] to the plain relative TOL.  From j = 2 on Ener[j] is an alternating binomial sum of the earlier energies and a
        # squared norm: the rounding of a term enters with its binomial weight, at most C(j, j / 2), on the scale of the largest term
        weight = [1, 1, 2, 3, 6, 10, 20, 35]
        bound = [TOL * abs(wen[j]) if j < 2 else TOL * weight[j] * max(abs(x) for x in wen[:j + 1]) for j in range(8)]
        print("ndpoly_acc %s precision %g: %d corrections, |Ener - restatement| / bound %s" % (dims, prec, steps, [abs(a - b) / bd if bd else 0.0 for a, b, bd in zip(ener, wen, bound)]))
        assert all(abs(a - b) < bd for a, b, bd in zip(ener[:steps + 1], wen, bound))
        assert e1 == ener[steps] and ener[steps + 1:] == [0.0] * (7 - steps)
    assert np.array_equal(pu.download(), hu) and np.array_equal(pd.download(), hd)
    lat.close()


# ---------------------------------------------------------------- 5: the force is the derivative of the energy
class PolyTrajectory:
    """H = p^2 / 2 - beta S_plaq + |B phi|^2 (Ener[0] of ndpoly_acc) with phi fixed, n = 4 on 4^4, leapfrog with update_momenta /
    update_gauge: everything resident, as tests/test_gpu_md_trajectory.py and the gauge + determinant trajectory of tests/test_gpu_gauge.py"""
    BETA, N_POLY = 5.6, 4

    def __init__(self, L=4, kappa=0.125, seed=5):
        from tmlqcd_amd import Lattice
        self.lat = lat = Lattice(L, L, L, L, kappa=kappa, mu=0.0)
        lat.set_nd(0.12, 0.1, 0.6)
        self.roots = synthetic_roots(self.N_POLY)
        self.g0 = syn.gauge_field(seed, L, L, L, L)
        self.p0 = np.random.default_rng(seed + 1).standard_normal((lat.V, 4, 8))
        self.reset()
        self.pf = [lat.field(syn.spinor_field_eo(seed + 2 + q, 1, L, L, L, L)) for q in range(2)]

    def reset(self):
        self.lat.set_gauge(self.g0)
        self.lat.momenta_upload(self.p0)

    def energy(self):
        lat = self.lat
        _, _, ener = lat.ndpoly_acc(self.pf[0], self.pf[1], self.roots, 1.1, 0.6, [2.0, 0.1, 0.05, 0.02], [2.0], 0.05, 1.0, np.inf)
        p = lat.momenta_download()
        return 0.5 * float((p * p).sum()) - self.BETA * lat.measure_gauge_action(0.0) + ener[0]   # gauge_acc: E = beta S_plaq enters with a minus

    def force(self, step):
        lat = self.lat
        lat.derivative_zero()
        lat.gauge_derivative(self.BETA)
        lat.ndpoly_derivative(self.pf[0], self.pf[1], self.roots, 1.1, 0.6)
        lat.update_momenta(step)

    def leapfrog(self, nsteps, eps):
        self.force(0.5 * eps)
        for k in range(nsteps):
            self.lat.update_gauge(eps)
            self.force(eps if k < nsteps - 1 else 0.5 * eps)


def test_leapfrog_with_the_polynomial_force_conserves_its_hamiltonian_to_second_order_and_is_reversible():
    tr = PolyTrajectory()
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
    pend = tr.lat.momenta_download()
    tr.lat.close()
    print("ndpoly: H0 = %.6f   dH(eps = 0.05) = %.3e   dH(eps = 0.025) = %.3e   ratio %.2f" % (h0, dh[4], dh[8], dh[4] / dh[8]))
    assert abs(dh[8]) < abs(dh[4])
    assert 3.0 <= dh[4] / dh[8] <= 5.0                                  # O(eps^2): a wrong forcefactor, a sign error or a dropped flavour leaves O(eps)
    assert np.abs(back - tr.g0).max() < 1e-10
    assert np.abs(pend + tr.p0).max() < 1e-9


# ---------------------------------------------------------------- 6: refusals
def test_refusals_leave_the_accumulator_alone():
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    orc, lat = pair((4, 4, 4, 4))
    N = lat.Vh
    a, b = lat.field(random_spinor(1, N)), lat.field(random_spinor(2, N))
    before = _nonzero_derivative(lat, 3)
    roots = synthetic_roots(4)
    other = Lattice(4, 4, 4, 6)                                         # another stride
    cases = {
        "n = 2": (a, b, synthetic_roots(2)),
        "fp32": (a, lat.field32(), roots),
        "full field": (lat.full_field(), b, roots),
        "stride": (a, other.field(), roots),
        "one field twice": (a, a, roots),
    }
    for what, (fu, fd, r) in cases.items():
        with pytest.raises(TmHipError):
            lat.ndpoly_derivative(fu, fd, r, CPOL, INVMAXEV)
        assert np.array_equal(lat.derivative(), before), what
    lat.set_loopback(1)
    with pytest.raises(TmHipError):
        lat.ndpoly_derivative(a, b, roots, CPOL, INVMAXEV)
    lat.set_loopback(0)
    assert np.array_equal(lat.derivative(), before)
    with pytest.raises(TmHipError):                                     # an invmaxev that is not the one of set_nd
        lat.ndpoly_derivative(a, b, roots, CPOL, 0.5 * INVMAXEV)
    assert np.array_equal(lat.derivative(), before)
    # a failed allocation: the first, one in the middle of the chain, the last of the chain, the first and the last of the group's work
    # fields (n = 6, poly_batch 2: 8 chain fields, 6 chi_hi, 8 H_eo results); the force keeps nothing, so every attempt allocates all 22 again
    roots6 = synthetic_roots(6)
    lat.set_option("poly_batch", 2)
    for k in (1, 5, 8, 9, 22):
        lat.set_option("poly_fail_alloc", k)
        with pytest.raises(TmHipError):
            lat.ndpoly_derivative(a, b, roots6, CPOL, INVMAXEV)
        assert np.array_equal(lat.derivative(), before), k
    lat.set_option("poly_fail_alloc", 23)                               # one more allocation than the call makes: it goes through ...
    lat.ndpoly_derivative(a, b, roots6, CPOL, INVMAXEV)
    got = lat.derivative() - before
    lat.set_option("poly_fail_alloc", 0)
    lat.derivative_zero()
    lat.ndpoly_derivative(a, b, roots6, CPOL, INVMAXEV)                 # ... and equals a call that was never disturbed
    clean = lat.derivative()
    assert np.abs(got - clean).max() < TOL * np.abs(clean).max() and np.abs(clean).max() > 0
    before = _nonzero_derivative(lat, 3)
    # Ptilde_ndpsi: no coefficient, the clover operator without a valid sw_inv_nd, R on the other flavour of S
    r0, r1 = lat.field(), lat.field()
    with pytest.raises(TmHipError):
        lat.Ptilde_ndpsi(r0, r1, [], a, b, EVMIN, EVMAX)
    with pytest.raises(TmHipError):
        lat.Ptilde_ndpsi(r0, r1, [1.0, 0.5], a, b, EVMIN, EVMAX, "Qsw_pm_ndpsi")
    with pytest.raises(TmHipError):
        lat.Ptilde_ndpsi(b, a, [1.0, 0.5], a, b, EVMIN, EVMAX)
    with pytest.raises(TmHipError):
        lat.Ptilde_ndpsi(r0, a, [1.0, 0.5], a, b, EVMIN, EVMAX)
    assert not r0.download().any() and not r1.download().any()
    # the doublet combination: an output on an input of the other flavour
    with pytest.raises(TmHipError):
        lat.comb4_ndpsi((r0, r1), (a, b), (a, b), (a, r0), (a, b), 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(TmHipError):
        lat.comb4_ndpsi((b, r1), (a, b), (a, b), (a, b), (a, b), 1.0, 1.0, 1.0, 1.0)
    assert np.array_equal(a.download(), random_spinor(1, N)) and np.array_equal(b.download(), random_spinor(2, N))
    # no gauge field yet
    other.derivative_zero()
    with pytest.raises(TmHipError):
        other.ndpoly_derivative(other.field(), other.field(), roots, CPOL, INVMAXEV)
    assert not other.derivative().any()
    other.close()
    # a T-split context
    split = Lattice(2, 4, 4, 4, nproc_t=2, proc_t=0)
    split.set_gauge(syn.gauge_field(6, 2, 4, 4, 4, 2, 0))
    split.derivative_zero()
    with pytest.raises(TmHipError):
        split.ndpoly_derivative(split.field(), split.field(), roots, CPOL, INVMAXEV)
    assert not split.derivative().any()
    split.close()
    lat.close()


# ---------------------------------------------------------------- 7: drop-in
def test_drop_in_symbols_equal_the_core_results():
    out = run_child("poly_dropin_child.py", "coherent")
    print(out)
    for k, v in out["errs"].items():
        assert v == 0.0, k
    assert out["corrections"] == out["corrections_core"]


def test_drop_in_ends_with_a_message_when_phmc_exact_poly_is_set():
    r = run_child("poly_dropin_child.py", "exact_poly", check=False)
    assert r.returncode not in (0, -6, -11, 134, 139), (r.returncode, r.stderr[-2000:])
    assert "phmc_exact_poly == 1" in r.stderr
    assert "returned" not in r.stdout
