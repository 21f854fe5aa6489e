"""GPU: the rational monomials on the device (rational.hip): the batched hopping force deriv_Sb_batch, Q_tau1_sub_const_ndpsi and
assign_add_mul, and the bodies of rat (monomial/rat_monomial.c, type RAT) and ndrat (monomial/ndrat_monomial.c, type NDRAT) --
against the reference's 4^4 fixture (tools/make_golden_rat.py), against the NumPy restatement over the CPU oracle
(tests/rat_restate.py) on ragged lattices, and as the force of a molecular-dynamics trajectory."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest

from oracle.nd_restate import cplx, hop_over, real
from tests import rat_restate
from tests.util import TOL, random_gauge, random_spinor, rel_err

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EO, OE = 0, 1
THETA = (1.0, 0.5, -0.25, 0.125)
MUBAR, EPSBAR, INVMAXEV = 0.11, 0.09, 0.71


def pair(dims, kappa=0.131, mu=0.0, theta=THETA, seed=91):
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    orc = Oracle(*dims, kappa=kappa, mu=mu, theta=theta, threads=8)
    lat = Lattice(*dims, kappa=kappa, mu=mu, theta=theta)
    g = random_gauge(seed, orc.VPR)
    orc.set_gauge(g); lat.set_gauge(g)
    return orc, lat


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_rat_4x4.npz")), json.load(open(os.path.join(GOLD, "ref_rat_scalars_4x4.json")))


# ---------------------------------------------------------------- 1, 2: the batched kernel
@pytest.mark.parametrize("n", [1, 2, 5, 64])
@pytest.mark.parametrize("dims", [(2, 2, 2, 2), (4, 2, 6, 2), (6, 6, 6, 6), (8, 6, 4, 12)])
def test_deriv_Sb_batch_against_oracle_and_against_single_calls(dims, n):
    """n pairs in one launch == n calls of the oracle's deriv_Sb == n calls of the single-pair kernel, on top of a non-zero
    accumulator, both parities, twisted phases in every direction; fields shared between pairs and sides; inputs untouched."""
    orc, lat = pair(dims)
    N = orc.Vh
    m = min(n, 5) + 1
    host = [random_spinor(300 + q, N) for q in range(m)]
    dev = [lat.field(h) for h in host]
    obuf = []
    for h in host:
        b = orc.new_field(); b[:N] = h; obuf.append(b)
    li = [j % m for j in range(n)]                    # pool[q] is l of pair q and k of pair q-1; n > m: shared by several pairs
    ki = [(j + 1) % m for j in range(n)]
    fac = np.array([(-1.0) ** j * (0.3 + 0.11 * (j % 7)) for j in range(n)])   # mixed signs from n = 3 on
    if n > 1:
        fac[1] = 0.0                                                           # and one factor exactly 0
    df = np.zeros((orc.VPR, 4, 8))
    lat.derivative_zero()
    orc.deriv_Sb(EO, obuf[0], obuf[1], df, 0.37); lat.deriv_Sb(EO, dev[0], dev[1], 0.37)       # something is there already
    for ieo in (EO, OE):
        for j in range(n):
            orc.deriv_Sb(ieo, obuf[li[j]], obuf[ki[j]], df, float(fac[j]))
        lat.deriv_Sb_batch(ieo, [dev[q] for q in li], [dev[q] for q in ki], fac)
    got = lat.derivative()
    e1 = rel_err(got, df[:orc.V])
    lat.derivative_zero()
    lat.deriv_Sb(EO, dev[0], dev[1], 0.37)
    for ieo in (EO, OE):
        for j in range(n):
            lat.deriv_Sb(ieo, dev[li[j]], dev[ki[j]], float(fac[j]))
    e2 = rel_err(got, lat.derivative())
    print("deriv_Sb_batch %s n = %d: against the oracle %.2e, against n single launches %.2e" % (dims, n, e1, e2))
    assert e1 < TOL
    assert e2 < TOL
    for h, d in zip(host, dev):
        assert np.array_equal(d.download(), h)
    lat.close()


# ---------------------------------------------------------------- 3: refusals
def test_deriv_Sb_batch_refusals_leave_the_accumulator_alone():
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    from tmlqcd_amd.hip import TmHipError
    orc, lat = pair((4, 4, 4, 4))
    N = lat.Vh
    a, b = lat.field(random_spinor(1, N)), lat.field(random_spinor(2, N))
    lat.derivative_zero()
    lat.deriv_Sb(OE, a, b, 0.8)
    before = lat.derivative()
    other = Lattice(4, 4, 4, 6)                                         # another stride
    cases = {
        "n = 0": ([], [], []),
        "n = 65": ([a] * 65, [b] * 65, [1.0] * 65),
        "null l": ([a, types.SimpleNamespace(h=None)], [b, b], [1.0, 1.0]),
        "null k": ([a], [types.SimpleNamespace(h=None)], [1.0]),
        "fp32": ([a], [lat.field32()], [1.0]),
        "full field": ([lat.full_field()], [b], [1.0]),
        "stride": ([a, a], [b, other.field()], [1.0, 1.0]),
    }
    for what, (ls, ks, fs) in cases.items():
        with pytest.raises(TmHipError):
            lat.deriv_Sb_batch(EO, ls, ks, fs)
        assert np.array_equal(lat.derivative(), before), what
    lat.set_loopback(1)
    with pytest.raises(TmHipError):
        lat.deriv_Sb_batch(EO, [a], [b], [1.0])
    lat.set_loopback(0)
    assert np.array_equal(lat.derivative(), before)
    lat.deriv_Sb_batch(EO, [a], [b], [0.0])                            # and a legal call with factor 0 adds nothing
    assert np.array_equal(lat.derivative(), before)
    # no gauge field yet
    other.derivative_zero()
    with pytest.raises(TmHipError):
        other.deriv_Sb_batch(EO, [other.field()], [other.field()], [1.0])
    assert not other.derivative().any()
    other.close()
    # a T-split context
    split = Lattice(2, 4, 4, 4, nproc_t=2, proc_t=0)
    split.set_gauge(syn.gauge_field(6, 2, 4, 4, 4, 2, 0))
    split.derivative_zero()
    with pytest.raises(TmHipError):
        split.deriv_Sb_batch(EO, [split.field()], [split.field()], [1.0])
    assert not split.derivative().any()
    split.close()
    lat.close()


# ---------------------------------------------------------------- 4: the two building blocks
def fixture_lattice(f, s, mu=0.0):
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    g = np.ascontiguousarray(f["gauge"])
    lat = Lattice(s["T"], s["L"], s["L"], s["L"], kappa=s["kappa"], mu=mu)
    lat.set_gauge(g)
    lat.set_nd(s["mubar"], s["epsbar"], s["invmaxev"])
    orc = Oracle(s["T"], s["L"], s["L"], s["L"], kappa=s["kappa"], mu=mu)
    orc.set_gauge(g)
    return orc, lat


def test_building_blocks_against_the_fixture(fx):
    f, s = fx
    orc, lat = fixture_lattice(f, s)
    N = lat.Vh
    ku, kd = lat.field(np.ascontiguousarray(f["chi_up_0"])), lat.field(np.ascontiguousarray(f["chi_dn_0"]))
    ls, lc = lat.field(), lat.field()
    lat.Q_tau1_sub_const_ndpsi(ls, lc, ku, kd, -1j * s["mu"][0], 1.0, s["invmaxev"])
    assert rel_err(ls.download(), f["Q_tau1_s"]) < TOL and rel_err(lc.download(), f["Q_tau1_c"]) < TOL
    # assign_add_mul: the reference's rat heatbath loop (rat_monomial.c:191-199) statement by statement on the device
    pf, t = lat.field(np.ascontiguousarray(f["eta_up"])), lat.field()
    for k in (2, 1, 0):
        chi = lat.field(np.ascontiguousarray(f["chi_up_%d" % k]))
        lat.op("Qtm_plus_psi", t, chi)
        lat.assign_add_mul(t, chi, -1j * s["nu"][k], N)
        lat.assign_add_mul(pf, t, 1j * s["rnu"][k], N)
    assert rel_err(pf.download(), f["rat_pf"]) < TOL
    lat.close()


def test_building_blocks_against_the_restatement_on_a_ragged_lattice():
    dims = (4, 2, 6, 2)
    orc, lat = pair(dims)
    lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
    N = lat.Vh
    ks, kc = random_spinor(11, N), random_spinor(12, N)
    z, Cpol, invev = 0.3 - 0.7j, 1.25, 0.83
    H = hop_over(orc.Hopping_Matrix, N)
    ws, wc = rat_restate.Q_tau1_sub_const_ndpsi(H, cplx(ks), cplx(kc), z, Cpol, invev, MUBAR, EPSBAR)
    dks, dkc, ls, lc = lat.field(ks), lat.field(kc), lat.field(), lat.field()
    lat.Q_tau1_sub_const_ndpsi(ls, lc, dks, dkc, z, Cpol, invev)
    assert rel_err(ls.download(), real(ws)) < TOL and rel_err(lc.download(), real(wc)) < TOL
    assert np.array_equal(dks.download(), ks) and np.array_equal(dkc.download(), kc)
    lat.set_option("nd_fused", 0)                                       # the two-stencil form has the same epilogue
    lat.Q_tau1_sub_const_ndpsi(ls, lc, dks, dkc, z, Cpol, invev)
    assert rel_err(ls.download(), real(ws)) < TOL and rel_err(lc.download(), real(wc)) < TOL
    lat.set_option("nd_fused", 1)
    c = -0.45 + 1.1j
    p = lat.field(ks)
    lat.assign_add_mul(p, dkc, c, N)
    assert rel_err(p.download(), real(cplx(ks) + c * cplx(kc))) < TOL
    lat.assign_add_mul(p, p, c, N)                                      # in place
    assert rel_err(p.download(), real((1 + c) * (cplx(ks) + c * cplx(kc)))) < TOL
    lat.assign_add_mul(p, dkc, c, 0)                                    # an empty loop in the reference
    lat.close()


# ---------------------------------------------------------------- 5: the forces from given solutions
def test_forces_against_the_fixture(fx):
    f, s = fx
    orc, lat = fixture_lattice(f, s, mu=0.2)                            # rat must not see the context's mu
    chi = [(lat.field(np.ascontiguousarray(f["chi_up_%d" % j])), lat.field(np.ascontiguousarray(f["chi_dn_%d" % j]))) for j in range(3)]
    for batch in (1, 2, 4):
        lat.set_option("rat_batch", batch)
        lat.derivative_zero()
        lat.ndrat_force(chi, s["mu"], s["rmu"], s["invmaxev"])
        assert rel_err(lat.derivative(), f["ndrat_derivative"]) < TOL, batch
        lat.derivative_zero()
        lat.rat_force([c[0] for c in chi], s["rmu"])
        assert rel_err(lat.derivative(), f["rat_derivative"]) < TOL, batch
    lat.close()


@pytest.mark.parametrize("np_", [1, 3, 7])
@pytest.mark.parametrize("dims", [(4, 2, 6, 2), (6, 4, 2, 8)])
def test_forces_against_the_restatement(dims, np_):
    orc, lat = pair(dims, mu=0.15)
    lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
    N = lat.Vh
    rng = np.random.default_rng(5 + np_)
    mu, rmu = list(rng.uniform(0.02, 2.0, np_)), list(rng.standard_normal(np_))
    hu, hd = [random_spinor(400 + j, N) for j in range(np_)], [random_spinor(500 + j, N) for j in range(np_)]
    chi = [(lat.field(a), lat.field(b)) for a, b in zip(hu, hd)]
    rat = rat_restate.Rat(orc, MUBAR, EPSBAR)
    want_nd = rat.ndrat_force([(cplx(a), cplx(b)) for a, b in zip(hu, hd)], mu, rmu, INVMAXEV, np.zeros((orc.VPR, 4, 8)))[:orc.V]
    want_rat = rat.rat_force([cplx(a) for a in hu], rmu, np.zeros((orc.VPR, 4, 8)))[:orc.V]
    for batch in (1, 2, 32):                                            # np = 3, 7 with 2: a ragged last group; 32: one group
        lat.set_option("rat_batch", batch)
        lat.derivative_zero()
        lat.ndrat_force(chi, mu, rmu, INVMAXEV)
        assert rel_err(lat.derivative(), want_nd) < TOL, batch
        lat.derivative_zero()
        lat.rat_force([c[0] for c in chi], rmu)
        assert rel_err(lat.derivative(), want_rat) < TOL, batch
    assert lat.mu == 0.15
    for (a, b), (fa, fb) in zip(zip(hu, hd), chi):
        assert np.array_equal(fa.download(), a) and np.array_equal(fb.download(), b)
    lat.close()


# ---------------------------------------------------------------- 6: the drivers
MU3, RMU3 = [0.21, 0.6, 1.7], [0.05, 0.4, 1.3]
NU3, RNU3 = [0.15, 0.5, 1.4], [0.04, 0.3, 0.9]
SOLVE = (2000, 1e-24, 1)


def test_ndrat_drivers():
    dims = (4, 4, 6, 4)
    orc, lat = pair(dims, kappa=0.125)
    lat.set_nd(MUBAR, EPSBAR, INVMAXEV)
    N = lat.Vh
    hu, hd = random_spinor(21, N), random_spinor(22, N)
    pu, pd = lat.field(hu), lat.field(hd)
    rat = rat_restate.Rat(orc, MUBAR, EPSBAR)
    # derivative
    it0, P = lat.cg_mms_tm_nd(pu, pd, MU3, *SOLVE)
    assert it0 > 0
    chi = [(cplx(a.download()), cplx(b.download())) for a, b in P]
    lat.derivative_zero()
    assert lat.ndrat_derivative(pu, pd, MU3, RMU3, INVMAXEV, *SOLVE) == it0
    got = lat.derivative()
    want = rat.ndrat_force(chi, MU3, RMU3, INVMAXEV, np.zeros((orc.VPR, 4, 8)))[:orc.V]
    assert rel_err(got, want) < TOL
    lat.derivative_zero()
    lat.ndrat_force(P, MU3, RMU3, INVMAXEV)
    assert np.array_equal(lat.derivative(), got)
    # acceptance
    e1, it = lat.ndrat_acc(pu, pd, MU3, RMU3, *SOLVE)
    assert it == it0
    w1 = rat.ndrat_acc(cplx(hu), cplx(hd), chi, RMU3)
    assert abs(e1 - w1) < TOL * abs(w1)
    # heatbath
    it0, P = lat.cg_mms_tm_nd(pu, pd, NU3, *SOLVE, P=P)
    chi = [(cplx(a.download()), cplx(b.download())) for a, b in P]
    e0, it = lat.ndrat_heatbath(pu, pd, NU3, RNU3, INVMAXEV, *SOLVE)
    assert it == it0
    w0, wu, wd = rat.ndrat_heatbath(cplx(hu), cplx(hd), chi, NU3, RNU3, INVMAXEV)
    assert abs(e0 - w0) < TOL * w0
    assert rel_err(pu.download(), real(wu)) < TOL and rel_err(pd.download(), real(wd)) < TOL
    lat.close()


def test_rat_drivers_run_at_mu_zero_and_restore_mu():
    from tmlqcd_amd import Lattice
    dims = (4, 4, 6, 4)
    g_mu = 0.3
    orc, lat = pair(dims, kappa=0.125, mu=g_mu)
    lat0 = Lattice(*dims, kappa=0.125, mu=0.0, theta=THETA)
    lat0.set_gauge(random_gauge(91, orc.VPR))
    N = lat.Vh
    h = random_spinor(31, N)
    pf, pf0 = lat.field(h), lat0.field(h)
    rat = rat_restate.Rat(orc)
    it0, _, P = lat0.cg_mms_tm(pf0, MU3, *SOLVE)
    assert it0 > 0
    chi = [cplx(a.download()) for a in P]
    lat.derivative_zero(); lat0.derivative_zero()
    assert lat.rat_derivative(pf, MU3, RMU3, *SOLVE) == it0
    assert lat0.rat_derivative(pf0, MU3, RMU3, *SOLVE) == it0
    got = lat.derivative()
    assert rel_err(got, lat0.derivative()) < TOL                         # the context's mu does not enter
    assert rel_err(got, rat.rat_force(chi, RMU3, np.zeros((orc.VPR, 4, 8)))[:orc.V]) < TOL
    lat0.derivative_zero()
    lat0.rat_force(P, RMU3)
    assert np.array_equal(lat0.derivative(), got)
    # mu is back: a following Qtm_pm_psi gives the mu != 0 answer
    assert lat.mu == g_mu
    out = lat.field()
    lat.Qtm_pm_psi(out, pf)
    want = np.zeros((N, 4, 3, 2))
    orc.op("Qtm_pm_psi", want, h)
    assert rel_err(out.download(), want) < TOL
    e1, it = lat.rat_acc(pf, MU3, RMU3, *SOLVE)
    assert it == it0
    w1 = rat.rat_acc(cplx(h), chi, RMU3)
    assert abs(e1 - w1) < TOL * abs(w1)
    it0, _, P = lat0.cg_mms_tm(pf0, NU3, *SOLVE, P=P)
    chi = [cplx(a.download()) for a in P]
    e0, it = lat.rat_heatbath(pf, NU3, RNU3, *SOLVE)
    assert it == it0
    w0, wpf = rat.rat_heatbath(cplx(h), chi, NU3, RNU3)
    assert abs(e0 - w0) < TOL * w0
    assert rel_err(pf.download(), real(wpf)) < TOL
    # an error path puts mu back too
    from tmlqcd_amd.hip import TmHipError
    with pytest.raises(TmHipError):
        lat.rat_derivative(pf, MU3, RMU3, 0, 1e-24, 1)                  # max_iter < 1 is refused by the solver
    lat.Qtm_pm_psi(out, lat.field(h))
    assert rel_err(out.download(), want) < TOL
    lat.close(); lat0.close()


# ---------------------------------------------------------------- 7: the force is the derivative of the action
class RatTrajectory:
    """H = p^2 / 2 + S, S = pf . (pf + sum_j rmu_j chi_j) with pf fixed (ndrat_acc / rat_acc), force from *_derivative, leapfrog with
    update_momenta / update_gauge: everything resident, as tests/test_gpu_md_trajectory.py."""
    MU, RMU = [0.4, 0.9, 2.0], [0.3, 0.8, 1.5]
    SOLVE = (2000, 1e-26, 1)

    def __init__(self, kind, L=8, kappa=0.125, seed=5):
        from tmlqcd_amd import Lattice
        from tmlqcd_amd import synthetic as syn
        self.kind = kind
        self.lat = lat = Lattice(L, L, L, L, kappa=kappa, mu=0.0)
        lat.set_nd(0.12, 0.1, 0.6)
        self.g0 = syn.gauge_field(seed, L, L, L, L)
        self.p0 = np.random.default_rng(seed + 1).standard_normal((lat.V, 4, 8))
        self.reset()
        self.pf = [lat.field(syn.spinor_field_eo(seed + 2 + q, 1, L, L, L, L)) for q in range(2 if kind == "ndrat" else 1)]
        self.iters = 0

    def reset(self):
        self.lat.set_gauge(self.g0)
        self.lat.momenta_upload(self.p0)

    def energy(self):
        lat = self.lat
        if self.kind == "ndrat":
            s, it = lat.ndrat_acc(self.pf[0], self.pf[1], self.MU, self.RMU, *self.SOLVE)
        else:
            s, it = lat.rat_acc(self.pf[0], self.MU, self.RMU, *self.SOLVE)
        assert it > 0
        p = lat.momenta_download()
        return 0.5 * float((p * p).sum()) + s

    def force(self, step):
        lat = self.lat
        lat.derivative_zero()
        if self.kind == "ndrat":
            it = lat.ndrat_derivative(self.pf[0], self.pf[1], self.MU, self.RMU, 0.6, *self.SOLVE)
        else:
            it = lat.rat_derivative(self.pf[0], self.MU, self.RMU, *self.SOLVE)
        assert it > 0
        self.iters += it
        lat.update_momenta(step)

    def leapfrog(self, nsteps, eps):
        self.force(0.5 * eps)
        for k in range(nsteps):
            self.lat.update_gauge(eps)
            self.force(eps if k < nsteps - 1 else 0.5 * eps)


@pytest.mark.parametrize("kind", ["ndrat", "rat"])
def test_leapfrog_with_the_rational_force_conserves_its_hamiltonian_to_second_order(kind):
    tr = RatTrajectory(kind)
    h0 = tr.energy()
    dh = {}
    for nsteps in (4, 8):                                               # trajectory length 0.2
        tr.reset()
        tr.leapfrog(nsteps, 0.2 / nsteps)
        dh[nsteps] = tr.energy() - h0
    tr.lat.close()
    print("%s: H0 = %.6f   dH(eps = 0.05) = %.3e   dH(eps = 0.025) = %.3e   ratio %.2f   CG iterations %d" % (kind, h0, dh[4], dh[8], dh[4] / dh[8], tr.iters))
    assert abs(dh[8]) < abs(dh[4])
    assert 3.0 < dh[4] / dh[8] < 5.5                                    # O(eps^2): a wrong forcefactor, a sign error or a dropped flavour leaves O(eps)


# ---------------------------------------------------------------- 8: drop-in
def test_drop_in_symbols(host_stub):
    """Q_tau1_sub_const_ndpsi and assign_add_mul under their reference names, and tmlqcd_hip_ndrat_derivative adding to hf->derivative
    (coherent mode) or holding back until tmlqcd_hip_flush_derivative (resident mode).  The stub program has no g_mubar / g_epsbar /
    phmc_invmaxev: the drop-in then works with 0, 0, 1."""
    from tmlqcd_amd import Lattice
    stub, d = host_stub
    VP, dbl = C.c_void_p, C.c_double
    T, L = 4, 4
    kappa, theta = 0.125, (1.0, 0.0, 0.0, 0.0)
    V = T * L ** 3
    N = V // 2
    gptr = stub.stub_init(T, L, L, L)
    g = random_gauge(95, V)
    C.memmove(gptr, g.ctypes.data_as(VP), g.nbytes)
    stub.stub_boundary(kappa, *theta)
    stub.stub_set_mu(0.0)
    lat = Lattice(T, L, L, L, kappa=kappa, mu=0.0, theta=theta)
    lat.set_gauge(g)
    lat.set_nd(0.0, 0.0, 1.0)
    hu, hd = random_spinor(97, N), random_spinor(98, N)
    pu, pd = lat.field(hu), lat.field(hd)
    ptr = lambda a: a.ctypes.data_as(VP)
    # the building blocks (complex by value: two consecutive doubles in the SysV ABI)
    d.Q_tau1_sub_const_ndpsi.argtypes = [VP] * 4 + [dbl] * 4
    d.Q_tau1_sub_const_ndpsi.restype = None
    d.assign_add_mul.argtypes = [VP, VP, dbl, dbl, C.c_int]
    d.assign_add_mul.restype = None
    z = 0.2 - 0.6j
    ls, lc = lat.field(), lat.field()
    lat.Q_tau1_sub_const_ndpsi(ls, lc, pu, pd, z, 1.0, 0.9)
    os_, oc_ = np.zeros((N, 4, 3, 2)), np.zeros((N, 4, 3, 2))
    d.Q_tau1_sub_const_ndpsi(ptr(os_), ptr(oc_), ptr(hu), ptr(hd), z.real, z.imag, 1.0, 0.9)
    assert np.array_equal(os_, ls.download()) and np.array_equal(oc_, lc.download())
    acc = hu.copy()
    d.assign_add_mul(ptr(acc), ptr(hd), z.real, z.imag, N)
    assert rel_err(acc, real(cplx(hu) + z * cplx(hd))) < TOL
    # the monomial body
    lat.derivative_zero()
    it0 = lat.ndrat_derivative(pu, pd, MU3, RMU3, 1.0, *SOLVE)
    ref = lat.derivative()

    class HF(C.Structure):        # hamiltonian_field.h:26-32
        _fields_ = [("gaugefield", VP), ("momenta", VP), ("derivative", VP), ("update_gauge_copy", C.c_int), ("traj_counter", C.c_int)]
    df_host = np.random.default_rng(96).standard_normal((V, 4, 8))
    start = df_host.copy()
    rows = (VP * V)(*[df_host.ctypes.data + 4 * 8 * 8 * i for i in range(V)])      # su3adj **derivative
    hf = HF(None, None, C.cast(rows, VP), 0, 0)
    pd_ = C.POINTER(dbl)
    d.tmlqcd_hip_ndrat_derivative.argtypes = [C.POINTER(HF), VP, VP, pd_, pd_, C.c_int, dbl, C.c_int, dbl, C.c_int]
    d.tmlqcd_hip_ndrat_derivative.restype = C.c_int
    d.tmlqcd_hip_flush_derivative.argtypes = [C.POINTER(HF)]
    d.tmlqcd_hip_set_residency.argtypes = [C.c_int]
    mu, rmu = (dbl * 3)(*MU3), (dbl * 3)(*RMU3)
    assert d.tmlqcd_hip_ndrat_derivative(C.byref(hf), ptr(hu), ptr(hd), mu, rmu, 3, 1.0, *SOLVE) == it0
    assert rel_err(df_host, start + ref) < TOL
    d.tmlqcd_hip_set_residency(1)
    assert d.tmlqcd_hip_ndrat_derivative(C.byref(hf), ptr(hu), ptr(hd), mu, rmu, 3, 1.0, *SOLVE) == it0
    assert rel_err(df_host, start + ref) < TOL                          # nothing flushed yet
    d.tmlqcd_hip_flush_derivative(C.byref(hf))
    assert rel_err(df_host, start + 2 * ref) < TOL
    d.tmlqcd_hip_set_residency(0)
    d.tmlqcd_hip_finalize()
    lat.close()
