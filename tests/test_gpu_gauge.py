"""GPU: the gauge monomial on the device-resident links (gauge.hip) -- tmhip_gauge_derivative and the three measures against the
reference's own outputs (tests/golden/ref_gauge_*), against the NumPy restatement (tests/gauge_restate.py) on other shapes, on T-split
contexts, through the drop-in, and as the force of a pure-gauge (and gauge + determinant) leapfrog trajectory.

Bounds: force rel_err < TOL (gather formulation, no atomics); sums |gpu - cpu| <= TOL * n_terms with n_terms = 6 V plaquettes /
12 V rectangles, each at most 1 after the / 3 (times the plane weight 1 + lambda where one applies)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import gauge_restate as gr
from tests.util import TOL, random_gauge, random_spinor, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
C1 = -0.331
IWASAKI = dict(c0=1.0 - 8.0 * C1, c1=C1, use_rectangles=True)
WILSON = dict(c0=1.0, c1=0.0, use_rectangles=False)


def _nonzero_derivative(lat, seed):
    """A non-zero device derivative field to accumulate onto: one deriv_Sb contribution of two random spinor fields."""
    l, k = lat.field(random_spinor(seed, lat.Vh)), lat.field(random_spinor(seed + 1, lat.Vh))
    lat.derivative_zero()
    lat.deriv_Sb(1, l, k, 0.7)
    d0 = lat.derivative()
    assert np.abs(d0).max() > 0.1
    return d0


def _check_scalars(lat, g, dims, lam=0.3):
    V = int(np.prod(dims))
    got = (lat.measure_plaquette(), lat.measure_gauge_action(0.0), lat.measure_gauge_action(lam), lat.measure_rectangles())
    want = (gr.measure_plaquette(g, dims), gr.measure_gauge_action(g, dims, 0.0), gr.measure_gauge_action(g, dims, lam), gr.measure_rectangles(g, dims))
    bounds = (TOL * 6 * V, TOL * 6 * V, TOL * 6 * V * (1 + lam), TOL * 12 * V)
    for a, b, bd, name in zip(got, want, bounds, ("plaquette", "action 0", "action lambda", "rectangles")):
        print("%s %s: gpu %.15e cpu %.15e |diff| %.3e bound %.3e" % (dims, name, a, b, abs(a - b), bd))
    for a, b, bd, name in zip(got, want, bounds, ("plaquette", "action 0", "action lambda", "rectangles")):
        assert abs(a - b) <= bd, name
    return got


def test_against_the_reference_fixtures_4x4():
    """Force (Wilson / Iwasaki, lambda 0 / 0.3, accumulated onto a non-zero derivative) and the five scalars == the reference."""
    from tmlqcd_amd import Lattice
    f = np.load(os.path.join(GOLD, "ref_gauge_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_gauge_scalars_4x4.json")))
    g = np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"][:256])
    lat = Lattice(4, 4, 4, 4)
    lat.set_gauge(g)
    seed = gr.seed_derivative(256)
    for name, c in s["cases"].items():
        d0 = _nonzero_derivative(lat, 40)
        lat.gauge_derivative(s["beta"], c["c0"], c["c1"], bool(c["use_rectangles"]), c["glambda"])
        got = lat.derivative()
        err = rel_err(got - d0, f[name] - seed)
        err_acc = rel_err(got, d0 + (f[name] - seed))
        print("4^4 %s: force rel err %.3e, accumulated %.3e" % (name, err, err_acc))
        assert err_acc < TOL and err < TOL, name
    V = 256
    b6, b12 = TOL * 6 * V, TOL * 12 * V
    assert abs(lat.measure_plaquette() - s["measure_plaquette"]) <= b6
    assert abs(lat.measure_gauge_action(0.0) - s["measure_gauge_action_0"]) <= b6
    assert abs(lat.measure_gauge_action(s["lambda"]) - s["measure_gauge_action_lambda"]) <= b6 * (1 + s["lambda"])
    assert abs(lat.measure_rectangles() - s["measure_rectangles"]) <= b12
    for name, c in s["cases"].items():                                   # gauge_heatbath's energy0
        e = s["beta"] * c["c0"] * lat.measure_gauge_action(c["glambda"])
        if c["use_rectangles"]:
            e += s["beta"] * c["c1"] * lat.measure_rectangles()
        assert abs(e - c["energy0"]) <= s["beta"] * (abs(c["c0"]) * b6 * (1 + c["glambda"]) + abs(c["c1"]) * b12), name
    lat.close()


@pytest.mark.parametrize("dims", [(8, 6, 4, 12), (4, 2, 6, 2), (2, 2, 2, 2), (16, 16, 16, 16)])
@pytest.mark.parametrize("moved", [False, True])
def test_against_the_restatement(dims, moved):
    """random_gauge links, and links after three update_gauge steps on the device; two consecutive calls are bit-identical."""
    from tmlqcd_amd import Lattice
    T, LX, LY, LZ = dims
    V = int(np.prod(dims))
    lat = Lattice(T, LX, LY, LZ)
    g = random_gauge(7, V)
    lat.set_gauge(g)
    if moved:
        lat.momenta_upload(np.random.default_rng(8).standard_normal((V, 4, 8)))
        for step in (0.05, -0.02, 0.03):
            lat.update_gauge(step)
        g = np.ascontiguousarray(lat.gauge_download()[:V])
    for kw, lam in ((WILSON, 0.0), (IWASAKI, 0.0), (WILSON, 0.3), (IWASAKI, 0.3)):
        lat.derivative_zero()
        lat.gauge_derivative(5.8, glambda=lam, **kw)
        a = lat.derivative()
        lat.derivative_zero()
        lat.gauge_derivative(5.8, glambda=lam, **kw)
        b = lat.derivative()
        assert np.array_equal(a, b)
        want = gr.gauge_derivative(g, dims, 5.8, glambda=lam, **kw)
        err = rel_err(a, want)
        print("%s moved %d rect %d lambda %.1f: force rel err %.3e" % (dims, moved, kw["use_rectangles"], lam, err))
        assert err < TOL
    d0 = _nonzero_derivative(lat, 50)                                   # accumulation next to a deriv_Sb contribution
    lat.gauge_derivative(5.8, **IWASAKI)
    assert rel_err(lat.derivative(), d0 + gr.gauge_derivative(g, dims, 5.8, **IWASAKI)) < TOL
    first = _check_scalars(lat, g, dims)
    again = (lat.measure_plaquette(), lat.measure_gauge_action(0.0), lat.measure_gauge_action(0.3), lat.measure_rectangles())
    assert first == again
    lat.close()


def test_needs_resident_links():
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    lat = Lattice(4, 4, 4, 4)
    for call in (lambda: lat.gauge_derivative(6.0), lat.measure_plaquette, lat.measure_gauge_action, lat.measure_rectangles):
        with pytest.raises(TmHipError):
            call()
    lat.close()


@pytest.mark.parametrize("T,L,world", [(2, 4, 2), (4, 4, 3)])
def test_on_t_slabs(T, L, world):
    """T-split contexts of one process after a multi_update_gauge: the plaquette force slab by slab == the unsplit restatement, the slab
    sums add up to the unsplit sums; rectangles reach two slices deep and are refused."""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    from tmlqcd_amd.hip import TmHipError, multi_update_gauge
    Tg = T * world
    dims = (Tg, L, L, L)
    orc = Oracle(Tg, L, L, L, kappa=0.13, mu=0.02, threads=4)
    g = syn.gauge_field(16, Tg, L, L, L)
    mom = np.random.default_rng(77).standard_normal((Tg * L ** 3, 4, 8))
    V = T * L ** 3
    lats = [Lattice(T, L, L, L, kappa=0.13, mu=0.02, nproc_t=world, proc_t=r) for r in range(world)]
    for r, lat in enumerate(lats):
        lat.set_gauge(syn.gauge_field(16, T, L, L, L, world, r))
        lat.momenta_upload(np.ascontiguousarray(mom[r * V:(r + 1) * V]))
    multi_update_gauge(lats, 0.05)
    orc.update_gauge(g, mom, 0.05)
    g = np.ascontiguousarray(g[:Tg * L ** 3])
    lam = 0.3
    tot_p, tot_a = 0.0, 0.0
    for r, lat in enumerate(lats):
        slab = (r * T, (r + 1) * T)
        lat.derivative_zero()
        lat.gauge_derivative(5.8, glambda=lam)
        err = rel_err(lat.derivative(), gr.gauge_derivative(g, dims, 5.8, glambda=lam, t_slab=slab))
        print("T-split %d/%d: force rel err %.3e" % (r, world, err))
        assert err < TOL, r
        p, a = lat.measure_plaquette(), lat.measure_gauge_action(lam)
        assert abs(p - gr.measure_plaquette(g, dims, t_slab=slab)) <= TOL * 6 * V
        assert abs(a - gr.measure_gauge_action(g, dims, lam, t_slab=slab)) <= TOL * 6 * V * (1 + lam)
        tot_p += p
        tot_a += a
        with pytest.raises(TmHipError):
            lat.gauge_derivative(5.8, **IWASAKI)
        with pytest.raises(TmHipError):
            lat.measure_rectangles()
    assert abs(tot_p - gr.measure_plaquette(g, dims)) <= TOL * 6 * V * world
    assert abs(tot_a - gr.measure_gauge_action(g, dims, lam)) <= TOL * 6 * V * world * (1 + lam)
    for lat in lats:
        lat.close()


def test_through_the_drop_in(host_stub):
    """The reference-named measures on host links; tmlqcd_hip_gauge_derivative in coherent mode next to a deriv_Sb contribution, held
    back then flushed in resident mode; after tmlqcd_hip_update_gauge in resident mode the device's newer links are the ones measured."""
    stub, d = host_stub
    VP = C.c_void_p
    T, L = 4, 6
    dims = (T, L, L, L)
    V = T * L ** 3
    N = V // 2
    gptr = stub.stub_init(T, L, L, L)
    g = random_gauge(295, V)
    C.memmove(gptr, g.ctypes.data_as(VP), g.nbytes)
    stub.stub_boundary(0.127, 1.0, 0.0, 0.0, 0.0)
    stub.stub_set_mu(0.01)

    class HF(C.Structure):        # hamiltonian_field.h:26-32
        _fields_ = [("gaugefield", VP), ("momenta", VP), ("derivative", VP), ("update_gauge_copy", C.c_int), ("traj_counter", C.c_int)]

    class GaugeInfo(C.Structure):  # io/params.h:98-104, first member
        _fields_ = [("plaquetteEnergy", C.c_double)]
    mom = np.random.default_rng(296).standard_normal((V, 4, 8))
    df_host = np.random.default_rng(297).standard_normal((V, 4, 8))
    start = df_host.copy()
    grows = (VP * V)(*[gptr + 4 * 144 * i for i in range(V)])
    mrows = (VP * V)(*[mom.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
    drows = (VP * V)(*[df_host.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
    hf = HF(C.cast(grows, VP), C.cast(mrows, VP), C.cast(drows, VP), 0, 0)
    for n in ("measure_plaquette", "measure_gauge_action", "measure_rectangles"):
        getattr(d, n).restype = C.c_double
    d.measure_plaquette.argtypes = [VP]
    d.measure_gauge_action.argtypes = [VP, C.c_double]
    d.measure_rectangles.argtypes = [VP]
    d.tmlqcd_hip_gauge_derivative.argtypes = [C.POINTER(HF)] + [C.c_double] * 3 + [C.c_int, C.c_double]
    d.tmlqcd_hip_gauge_derivative.restype = None
    d.deriv_Sb.argtypes = [C.c_int, VP, VP, C.POINTER(HF), C.c_double]
    d.deriv_Sb.restype = None
    d.tmlqcd_hip_flush_derivative.argtypes = [C.POINTER(HF)]
    d.tmlqcd_hip_update_gauge.argtypes = [C.c_double, C.POINTER(HF)]
    d.tmlqcd_hip_update_gauge.restype = None
    d.tmlqcd_hip_sync_gauge_to_host.argtypes = [C.POINTER(HF)]
    d.tmlqcd_hip_set_residency.argtypes = [C.c_int]
    gf = C.cast(grows, VP)
    b6, b12 = TOL * 6 * V, TOL * 12 * V

    def check_measures(links):
        assert abs(d.measure_plaquette(gf) - gr.measure_plaquette(links, dims)) <= b6
        a = d.measure_gauge_action(gf, 0.3)
        assert abs(a - gr.measure_gauge_action(links, dims, 0.3)) <= b6 * 1.3
        assert GaugeInfo.in_dll(d, "GaugeInfo").plaquetteEnergy == a               # measure_gauge_action.c:187
        assert abs(d.measure_rectangles(gf) - gr.measure_rectangles(links, dims)) <= b12
    check_measures(g)
    # coherent mode: next to a deriv_Sb contribution, both added to hf->derivative
    from oracle.oraclebind import Oracle
    orc = Oracle(T, L, L, L, kappa=0.127, mu=0.01, theta=(1.0, 0.0, 0.0, 0.0), threads=4)
    orc.set_gauge(g)
    l, k = random_spinor(298, N), random_spinor(299, N)
    lo, ko = orc.new_field(), orc.new_field(); lo[:N] = l; ko[:N] = k
    ref = np.zeros((orc.VPR, 4, 8))
    d.deriv_Sb(1, l.ctypes.data_as(VP), k.ctypes.data_as(VP), C.byref(hf), 0.9)
    orc.deriv_Sb(1, lo, ko, ref, 0.9)
    d.tmlqcd_hip_gauge_derivative(C.byref(hf), 5.8, IWASAKI["c0"], C1, 1, 0.3)
    want = start + ref[:V] + gr.gauge_derivative(g, dims, 5.8, glambda=0.3, **IWASAKI)
    assert rel_err(df_host, want) < TOL
    # resident mode: held back until the flush
    d.tmlqcd_hip_set_residency(1)
    d.tmlqcd_hip_gauge_derivative(C.byref(hf), 5.8, 1.0, 0.0, 0, 0.0)
    assert rel_err(df_host, want) < TOL
    d.tmlqcd_hip_flush_derivative(C.byref(hf))
    want = want + gr.gauge_derivative(g, dims, 5.8, **WILSON)
    assert rel_err(df_host, want) < TOL
    # resident mode: the device links move, the host's stay behind, the measures see the device's
    d.tmlqcd_hip_update_gauge(0.04, C.byref(hf))
    moved = g.copy()
    orc.update_gauge(moved, mom, 0.04)
    host_links = np.frombuffer((C.c_double * (V * 72)).from_address(gptr), dtype=np.float64).reshape(V, 4, 3, 3, 2)
    assert np.array_equal(host_links, g)
    check_measures(moved)
    assert abs(gr.measure_plaquette(moved, dims) - gr.measure_plaquette(g, dims)) > 1e3 * b6     # the two fields are told apart
    d.tmlqcd_hip_set_residency(0)
    d.tmlqcd_hip_sync_gauge_to_host(C.byref(hf))
    d.tmlqcd_hip_finalize()


@pytest.mark.parametrize("world", [2, 4])
def test_drop_in_measures_are_global_on_t_split_ranks(world, tmp_path):
    """The reference's measure_plaquette / measure_gauge_action end with an MPI_Allreduce: under their names every rank of a T split gets
    the sum over the WHOLE lattice (the same bits on every rank; GaugeInfo.plaquetteEnergy too), not its share, or gauge_heatbath /
    gauge_acc would accept and reject per rank.  Ranks are host processes with tmLQCD's own globals (tests/mp_gauge_worker.py), before
    and after a tmlqcd_hip_update_gauge; the plaquette force of each rank == its slab of the unsplit restatement."""
    import subprocess
    import sys
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import synthetic as syn
    worker = os.path.join(ROOT, "tests", "mp_gauge_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TMLQCD_HIP_FLAG_TIMEOUT_S="60")
    job = "ga_%d_%d" % (os.getpid(), world)
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), job, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=400) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    parts = [np.load(os.path.join(str(tmp_path), "gauge_%d_of_%d.npz" % (r, world))) for r in range(world)]
    Tg, L = 8, 4
    dims = (Tg, L, L, L)
    Vg = Tg * L ** 3
    T = Tg // world
    g = syn.gauge_field(51, Tg, L, L, L)
    mom = np.random.default_rng(52).standard_normal((Vg, 4, 8))
    orc = Oracle(Tg, L, L, L, kappa=0.13, mu=0.02, threads=4)
    for tag in ("start", "moved"):
        if tag == "moved":
            orc.update_gauge(g, mom, 0.05)
        links = np.ascontiguousarray(g[:Vg])
        want_p, want_a = gr.measure_plaquette(links, dims), gr.measure_gauge_action(links, dims, 0.3)
        for r in range(world):
            p_, a_, info = parts[r][tag + "_sums"]
            print("%s rank %d/%d: plaquette %.15e (cpu %.15e) action %.15e (cpu %.15e)" % (tag, r, world, p_, want_p, a_, want_a))
            assert abs(p_ - want_p) <= TOL * 6 * Vg and abs(a_ - want_a) <= TOL * 6 * Vg * 1.3, (tag, r)
            assert info == a_
            assert np.array_equal(parts[r][tag + "_sums"], parts[0][tag + "_sums"])          # the same bits on every rank
            want = gr.gauge_derivative(links, dims, 5.8, glambda=0.3, t_slab=(r * T, (r + 1) * T))
            assert rel_err(parts[r][tag + "_force"], want) < TOL, (tag, r)
        share = gr.measure_plaquette(links, dims, t_slab=(0, T))
        assert abs(share - want_p) > 1e3 * TOL * 6 * Vg                                        # a rank-local sum would not pass


class GaugeTrajectory:
    """Pure-gauge leapfrog with links, momenta and derivative resident: H = p^2 / 2 - E, E = beta (c0 S_plaq + c1 S_rect) as
    gauge_heatbath / gauge_acc measure it (gauge_acc returns E_old - E_new as the monomial's part of dH)."""
    L, BETA, TAU = 8, 5.6, 0.05

    def __init__(self, action):
        from tmlqcd_amd import Lattice
        L = self.L
        self.kw = action
        self.lat = Lattice(L, L, L, L)
        self.g0 = random_gauge(1, L ** 4)
        self.p0 = np.random.default_rng(2).standard_normal((L ** 4, 4, 8))
        self.reset()

    def reset(self):
        self.lat.set_gauge(self.g0)
        self.lat.momenta_upload(self.p0)

    def energy(self):
        p = self.lat.momenta_download()
        e = self.BETA * self.kw["c0"] * self.lat.measure_gauge_action(0.0)
        if self.kw["use_rectangles"]:
            e += self.BETA * self.kw["c1"] * self.lat.measure_rectangles()
        return 0.5 * float((p * p).sum()) - e

    def force(self, step):
        self.lat.derivative_zero()
        self.lat.gauge_derivative(self.BETA, **self.kw)
        self.lat.update_momenta(step)

    def leapfrog(self, nsteps, eps):
        self.force(0.5 * eps)
        for k in range(nsteps):
            self.lat.update_gauge(eps)
            self.force(eps if k < nsteps - 1 else 0.5 * eps)


@pytest.mark.parametrize("action", [WILSON, IWASAKI], ids=["wilson", "iwasaki"])
def test_pure_gauge_leapfrog(action):
    """dH falls by the factor 4 between 4 and 8 steps and the trajectory is reversible.  beta 5.6, trajectory length 0.05, start
    tests.util.random_gauge(1, V) with Gaussian momenta (seed 2) were chosen by running this leapfrog on tests/gauge_restate.py on the
    CPU, which alone gave  Wilson: H0 = 65707.870, dH(4) = -0.65971, dH(8) = -0.16510, ratio 3.996;
    Iwasaki: H0 = 66183.136, dH(4) = -9.1800, dH(8) = -2.3051, ratio 3.982."""
    tr = GaugeTrajectory(action)
    h0 = tr.energy()
    dh = {}
    for nsteps in (4, 8):
        tr.reset()
        tr.leapfrog(nsteps, tr.TAU / nsteps)
        dh[nsteps] = tr.energy() - h0
    p = tr.lat.momenta_download()
    tr.lat.momenta_upload(-p)
    tr.leapfrog(8, tr.TAU / 8)
    back = tr.lat.gauge_download()[:tr.lat.V]
    pend = tr.lat.momenta_download()
    tr.lat.close()
    print("pure gauge rect %d: H0 = %.6f   dH(4) = %.5e   dH(8) = %.5e   ratio %.3f" % (action["use_rectangles"], h0, dh[4], dh[8], dh[4] / dh[8]))
    assert 3.0 < dh[4] / dh[8] < 5.5
    assert np.abs(back - tr.g0).max() < 1e-10
    assert np.abs(pend + tr.p0).max() < 1e-9


@pytest.mark.parametrize("action", [WILSON, IWASAKI], ids=["wilson", "iwasaki"])
def test_gauge_plus_determinant_leapfrog(action):
    """The determinant trajectory of tests/test_gpu_md_trajectory.py with the gauge monomial added: both forces in ONE derivative field,
    H = p^2 / 2 + S_det - E_gauge.  That test's start field and momenta, beta 5.6, trajectory length 0.1: the gauge part alone, run on
    tests/gauge_restate.py on the CPU from this start, gave the ratios 3.986 (Wilson: dH(4) = -11.722, dH(8) = -2.9410) and 3.966
    (Iwasaki: -295.59, -74.532)."""
    from tests.test_gpu_md_trajectory import EO, OE, DetTrajectory
    beta = 5.6

    class Both(DetTrajectory):
        def gauge_energy(self):
            e = beta * action["c0"] * self.lat.measure_gauge_action(0.0)
            if action["use_rectangles"]:
                e += beta * action["c1"] * self.lat.measure_rectangles()
            return e

        def energy(self):
            return DetTrajectory.energy(self) - self.gauge_energy()

        def force(self, step):
            lat = self.lat
            lat.derivative_zero()
            lat.gauge_derivative(beta, **action)
            self.solve()
            lat.H_eo_tm_inv_psi(self.w2, self.X, EO, -1.0)
            lat.deriv_Sb(OE, self.Y, self.w2, 1.0)
            lat.H_eo_tm_inv_psi(self.w3, self.Y, EO, +1.0)
            lat.deriv_Sb(EO, self.w3, self.X, 1.0)
            lat.update_momenta(step)
    tr = Both()
    tau = 0.1
    h0 = tr.energy()
    dh = {}
    for nsteps in (4, 8):
        tr.reset()
        tr.leapfrog(nsteps, tau / nsteps)
        dh[nsteps] = tr.energy() - h0
    p = tr.lat.momenta_download()
    tr.lat.momenta_upload(-p)
    tr.leapfrog(8, tau / 8)
    back = tr.lat.gauge_download()[:tr.lat.V]
    pend = tr.lat.momenta_download()
    tr.close()
    print("gauge + det rect %d: H0 = %.6f   dH(4) = %.5e   dH(8) = %.5e   ratio %.3f" % (action["use_rectangles"], h0, dh[4], dh[8], dh[4] / dh[8]))
    assert 3.0 < dh[4] / dh[8] < 5.5
    assert np.abs(back - tr.g0).max() < 1e-10
    assert np.abs(pend + tr.p0).max() < 1e-9
