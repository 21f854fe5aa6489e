"""GPU: the frame of a trajectory on the device (md_update.hip, trajectory.hip): gauge_snapshot / gauge_restore / gauge_reunitarize,
gauge_snapshot_diff, moment_energy, derivative_norms -- what update_tm.c does around the integrator, on the resident fields.

Shapes are those of tests/test_gpu_md_update.py, where links_kernel's blocks are partial: (2,2,2,2) 64 links in one block, (2,2,2,6) a
partial block of another size, (6,2,2,6) three blocks with the last partial, (8,6,4,12) many whole blocks and every wrap; 4^4 for the
fixtures of tools/make_golden_traj.py; T-split ranks as contexts of one process.

* (1) test_snapshot_restore_is_exact: links and every probe of the derived state (both parities of the fp64 stencil, the fp32 stencil,
  Qsw_pm_psi after sw_term / sw_invert) return bit for bit; the clover blocks are stale in between;
* (2) test_reunitarize: against the reference's restoresu3_in_place (fixture) and its NumPy restatement, the stencil on the new links;
* (3) test_t_slabs: halo slabs without an exchange, snapshot / restore and the shares of the sums on slabs;
* (4) test_sums: the three reductions against math.fsum and the reference's values; the bound is derived below from the launch geometry;
* (5) test_trajectory: a determinant trajectory that uses all of it: reject, accept, reversibility;
* (7) test_errors: the refusals.

Bound of the sums.  Every term is non-negative, so a term that passes through at most n additions and roundings on its way into the
result carries a relative error of at most n 2^-53 (to first order; n <= 64 keeps the second order below 2^-100).  n is read off the
kernels in trajectory.hip and tmhip_reduce_finish -- chain_* below -- and asserted to stay <= 64 on every shape used here."""
import json
import math
import os

import numpy as np
import pytest

from tests import traj_restate as tj
from tests.util import TOL, random_gauge, random_spinor, rel_err

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAPPA, MU, THETA = 0.131, 0.02, (1.0, 0.5, -0.25, 0.125)
C_SW = 1.57
SHAPES = [(2, 2, 2, 2), (2, 2, 2, 6), (6, 2, 2, 6), (8, 6, 4, 12), (4, 4, 4, 4)]
SLABS = [((2, 2, 6, 2), 3), ((4, 6, 2, 4), 2)]
FIXTURE = {(4, 4, 4, 4): "4x4", (8, 6, 4, 12): "8x6x4x12"}
U = tj.U53
ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]
slab_ids = ["%s_x%d" % ("x".join(map(str, s)), w) for s, w in SLABS]


# ------------------------------------------------------------------ the launch geometry: tests/traj_restate.py (max_partials, chain_*)
max_partials, chain_energy, chain_diff, chain_norms = tj.max_partials, tj.chain_energy, tj.chain_diff, tj.chain_norms


def test_the_chains_stay_short():
    """the cap that keeps the derived bound from hiding a bug: n <= 64 on every shape of this file"""
    for s in SHAPES + [loc for loc, _ in SLABS] + [(8, 8, 8, 8)]:
        n = (chain_energy(s), chain_diff(s), chain_norms(s))
        print(s, "max_partials", max_partials(s), "n (energy, diff, norms) =", n)
        assert max(n) <= 64, (s, n)


def close_to(got, exact, n, what):
    err = abs(got - exact) / (U * abs(exact)) if exact else abs(got)
    print("%s: %.17g against %.17g: %.2f x 2^-53 (allowed %d)" % (what, got, exact, err, n))
    assert abs(got - exact) <= n * U * abs(exact), (what, got, exact, err, n)


def scalars(shape):
    return json.load(open(os.path.join(GOLD, "ref_traj_scalars_%s.json" % FIXTURE[shape])))


# ------------------------------------------------------------------ probes of the state derived from the links
def _lattice(shape, **kw):
    from tmlqcd_amd import Lattice
    return Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA, **kw)


class Probes:
    """Outputs of everything that reads a copy of the links: the fp64 stencil of both parities (the two parities and the backward
    slots of the stencil's copy, its packed twin), the fp32 stencil (the fp32 twin), Qsw_pm_psi (the clover blocks)."""

    def __init__(self, lat):
        self.lat, N = lat, lat.Vh
        k = random_spinor(5, N)
        self.dk, self.dl = lat.field(k), lat.field()
        self.dk32, self.dl32 = lat.field32(k.astype(np.float32)), lat.field32()

    def links(self):
        lat, out = self.lat, {}
        for ieo in (0, 1):
            lat.Hopping_Matrix(ieo, self.dl, self.dk)
            out["Hopping_Matrix(%d)" % ieo] = self.dl.download()
            lat.Hopping_Matrix_32(ieo, self.dl32, self.dk32)
            out["Hopping_Matrix_32(%d)" % ieo] = self.dl32.download()
        return out

    def clover(self):
        lat = self.lat
        lat.sw_term(None, KAPPA, C_SW)
        lat.sw_invert(0, MU)
        lat.op("Qsw_pm_psi", self.dl, self.dk)
        return {"Qsw_pm_psi": self.dl.download()}

    def clover_is_stale(self):
        from tmlqcd_amd.hip import TmHipError
        with pytest.raises(TmHipError):
            self.lat.op("Qsw_pm_psi", self.dl, self.dk)
        with pytest.raises(TmHipError):
            self.lat.sw_invert(0, MU)


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def moved(a, b, what):
    for k in a:
        assert not np.array_equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------ (1)
def _snapshot_restore(shape, recon12):
    lat = _lattice(shape)
    g = random_gauge(3, lat.VPR)
    lat.set_gauge(g)
    lat.momenta_upload(tj.momenta(shape))
    if recon12:
        lat.set_option("block", 256)
        lat.set_option("gauge_recon", 12)
    pr = Probes(lat)
    before = dict(pr.links(), **pr.clover())
    lat.gauge_snapshot()
    lat.update_gauge(0.1)
    lat.update_gauge(0.1)
    pr.clover_is_stale()
    mid = dict(pr.links(), **pr.clover())
    moved(before, mid, "after two steps of 0.1")
    assert rel_err(lat.gauge_download(), g) > 1e-3
    guard_held = lat.gauge_su3_deviation() <= 1e-13   # (recon12: above it the option is given up for good, as after any update_gauge)
    lat.gauge_restore()
    assert np.array_equal(lat.gauge_download(), g)
    pr.clover_is_stale()
    after = dict(pr.links(), **pr.clover())
    if recon12 and not guard_held:
        # the 12-real read was refused on the moved links and stays off: the restored links are read in full, exactly as a context does
        # that never had the option
        twin = _lattice(shape)
        twin.set_gauge(g)
        tp = Probes(twin)
        before = dict(tp.links(), **tp.clover())
        twin.close()
    same(before, after, "%s restored" % (shape,))
    # a second restore from the same snapshot, and a snapshot that survives set_gauge
    lat.set_gauge(random_gauge(4, lat.VPR))
    lat.gauge_restore()
    assert np.array_equal(lat.gauge_download(), g)
    same(before, dict(pr.links(), **pr.clover()), "%s restored after set_gauge" % (shape,))
    lat.gauge_snapshot_free()
    lat.gauge_snapshot_free()
    lat.close()


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_snapshot_restore_is_exact(shape):
    _snapshot_restore(shape, False)


@gpu
def test_snapshot_restore_is_exact_under_the_12_real_read():
    _snapshot_restore((8, 6, 4, 12), True)


# ------------------------------------------------------------------ (2)
@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_reunitarize(shape):
    from oracle.oraclebind import Oracle
    lat = _lattice(shape)
    orc = Oracle(*shape, kappa=KAPPA, mu=MU, theta=THETA, threads=8)
    noisy = tj.noisy_gauge(shape)
    lat.set_gauge(noisy)
    lat.momenta_upload(tj.momenta(shape))
    pr = Probes(lat)
    old = dict(pr.links(), **pr.clover())
    dev0 = lat.gauge_su3_deviation()
    assert dev0 > 1e-4, dev0
    lat.gauge_reunitarize()
    pr.clover_is_stale()
    got = lat.gauge_download()
    want = tj.restoresu3(noisy)
    err = rel_err(got, want)
    dev1 = lat.gauge_su3_deviation()
    print("%s reunitarize: rel err to the restatement %.3e, SU(3) deviation %.3e -> %.3e" % (shape, err, dev0, dev1))
    assert err < TOL, err
    assert dev1 < 1e-13, dev1
    if shape in FIXTURE and FIXTURE[shape] == "4x4":
        ref = np.load(os.path.join(GOLD, "ref_traj_4x4.npz"))["reunitarized"]
        eref = rel_err(got, ref)
        print("%s reunitarize: rel err to the reference's restoresu3_in_place %.3e" % (shape, eref))
        assert eref < TOL, eref
    # the stencil reads the new links: both parities against the oracle on the downloaded links, fp32 and clover moved with them
    orc.set_gauge(got)
    k = pr.dk.download()
    ref_f = orc.new_field()
    new = dict(pr.links(), **pr.clover())
    moved(old, new, "reunitarized")
    for ieo in (0, 1):
        orc.Hopping_Matrix(ieo, ref_f, k)
        e = rel_err(new["Hopping_Matrix(%d)" % ieo], ref_f[:orc.Vh])
        print("%s Hopping_Matrix(%d) on the reunitarized links rel err %.3e" % (shape, ieo, e))
        assert e < TOL, (ieo, e)
    # the fused pass wrote, into both slots of every link, exactly what the plain re-sort of the same links writes
    twin = _lattice(shape)
    twin.set_gauge(got)
    tp = Probes(twin)
    same(dict(tp.links(), **tp.clover()), new, "%s twin" % (shape,))
    twin.close()
    # idempotent up to rounding
    lat.gauge_reunitarize()
    again = lat.gauge_download()
    change = float(np.abs(again - got).max() / np.abs(got).max())
    print("%s second reunitarize changes the links by %.3e" % (shape, change))
    assert change < 4 * 2.0 ** -52, change
    assert np.array_equal(lat.momenta_download(), tj.momenta(shape))
    lat.close()


# ------------------------------------------------------------------ (3)
@gpu
@pytest.mark.parametrize("local,world", SLABS, ids=slab_ids)
def test_t_slabs(local, world):
    from oracle.oraclebind import Oracle
    from tmlqcd_amd.hip import multi_Hopping_Matrix, multi_update_gauge
    T, LX, LY, LZ = local
    dims = (T * world, LX, LY, LZ)
    XYZ = LX * LY * LZ
    V = T * XYZ
    Vh = V // 2
    orc = Oracle(*dims, kappa=KAPPA, mu=MU, theta=THETA, threads=8)
    noisy, mom, df = tj.noisy_gauge(dims), tj.momenta(dims), tj.derivative(dims)
    sl = lambda a, r: a[r * V:(r + 1) * V]
    lats = [_lattice(local, nproc_t=world, proc_t=r) for r in range(world)]
    for r, lat in enumerate(lats):
        up, dn = (r + 1) % world, (r - 1) % world
        lat.set_gauge(np.ascontiguousarray(np.concatenate([sl(noisy, r), sl(noisy, up)[:XYZ], sl(noisy, dn)[V - XYZ:]])))
        lat.momenta_upload(np.ascontiguousarray(sl(mom, r)))
        lat.derivative_upload(np.ascontiguousarray(sl(df, r)))
    kin = [random_spinor(15, orc.Vh), random_spinor(16, orc.Vh)]
    ls = [lat.field() for lat in lats]

    def stencil():
        out = []
        for ieo in (0, 1):
            ks = [lat.field(np.ascontiguousarray(kin[ieo][r * Vh:(r + 1) * Vh])) for r, lat in enumerate(lats)]
            multi_Hopping_Matrix(lats, ieo, ls, ks)
            out.append([f.download() for f in ls])
        return out

    # accept on every rank: no exchange, and the slabs are the neighbours' slices
    for lat in lats:
        lat.gauge_reunitarize()
    down = [lat.gauge_download() for lat in lats]
    want = tj.restoresu3(noisy)
    for r in range(world):
        up, dn = (r + 1) % world, (r - 1) % world
        assert np.array_equal(down[r][V:V + XYZ], down[up][:XYZ]) and np.array_equal(down[r][V + XYZ:], down[dn][V - XYZ:V]), r
        err = rel_err(down[r][:V], sl(want, r))
        print("%s x %d rank %d: reunitarized links rel err %.3e" % (local, world, r, err))
        assert err < TOL, (r, err)
        assert lats[r].gauge_su3_deviation() < 1e-13
    whole = np.ascontiguousarray(np.concatenate([d[:V] for d in down]))
    orc.set_gauge(whole)
    ref = orc.new_field()
    first = stencil()
    for ieo in (0, 1):
        orc.Hopping_Matrix(ieo, ref, kin[ieo])
        for r in range(world):
            err = rel_err(first[ieo][r], ref[r * Vh:(r + 1) * Vh])
            print("%s x %d rank %d: multi_Hopping_Matrix(%d) on the reunitarized links rel err %.3e" % (local, world, r, ieo, err))
            assert err < TOL, (r, ieo, err)
    # snapshot, two steps, reject
    for lat in lats:
        lat.gauge_snapshot()
        assert lat.gauge_snapshot_diff() == 0.0
    multi_update_gauge(lats, 0.1)
    multi_update_gauge(lats, 0.1)
    mid = stencil()
    assert all(not np.array_equal(mid[i][r], first[i][r]) for i in (0, 1) for r in range(world))
    for lat in lats:
        lat.gauge_restore()
    for r, lat in enumerate(lats):
        assert np.array_equal(lat.gauge_download(), down[r]), r
    last = stencil()
    assert all(np.array_equal(last[i][r], first[i][r]) for i in (0, 1) for r in range(world))
    # the shares of the three sums add up to the unsplit values
    multi_update_gauge(lats, tj.DIFF_STEP)
    now = np.ascontiguousarray(np.concatenate([lat.gauge_download()[:V] for lat in lats]))
    shares = [(lat.moment_energy(), lat.gauge_snapshot_diff(), lat.derivative_norms()) for lat in lats]
    again = [(lat.moment_energy(), lat.gauge_snapshot_diff(), lat.derivative_norms()) for lat in lats]
    assert shares == again
    extra = world - 1                                          # the additions of the shares below
    close_to(math.fsum(s[0] for s in shares), tj.moment_energy(mom)[1], chain_energy(local) + extra, "%s x %d moment_energy" % (local, world))
    close_to(math.fsum(s[1] for s in shares), tj.snapshot_diff(now, whole)[1], chain_diff(local) + extra, "%s x %d gauge_snapshot_diff" % (local, world))
    plain, exact, mx = tj.derivative_norms(df)
    close_to(math.fsum(s[2][0] for s in shares), exact, chain_norms(local) + extra, "%s x %d derivative_norms sum" % (local, world))
    assert abs(max(s[2][1] for s in shares) - mx) <= 8 * U * mx
    for r in range(world):
        assert abs(shares[r][2][1] - tj.derivative_norms(sl(df, r))[2]) <= 8 * U * mx, r
    for lat in lats:
        lat.close()


# ------------------------------------------------------------------ (4)
@pytest.fixture(scope="module")
def oracle_moved():
    """gauge(shape) after update_gauge(momenta, 1e-3) by the CPU oracle: the second field of the fixtures' gauge_diff (made once)"""
    from oracle.oraclebind import Oracle
    out = {}
    for shape in SHAPES:
        g = tj.gauge(shape)
        Oracle(*shape, kappa=KAPPA, mu=MU).update_gauge(g, tj.momenta(shape), tj.DIFF_STEP)
        out[shape] = g
    return out


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_sums(shape, oracle_moved):
    lat = _lattice(shape)
    V = lat.V
    g, mom, df = tj.gauge(shape), tj.momenta(shape), tj.derivative(shape)
    fix = scalars(shape) if shape in FIXTURE else None
    ne, nd, nn = chain_energy(shape), chain_diff(shape), chain_norms(shape)

    # moment_energy
    lat.momenta_upload(mom)
    e = lat.moment_energy()
    assert lat.moment_energy() == e
    plain, exact = tj.moment_energy(mom)
    close_to(e, exact, ne, "%s moment_energy vs fsum" % (shape,))
    if fix:
        close_to(e, fix["moment_energy"], ne + 4, "%s moment_energy vs the reference" % (shape,))
    assert np.array_equal(lat.momenta_download(), mom)

    # gauge_snapshot_diff: identical fields, then the fixture's pair, then the device's own step
    lat.set_gauge(g)
    lat.gauge_snapshot()
    assert lat.gauge_snapshot_diff() == 0.0
    lat.set_gauge(oracle_moved[shape])                           # (leaves the snapshot alone)
    d = lat.gauge_snapshot_diff()
    assert lat.gauge_snapshot_diff() == d
    plain, exact = tj.snapshot_diff(oracle_moved[shape], g)
    close_to(d, exact, nd, "%s gauge_snapshot_diff vs fsum" % (shape,))
    if fix:
        close_to(d, fix["gauge_diff"], nd + 4, "%s gauge_snapshot_diff vs the reference" % (shape,))
    lat.set_gauge(g)
    lat.update_gauge(tj.DIFF_STEP)
    d = lat.gauge_snapshot_diff()
    assert lat.gauge_snapshot_diff() == d
    close_to(d, tj.snapshot_diff(lat.gauge_download()[:V], g)[1], nd, "%s gauge_snapshot_diff after update_gauge(1e-3) vs fsum" % (shape,))
    lat.gauge_restore()
    assert lat.gauge_snapshot_diff() == 0.0 and np.array_equal(lat.gauge_download(), g)

    # derivative_norms
    lat.derivative_upload(df)
    assert np.array_equal(lat.derivative(), df)
    s, m = lat.derivative_norms()
    assert lat.derivative_norms() == (s, m)
    plain, exact, mx = tj.derivative_norms(df)
    close_to(s, exact, nn, "%s derivative_norms sum vs fsum" % (shape,))
    print("%s derivative_norms max %.17g against %.17g" % (shape, m, mx))
    assert abs(m - mx) <= 8 * U * mx
    if fix:
        # monitor_forces.c adds its per-link norms in a plain serial loop: within (links - 1) 2^-53 of the exact sum (recursive summation)
        close_to(s, fix["force_sum"], nn + 4 * V - 1, "%s derivative_norms sum vs the reference" % (shape,))
        assert abs(m - fix["force_max"]) <= 8 * U * mx
    # a single non-zero link, the last one of the last block (odd parity, direction 3, last e/o index)
    one = np.zeros_like(df)
    one[V - 2, 3] = np.arange(1.0, 9.0) * 0.37
    lat.derivative_upload(one)
    s, m = lat.derivative_norms()
    want = float(tj.adj_sqnorm(one[V - 2, 3]))
    print("%s single link: sum %.17g max %.17g want %.17g" % (shape, s, m, want))
    assert abs(s - want) <= 8 * U * want and abs(m - want) <= 8 * U * want and s == m
    lat.derivative_zero()
    assert lat.derivative_norms() == (0.0, 0.0)
    lat.close()


# ------------------------------------------------------------------ (5)
EO, OE = 0, 1


class DetTrajectory:
    """tests/test_gpu_md_trajectory.py's, with the energy taken on the device: moment_energy() instead of a download of the momenta"""

    def __init__(self, L=8, kappa=0.125, mu=0.25, seed=5):
        from tmlqcd_amd import Lattice
        from tmlqcd_amd import synthetic as syn
        self.lat = lat = Lattice(L, L, L, L, kappa=kappa, mu=mu)
        self.g0 = syn.gauge_field(seed, L, L, L, L)
        rng = np.random.default_rng(seed + 1)
        self.p0 = rng.standard_normal((lat.V, 4, 8))
        self.R = lat.field(syn.spinor_field_eo(seed + 2, 1, L, L, L, L))       # det_heatbath (:177-180): phi = Q_+ R, R Gaussian
        self.phi, self.X, self.Y, self.w2, self.w3 = (lat.field() for _ in range(5))
        lat.set_gauge(self.g0)
        lat.momenta_upload(self.p0)
        lat.op("Qtm_plus_psi", self.phi, self.R)
        self.iters = 0

    def solve(self):
        lat = self.lat
        self.X.zero()
        it, _ = lat.cg_her(self.X, self.phi, 2000, 1e-26, 1, lat.Vh)
        assert it > 0
        self.iters += it
        lat.op("Qtm_minus_psi", self.Y, self.X)

    def action(self):
        self.solve()                                                    # det_acc: S = |Q_- (Q_+ Q_-)^-1 phi|^2
        return self.lat.square_norm(self.Y, self.lat.Vh, 1)

    def force(self, step):
        lat = self.lat
        lat.derivative_zero()
        self.solve()
        lat.H_eo_tm_inv_psi(self.w2, self.X, EO, -1.0)
        lat.deriv_Sb(OE, self.Y, self.w2, 1.0)
        lat.H_eo_tm_inv_psi(self.w3, self.Y, EO, +1.0)
        lat.deriv_Sb(EO, self.w3, self.X, 1.0)
        lat.update_momenta(step)

    def leapfrog(self, nsteps, eps):
        self.force(0.5 * eps)
        for k in range(nsteps):
            self.lat.update_gauge(eps)
            self.force(eps if k < nsteps - 1 else 0.5 * eps)


@gpu
def test_trajectory():
    shape = (8, 8, 8, 8)
    ne, nd = chain_energy(shape), chain_diff(shape)
    tr = DetTrajectory()
    lat, V = tr.lat, tr.lat.V
    nsteps, eps = 4, 0.05

    def trajectory():
        """update_tm.c:109-166 with the momenta already drawn: snapshot, energies, integrate, energies; returns (dH, its momenta part)"""
        lat.gauge_snapshot()
        enep, s0 = lat.moment_energy(), tr.action()
        tr.leapfrog(nsteps, eps)
        enepx, s1 = lat.moment_energy(), tr.action()
        return (s1 - s0) + (enepx - enep), enep, enepx, s0, s1

    dh, enep, enepx, s0, s1 = trajectory()
    close_to(enep, tj.moment_energy(tr.p0)[1], ne, "moment_energy of the drawn momenta")
    p = lat.momenta_download()
    close_to(enepx, tj.moment_energy(p)[1], ne, "moment_energy at the end of the trajectory")
    host = 0.5 * float((p * p).sum())
    assert abs(enepx - host) <= (ne + 64) * U * host                 # (NumPy's pairwise sum: its own 64)
    dh_host = (s1 - s0) + (host - 0.5 * float((tr.p0 * tr.p0).sum()))
    print("dH = %.12e on the device, %.12e with downloaded momenta; H = %.6f" % (dh, dh_host, enep + s0))
    assert abs(dh - dh_host) <= 2 * (ne + 64) * U * (enep + enepx)
    assert abs(dh) < 2e-4 * abs(enep + s0)                           # the bound tests/test_gpu_md_trajectory.py holds eps = 0.05 to
    # reject: the links return bit for bit, and the same momenta give the same trajectory bit for bit
    moved_by = lat.gauge_snapshot_diff()
    assert moved_by / (12 * V) > 1e-3
    lat.gauge_restore()
    assert np.array_equal(lat.gauge_download(), tr.g0)
    lat.momenta_upload(tr.p0)
    again = trajectory()
    assert again == (dh, enep, enepx, s0, s1), (again, dh)
    assert lat.gauge_snapshot_diff() == moved_by
    # reversibility (update_tm.c:185-289): flip, integrate back, ddU = ret_gauge_diff / 4 / VOLUME / 3
    lat.momenta_upload(-lat.momenta_download())
    tr.leapfrog(nsteps, eps)
    ddu = lat.gauge_snapshot_diff()
    back = lat.gauge_download()[:V]
    close_to(ddu, tj.snapshot_diff(back, tr.g0)[1], nd, "ret_gauge_diff")
    print("ddU = %.3e, max |dU| = %.3e" % (ddu / (12 * V), np.abs(back - tr.g0).max()))
    assert ddu / (12 * V) < 1e-10 and np.abs(back - tr.g0).max() < 1e-10
    # accept (of the links as they are now): back on the group, the plaquette does not notice
    plaq = lat.measure_plaquette()
    lat.gauge_reunitarize()
    assert abs(lat.measure_plaquette() - plaq) <= 1e-13 * abs(plaq)
    assert lat.gauge_su3_deviation() < 1e-13
    assert rel_err(lat.gauge_download()[:V], tj.restoresu3(back)) < TOL
    lat.close()


# ------------------------------------------------------------------ (7)
@gpu
def test_errors(capfd):
    from tmlqcd_amd.hip import TmHipError
    shape = (2, 2, 2, 6)
    lat = _lattice(shape)
    g = random_gauge(3, lat.VPR)

    def refused(call, word):
        capfd.readouterr()
        with pytest.raises(TmHipError):
            call()
        err = capfd.readouterr().err
        assert "[tmlqcd_hip]" in err and word in err, err

    refused(lat.gauge_snapshot, "not resident")                  # no links
    refused(lat.gauge_reunitarize, "not resident")
    refused(lat.gauge_restore, "no snapshot")
    refused(lat.gauge_snapshot_diff, "no snapshot")
    refused(lat.moment_energy, "no momenta")
    refused(lat.derivative_norms, "no derivative")
    lat.set_gauge(g)
    refused(lat.gauge_restore, "no snapshot")                    # links, still no snapshot
    refused(lat.gauge_snapshot_diff, "no snapshot")
    lat.gauge_snapshot()
    lat.gauge_snapshot_free()
    refused(lat.gauge_restore, "no snapshot")                    # freed
    refused(lat.derivative_norms, "no derivative")
    # ... and the context is as usable as before
    assert np.array_equal(lat.gauge_download(), g)
    lat.gauge_snapshot()
    assert lat.gauge_snapshot_diff() == 0.0
    lat.momenta_upload(tj.momenta(shape))
    close_to(lat.moment_energy(), tj.moment_energy(tj.momenta(shape))[1], chain_energy(shape), "moment_energy after the refusals")
    lat.derivative_zero()
    assert lat.derivative_norms() == (0.0, 0.0)
    lat.gauge_restore()
    assert np.array_equal(lat.gauge_download(), g)
    lat.close()
