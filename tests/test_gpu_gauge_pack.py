"""The packed link read of the fp64 stencil (option gauge_pack): 121 instead of 144 bytes per link, bit for bit.

Everything here compares gauge_pack 0 with the default in one process, with np.array_equal on downloaded fields and equal iteration
counts -- never a tolerance.  Shapes: the smallest that reach the staged 256-thread kernel with set_option("block", 256), one of them
non-cubic, both with twisted boundary phases."""
import numpy as np
import pytest

from tests.util import TOL, random_spinor, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4, 16, 16), (6, 8, 8, 16)]
KAPPA, MU, THETA = 0.137, 0.011, (1.0, 0.3, -0.2, 0.5)
C1 = 0.83 - 0.41j


def _lattice(shape, g):
    from tmlqcd_amd import Lattice
    lat = Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA)
    lat.set_option("block", 256)
    lat.set_gauge(g)
    return lat


def _gauge(shape, seed=7):
    from tmlqcd_amd import synthetic as syn
    return syn.gauge_field(seed, *shape)


def _battery(lat, N, k, p, cg=True):
    """Hopping_Matrix (both parities), tm_times_ / tm_sub_Hopping_Matrix, Qtm_pm_psi and cg_her to 1e-20: downloaded fields + iterations."""
    dk, dp, dl = lat.field(k), lat.field(p), lat.field()
    out = []
    for ieo in (0, 1):
        lat.Hopping_Matrix(ieo, dl, dk); out.append(dl.download())
        lat.tm_times_Hopping_Matrix(ieo, dl, dk, C1); out.append(dl.download())
        lat.tm_sub_Hopping_Matrix(ieo, dl, dp, dk, C1); out.append(dl.download())
    lat.Qtm_pm_psi(dl, dk); out.append(dl.download())
    iters = None
    if cg:
        dl.zero()
        iters, _ = lat.cg_her(dl, dk, 1000, 1e-20, 1, N)
        out.append(dl.download())
    for f in (dk, dp, dl):
        f.free()
    return out, iters


def _assert_same_with_and_without(lat, N, k, p, cg=True, packed=True, battery=None):
    """The battery with gauge_pack 0 and with the default, bit for bit.  packed: the default must have launched the packed instance
    for every stencil of the battery (at least seven launches) -- or, for a field that is not packed, for none; gauge_pack 0 for none."""
    battery = battery or _battery
    lat.set_option("gauge_pack", 0)
    n0 = lat.gauge_pack_launches()
    ref, it_ref = battery(lat, N, k, p, cg)
    assert lat.gauge_pack_launches() == n0
    lat.set_option("gauge_pack", -1)
    got, it = battery(lat, N, k, p, cg)
    n1 = lat.gauge_pack_launches()
    print("packed launches", n1 - n0, "iterations", it)
    assert (n1 - n0 >= 7) if packed else (n1 == n0)
    assert it == it_ref
    assert len(got) == len(ref)
    for n, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(a, b), "output %d differs: max |diff| %.3e" % (n, float(np.abs(a - b).max()))
    return ref


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def setup(request):
    shape = request.param
    g = _gauge(shape)
    lat = _lattice(shape, g)
    N = shape[0] * shape[1] * shape[2] * shape[3] // 2
    k, p = random_spinor(31, N), random_spinor(32, N)
    yield shape, g, lat, N, k, p
    lat.close()


def test_random_su3_field_is_packed_and_gives_the_same_bits(setup):
    shape, g, lat, N, k, p = setup
    _assert_same_with_and_without(lat, N, k, p)
    st = lat.gauge_pack_stats()
    print("stats", st, "build %.3f ms" % lat.gauge_pack_build_ms())
    assert st[0] == 1 and st[4] == 0
    assert sum(st[1:4]) == 16 * N               # every link slot of the stencil's copy: 8 directions, two parities


def _battery_dot_and_shifted(lat, N, k, p, cg=True):
    """The two reducing epilogues the plain battery does not reach: <p, A p> in the last stencil (cg_fused_dot 1) and the shifted
    residual update of the multi-shift CG."""
    dk, dl = lat.field(k), lat.field()
    out = []
    lat.set_option("cg_fused_dot", 1)
    try:
        iters, _ = lat.cg_her(dl, dk, 1000, 1e-20, 1, N)
    finally:
        lat.set_option("cg_fused_dot", 2)
    out.append(dl.download())
    it2, _, P = lat.cg_mms_tm(dk, [0.0, 0.05, 0.3], 1000, 1e-20, 1)
    for f in P:
        out.append(f.download()); f.free()
    for f in (dk, dl):
        f.free()
    return out, (iters, it2)


def test_dot_and_shifted_residual_epilogues(setup):
    shape, g, lat, N, k, p = setup
    _assert_same_with_and_without(lat, N, k, p, battery=_battery_dot_and_shifted)


@pytest.mark.parametrize("rot", [1, 2])
def test_forced_rotation(setup, rot):
    shape, g, lat, N, k, p = setup
    lat.set_option("gauge_pack_rot", rot)
    try:
        st = lat.gauge_pack_stats()
        print("rot", rot, "stats", st)
        assert st[0] == 1 and st[4] == 0
        assert st[1 + rot] >= 16 * N - 16       # (a link in 10^7 fails one given rotation: none expected among 10^5, a handful allowed)
        _assert_same_with_and_without(lat, N, k, p)
    finally:
        lat.set_option("gauge_pack_rot", -1)


def _planted_link(rng, row):
    """A generic SU(3) matrix whose element [row][0] is ~1e-9 plus 2^20 .. 2^30 ulps: W times the rotation of columns 0 and 1 that
    leaves that element at 1e-9, then the offset on its real part.  Unitary to 3e-15."""
    from tests.util import random_su3
    w = random_su3(rng, 1)[0]
    W = w[..., 0] + 1j * w[..., 1]
    w0, w1 = W[row, 0], W[row, 1]
    n = np.sqrt(abs(w0) ** 2 + abs(w1) ** 2)
    s = 1e-9 / n
    c = np.sqrt(1.0 - s * s)
    a = (c * w1 + s * np.conj(w0)) / n
    b = (-c * w0 + s * np.conj(w1)) / n
    V = np.eye(3, dtype=complex)
    V[0, 0], V[0, 1], V[1, 0], V[1, 1] = a, -np.conj(b), b, np.conj(a)
    U = W @ V
    out = np.empty((3, 3, 2))
    out[..., 0], out[..., 1] = U.real, U.imag
    e = out[row, 0, 0]
    assert 0.5e-9 < e < 2e-9
    out[row, 0, 0] = e + float(rng.integers(2 ** 20, 2 ** 30)) * np.spacing(e)
    return out


def test_field_that_needs_the_selector(setup):
    """200 links whose rebuild of one row cannot be exact (a tiny element: the fp32 residual is too coarse for it), a third for each
    row.  With the rotation that rebuilds a link's tiny row tried FIRST (gauge_pack_rot), at least half of the planted links must
    sit on another rotation; none is without one; the outputs are those of the full read."""
    shape, g, lat, N, k, p = setup
    rng = np.random.default_rng(101)
    V = 2 * N
    g2 = g.copy()
    where = rng.choice(V * 4, size=200, replace=False)
    rows = np.arange(200) % 3
    for w, row in zip(where, rows):
        u = _planted_link(rng, int(row))
        U = u[..., 0] + 1j * u[..., 1]
        assert np.abs(U @ U.conj().T - np.eye(3)).max() < 3e-15
        g2[w // 4, w % 4] = u
    lat.set_gauge(g2)
    try:
        for rot in (0, 1, 2):
            # rotation `rot` rebuilds row rot + 2 (mod 3); every link is in the stencil's copy twice (forward and backward hop)
            lat.set_option("gauge_pack_rot", rot)
            st = lat.gauge_pack_stats()
            n_row = 2 * int(np.sum(rows == (rot + 2) % 3))
            print("rot", rot, "stats", st, "slots planted on its row", n_row, "slots elsewhere", 16 * N - st[1 + rot])
            assert st[0] == 1 and st[4] == 0
            # of the slots planted on the row this rotation rebuilds, at least half sit elsewhere -- and nothing else does (an
            # unplanted link fails a given rotation once in 10^7: at most the 400 planted slots and a handful)
            assert n_row // 2 <= 16 * N - st[1 + rot] <= 400 + 4
        lat.set_option("gauge_pack_rot", -1)
        st = lat.gauge_pack_stats()
        print("default stats", st)
        assert st[0] == 1 and st[4] == 0
        _assert_same_with_and_without(lat, N, k, p)
    finally:
        lat.set_option("gauge_pack_rot", -1)
        lat.set_gauge(g)


def test_a_link_that_is_not_su3_is_reported_and_read_in_full(setup):
    from oracle.oraclebind import Oracle
    shape, g, lat, N, k, p = setup
    g2 = g.copy()
    g2[7, 2] *= 1.0 + 1e-6
    lat.set_gauge(g2)
    try:
        st = lat.gauge_pack_stats()
        print("stats", st)
        assert st[0] == 0 and st[4] == 2        # the link's forward and backward slot
        ref = _assert_same_with_and_without(lat, N, k, p, cg=False, packed=False)
        orc = Oracle(*shape, kappa=KAPPA, mu=MU, theta=THETA, threads=8)
        orc.set_gauge(g2)
        want = orc.new_field()
        for ieo in (0, 1):
            orc.Hopping_Matrix(ieo, want, k)
            assert rel_err(ref[3 * ieo], want[:N]) < TOL
    finally:
        lat.set_gauge(g)


def test_invalidation_by_set_gauge_and_update_gauge(setup):
    shape, g, lat, N, k, p = setup
    assert lat.gauge_pack_stats()[0] == 1                       # the packed copy of the fixture's links exists
    first = _assert_same_with_and_without(lat, N, k, p, cg=False)
    g2 = _gauge(shape, seed=8)
    lat.set_gauge(g2)
    try:
        second = _assert_same_with_and_without(lat, N, k, p, cg=False)
        assert not np.array_equal(first[0], second[0])
        mom = 0.3 * np.random.default_rng(5).standard_normal((2 * N, 4, 8))
        lat.momenta_upload(mom)
        lat.set_option("gauge_pack", -1)
        lat.update_gauge(0.05)
        third = _assert_same_with_and_without(lat, N, k, p, cg=False)
        assert not np.array_equal(second[0], third[0])
    finally:
        lat.set_gauge(g)


def test_gauge_recon_12_keeps_precedence(setup):
    shape, g, lat, N, k, p = setup
    full, _ = _battery(lat, N, k, p, cg=False)
    lat.set_option("gauge_recon", 12)
    try:
        ref = _assert_same_with_and_without(lat, N, k, p, cg=False, packed=False)
        # the 12-real read is what ran: it rounds differently from the full read, and stays within the tolerance of it
        assert any(not np.array_equal(a, b) for a, b in zip(ref, full))
        for a, b in zip(ref, full):
            assert rel_err(a, b) < TOL
    finally:
        lat.set_option("gauge_recon", 18)
