"""GPU: update_gauge / update_momenta (md_update.hip) and the state they invalidate, on shapes where their blocks are partial.

links_kernel<true> owns 64 lexicographic sites (256 links) per block, update_momenta_kernel 32 e/o indices per parity; the
shapes below leave both partial, put an odd number of site pairs on a z-row, and make the forward and backward neighbour
coincide (extent 2).  test_shapes_reach_the_forms states which shape reaches what.

* (a) test_update_chain: three steps against the CPU oracle (pinned bit for bit to the reference's update_gauge), links and
  the stencil after each; the scatter of the UPDATE form == the plain re-sort of the same links, bit for bit;
* (b) test_large_arguments: |step P| up to 7, where terms 12-15 of the Cayley-Hamilton recursion carry weight, oracle only;
* (c) test_against_the_true_exponential: exp(step P) U in long double (tests/md_restate.py), device at most 8 x the oracle's own
  distance -- the two differ by FMA contraction and the rounding of 1/sqrt over about a hundred flops per entry;
* (d) test_update_momenta: P -= step dS with dS from deriv_Sb + the Iwasaki gauge force, and the refusals;
* (e) test_fp32_links_follow / test_clover_flags_follow / test_sw_term_with_host_links: what is derived from the links;
* (f) test_recon12_guard_*: no stencil reads 12 reals of links that left SU(3) by more than the guard's 1e-13;
* (g) test_t_slabs: T-split ranks as contexts of one process, halo_backward_kernel off the cubic case; test_recon12_guard_on_t_slabs:
  the guard behind tmhip_multi_update_gauge.
"""
import numpy as np
import pytest

from tests import md_restate as md
from tests import ndsw_restate as sw
from tests.util import TOL, random_gauge, random_spinor, rel_err

gpu = pytest.mark.gpu

TOL32 = 2e-6                                      # tests/test_gpu_mixed.py
KAPPA, MU, THETA = 0.131, 0.02, (1.0, 0.5, -0.25, 0.125)
C_SW = 1.57
C1 = -0.331
IWASAKI = dict(c0=1.0 - 8.0 * C1, c1=C1, use_rectangles=True)
MUBAR, EPSBAR, INVMAXEV = sw.FIXTURE
SHAPES = [(2, 2, 2, 2), (2, 2, 2, 6), (4, 2, 6, 2), (6, 2, 2, 6), (2, 6, 10, 2), (8, 6, 4, 12)]
LARGE = [(2, 2, 2, 6), (6, 2, 2, 6)]              # (b), (c)
FOLLOW = [(4, 2, 6, 2), (8, 6, 4, 12)]            # (e)
GUARD = [(2, 2, 2, 6), (8, 6, 4, 12)]             # (f)
SLABS = [((2, 2, 6, 2), 3), ((4, 6, 2, 4), 2)]    # (g): local shape, ranks
# (f): the 12-real read exists in the 256-thread stencil kernels only (launch_variant, hopping_impl.inc), and the automatic block size
# is 64 below 131072 sites per parity (tmhip_hop_block): with "block" 0 these shapes keep the full read whatever the option says, with
# "block" 256 the option decides what is read.  Both are run; only the second can see a guard that has lapsed.
BLOCKS, BLOCK_IDS = (0, 256), ("auto", "b256")
RECON12_SLAB = ((2, 4, 8, 4), 2)
GAUGE_SEED, MOM_SEED = 3, 4
# (c) asks for max |step P| <= 0.55 at step 0.1.  Seed 4 gives max |P| = 5.02 on the 192 links of (2, 2, 2, 6) and 5.55 on the 576 of
# (6, 2, 2, 6); seed 10 gives 5.22 there (chosen on the momenta alone: the first seed after 4 with 5 < max |P| <= 5.5).
TRUE_EXP_MOM_SEED = {(2, 2, 2, 6): 4, (6, 2, 2, 6): 10}
ids = lambda shapes: ["x".join(map(str, s)) for s in shapes]


def test_shapes_reach_the_forms():
    """The premise of the cases below (a condition, not a measurement): which blocks of the two kernels each shape leaves partial."""
    f = {}
    for s in SHAPES:
        V = int(np.prod(s))
        f[s] = dict(V=V, Vh=V // 2, full=V // 64, rest=V % 64, mrest=(V // 2) % 32, LZ=s[3])
    a = f[(2, 2, 2, 2)]
    assert (a["V"], a["full"], a["rest"], a["Vh"]) == (16, 0, 16, 8) and set(SHAPES[0]) == {2}  # one partial block of both kernels
    b = f[(2, 2, 2, 6)]
    assert (b["V"], b["full"], b["rest"], b["mrest"]) == (48, 0, 48, 24) and (b["LZ"] // 2) % 2 == 1         # LZ/2 odd
    c = f[(4, 2, 6, 2)]
    assert (c["V"], c["full"], c["rest"], c["mrest"], c["LZ"]) == (96, 1, 32, 16, 2)                         # a site pair is a whole z-row
    d = f[(6, 2, 2, 6)]
    assert (d["V"], d["full"], d["rest"], d["Vh"], d["mrest"]) == (144, 2, 16, 72, 8)
    e = f[(2, 6, 10, 2)]
    assert (e["V"], e["full"], e["rest"], e["mrest"]) == (240, 3, 48, 24)
    w = f[(8, 6, 4, 12)]
    assert (w["V"], w["full"], w["rest"], w["mrest"]) == (2304, 36, 0, 0)                                    # whole blocks only
    assert sum(1 for v in f.values() if v["rest"]) == 5 and sum(1 for v in f.values() if v["mrest"]) == 5
    assert sum(1 for s in SHAPES if 2 in s) == 5 and all(all(x % 2 == 0 for x in s) for s in SHAPES)
    assert all(f[s]["Vh"] < 131072 for s in GUARD) and 256 in BLOCKS and 0 in BLOCKS        # automatic block 64: no 12-real kernel without "block" 256
    for group in (LARGE, FOLLOW, GUARD):
        assert set(group) <= set(SHAPES)
        assert any(f[s]["rest"] for s in group)                                                           # each group keeps a partial block
    # (g): the t = 0 slice of a slab is one partial block of halo_backward_kernel, not cubic, and the slabs start on an even t
    for (T, LX, LY, LZ), world in SLABS:
        assert 0 < LX * LY * LZ < 256 and len({LX, LY, LZ}) > 1 and T % 2 == 0 and world >= 2
    assert (2 * 2 * 6 * 2) % 64 == 48 and (4 * 6 * 2 * 4) % 64 == 0


def _momenta(V, scale=1.0, seed=MOM_SEED):
    return scale * np.random.default_rng(seed).standard_normal((V, 4, 8))


def _pair(shape, mom_scale=1.0, upload=True, mom_seed=MOM_SEED):
    """Oracle and device lattice of one shape on the same SU(3) links; the momenta on the device."""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    orc = Oracle(*shape, kappa=KAPPA, mu=MU, theta=THETA, threads=8)
    lat = Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA)
    g = random_gauge(GAUGE_SEED, orc.VPR)
    mom = _momenta(orc.V, mom_scale, mom_seed)
    orc.set_gauge(g)
    lat.set_gauge(g)
    if upload:
        lat.momenta_upload(mom)
    return orc, lat, g, mom


def _stencil(orc, lat, links, k, dk, dl, what, tol=TOL):
    """Hopping_Matrix of both parities on the device == the oracle on `links`"""
    orc.set_gauge(links)
    ref = orc.new_field()
    for ieo in (0, 1):
        orc.Hopping_Matrix(ieo, ref, k)
        lat.Hopping_Matrix(ieo, dl, dk)
        err = rel_err(dl.download(), ref[:orc.Vh])
        print("%s Hopping_Matrix(%d) rel err %.3e" % (what, ieo, err))
        assert err < tol, (what, ieo, err)


# ------------------------------------------------------------------ (a)
@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_update_chain(shape):
    from tmlqcd_amd import Lattice
    orc, lat, g, mom = _pair(shape)
    N = orc.Vh
    k = random_spinor(5, N)
    dk, dl = lat.field(k), lat.field()
    og = g.copy()
    for step in (0.05, -0.02, 0.03):
        lat.update_gauge(step)
        orc.update_gauge(og, mom, step)
        err = rel_err(lat.gauge_download(), og)
        print("%s step %+.2f links rel err %.3e" % (shape, step, err))
        assert err < TOL, (shape, step, err)
        _stencil(orc, lat, og, k, dk, dl, "%s step %+.2f" % (shape, step))
    # the UPDATE scatter wrote, into both slots of every link, exactly what the plain re-sort of the same links writes
    down = lat.gauge_download()
    twin = Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA)
    twin.set_gauge(down)
    tk, tl = twin.field(k), twin.field()
    for ieo in (0, 1):
        lat.Hopping_Matrix(ieo, dl, dk)
        twin.Hopping_Matrix(ieo, tl, tk)
        assert np.array_equal(dl.download(), tl.download()), (shape, ieo)
    assert np.array_equal(lat.momenta_download(), mom)
    assert np.array_equal(dk.download(), k)
    twin.close()
    lat.close()


# ------------------------------------------------------------------ (b)
@gpu
@pytest.mark.parametrize("shape", LARGE, ids=ids(LARGE))
def test_large_arguments(shape):
    """momenta x 3, steps (0.2, -0.2, 0.5): the polynomial is the reference's and far from unitary here, so the oracle alone is the
    measure.  Premise: |step P| exceeds 3 on some link at every step, where term 15 of the series (x^15 / 15!) is above 1e-7."""
    orc, lat, g, mom = _pair(shape, 3.0)
    steps = (0.2, -0.2, 0.5)
    pmax = md.adj_norm(mom).max()
    assert min(abs(s) for s in steps) * pmax > 3.0 and max(abs(s) for s in steps) * pmax > 6.0, pmax
    assert 3.0 ** 15 / 1307674368000.0 > 1e-7
    og = g.copy()
    for step in steps:
        lat.update_gauge(step)
        orc.update_gauge(og, mom, step)
        err = rel_err(lat.gauge_download(), og)
        print("%s step %+.1f max |step P| %.2f links rel err %.3e" % (shape, step, abs(step) * pmax, err))
        assert err < TOL, (shape, step, err)
    lat.close()


# ------------------------------------------------------------------ (c)
@gpu
@pytest.mark.parametrize("shape", LARGE, ids=ids(LARGE))
def test_against_the_true_exponential(shape):
    """One step of 0.1 on standard-normal momenta against exp(step P) U in long double.  Measured on an MI355X:
    (2, 2, 2, 6): oracle 3.51e-16, device 3.83e-16;  (6, 2, 2, 6): oracle 5.46e-16, device 4.77e-16  (the MD update)."""
    orc, lat, g, mom = _pair(shape, mom_seed=TRUE_EXP_MOM_SEED[shape])
    step = 0.1
    assert 0.5 < step * md.adj_norm(mom).max() <= 0.55
    true = md.update_gauge_ld(g, mom, step)
    og = g.copy()
    orc.update_gauge(og, mom, step)
    d_orc = float(np.abs(md.cld(og) - true).max())
    assert d_orc < 2e-15, d_orc
    lat.update_gauge(step)
    d_dev = float(np.abs(md.cld(lat.gauge_download()) - true).max())
    print("%s distance to exp(step P) U in long double: oracle %.3e device %.3e" % (shape, d_orc, d_dev))
    assert d_dev <= 8 * d_orc, (shape, d_orc, d_dev)
    lat.close()


# ------------------------------------------------------------------ (d)
def _refusals(shape, g, mom):
    """update_momenta without momenta / without a derivative field, update_gauge without links / without momenta: refused, and
    what is on the device stays as it was"""
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    lat = Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA)
    with pytest.raises(TmHipError):
        lat.update_gauge(0.05)                          # no resident links (and no momenta)
    lat.momenta_upload(mom)
    with pytest.raises(TmHipError):
        lat.update_gauge(0.05)                          # momenta, still no links
    with pytest.raises(TmHipError):
        lat.update_momenta(0.05)                        # no derivative field
    assert np.array_equal(lat.momenta_download(), mom)
    with pytest.raises(TmHipError):
        lat.gauge_download()
    lat.close()
    lat = Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA)
    lat.set_gauge(g)
    lat.derivative_zero()
    with pytest.raises(TmHipError):
        lat.update_momenta(0.05)                        # no momenta uploaded
    with pytest.raises(TmHipError):
        lat.update_gauge(0.05)
    with pytest.raises(TmHipError):
        lat.momenta_download()
    assert np.array_equal(lat.gauge_download(), g) and not lat.derivative().any()
    lat.close()


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_update_momenta(shape):
    orc, lat, g, mom = _pair(shape)
    N = orc.Vh
    dl, dk = lat.field(random_spinor(6, N)), lat.field(random_spinor(7, N))
    lat.derivative_zero()
    lat.deriv_Sb(0, dl, dk, 0.7)
    lat.deriv_Sb(1, dl, dk, -1.3)
    lat.gauge_derivative(5.8, **IWASAKI)
    df = lat.derivative()
    assert np.abs(df).max() > 0.1 and np.abs(df).min() > 0.0
    want = mom
    for step in (0.05, -0.11):
        lat.update_momenta(step)
        want = md.update_momenta(want, df, step)
        err = rel_err(lat.momenta_download(), want)
        print("%s update_momenta(%+.2f) rel err %.3e" % (shape, step, err))
        assert err < TOL, (shape, step, err)
        assert np.array_equal(lat.derivative(), df)
    assert np.array_equal(lat.gauge_download(), g)
    lat.close()
    _refusals(shape, g, mom)


# ------------------------------------------------------------------ (e)
@gpu
@pytest.mark.parametrize("shape", FOLLOW, ids=ids(FOLLOW))
def test_fp32_links_follow(shape):
    """The fp32 copy of the links is rebuilt lazily at the next fp32 stencil (gauge32_set): a stale copy gives the old output, which
    is more than 100 x TOL32 away from the new one."""
    orc, lat, g, mom = _pair(shape)
    N = orc.Vh
    k32 = random_spinor(8, N).astype(np.float32)
    dk, dl = lat.field32(k32), lat.field32()
    old = []
    for ieo in (0, 1):
        lat.Hopping_Matrix_32(ieo, dl, dk)
        old.append(dl.download().astype(np.float64))
    lat.update_gauge(0.1)
    og = g.copy()
    orc.update_gauge(og, mom, 0.1)
    orc.set_gauge(og)
    ref = orc.new_field()
    for ieo in (0, 1):
        lat.Hopping_Matrix_32(ieo, dl, dk)
        new = dl.download().astype(np.float64)
        orc.Hopping_Matrix(ieo, ref, k32.astype(np.float64))
        err, moved = rel_err(new, ref[:N]), rel_err(old[ieo], new)
        print("%s Hopping_Matrix_32(%d) rel err %.3e, old - new %.3e" % (shape, ieo, err, moved))
        assert err < TOL32, (shape, ieo, err)
        assert moved > 100 * TOL32, (shape, ieo, moved)
    lat.close()


@gpu
@pytest.mark.parametrize("shape", FOLLOW, ids=ids(FOLLOW))
def test_clover_flags_follow(shape):
    """update_gauge drops sw_set, clover_set, clover_nd_set and clover32_set: every clover operator is refused with its outputs
    untouched until sw_term (from the resident links) and the inversions have run again, and then works on the new links."""
    from tmlqcd_amd.hip import TmHipError
    orc, lat, g, mom = _pair(shape)
    N = orc.Vh
    shift = MUBAR * MUBAR - EPSBAR * EPSBAR
    lat.set_nd(MUBAR, EPSBAR, INVMAXEV)

    def clover_state():
        lat.sw_invert(0, MU)
        lat.sw_invert_nd(shift)
        assert lat.sw_invert_failures() == 0

    lat.sw_term(g, KAPPA, C_SW)
    clover_state()
    ks, kc = random_spinor(9, N), random_spinor(10, N)
    mark, mark2 = random_spinor(11, N), random_spinor(12, N)
    dks, dkc, dls, dlc = lat.field(ks), lat.field(kc), lat.field(mark), lat.field(mark2)
    dk32, dl32 = lat.field32(ks.astype(np.float32)), lat.field32(mark.astype(np.float32))
    lat.Qsw_pm_psi_32(dl32, dk32)                       # the fp32 clover copy exists (clover32_set) ...
    dl32.upload(mark.astype(np.float32))                # ... and the output holds the mark again
    lat.derivative_zero()
    lat.deriv_Sb(1, dks, dkc, 0.8)
    before = lat.derivative()
    assert np.abs(before).max() > 0.1

    lat.update_gauge(0.1)
    og = g.copy()
    orc.update_gauge(og, mom, 0.1)
    assert rel_err(lat.gauge_download(), og) < TOL

    calls = {
        "Qsw_pm_psi": lambda: lat.op("Qsw_pm_psi", dls, dks),
        "Qsw_pm_psi_32": lambda: lat.Qsw_pm_psi_32(dl32, dk32),
        "Qsw_pm_ndpsi": lambda: lat.Qsw_pm_ndpsi(dls, dlc, dks, dkc),
        "ndcloverrat_force": lambda: lat.ndcloverrat_force([(dks, dkc)], [0.1], [0.5], INVMAXEV, KAPPA, C_SW, 1),
        "sw_invert": lambda: lat.sw_invert(0, MU),
        "sw_invert_nd": lambda: lat.sw_invert_nd(shift),
    }
    for name, call in calls.items():
        with pytest.raises(TmHipError):
            call()
        assert np.array_equal(dls.download(), mark) and np.array_equal(dlc.download(), mark2), name
        assert np.array_equal(dl32.download(), mark.astype(np.float32)), name
        assert np.array_equal(lat.derivative(), before), name

    lat.sw_term(None, KAPPA, C_SW)
    clover_state()
    orc.set_gauge(og)
    osw = orc.sw_term(KAPPA, C_SW)
    oswi, fails = orc.sw_invert(osw, 0, MU)
    assert fails == 0
    orc.set_clover(osw, oswi)
    ref = orc.new_field()
    orc.op("Qsw_pm_psi", ref, ks.copy())
    lat.op("Qsw_pm_psi", dls, dks)
    err = rel_err(dls.download(), ref[:N])
    print("%s Qsw_pm_psi on the new links rel err %.3e" % (shape, err))
    assert err < TOL, err
    cl = sw.clover_of(orc, KAPPA, C_SW)
    assert cl.cond(shift) < sw.COND_MAX
    cl.sw_invert_nd(shift)
    assert cl.fails == 0
    H = sw.hop_over(orc.Hopping_Matrix, N)
    ws, wc = sw.Qsw_pm_ndpsi(cl, H, sw.cplx(ks), sw.cplx(kc), MUBAR, EPSBAR, INVMAXEV)
    lat.Qsw_pm_ndpsi(dls, dlc, dks, dkc)
    es, ec = rel_err(dls.download(), sw.real(ws)), rel_err(dlc.download(), sw.real(wc))
    print("%s Qsw_pm_ndpsi on the new links rel err %.3e %.3e" % (shape, es, ec))
    assert es < TOL and ec < TOL, (es, ec)
    lat.close()


@gpu
@pytest.mark.parametrize("shape", FOLLOW, ids=ids(FOLLOW))
def test_sw_term_with_host_links(shape):
    """sw_term(g2) replaces the resident links: the stencil copy is re-sorted from them (gauge_copy_current) before the next stencil"""
    orc, lat, g, mom = _pair(shape)
    N = orc.Vh
    g2 = random_gauge(GAUGE_SEED + 10, orc.VPR)
    assert rel_err(g2, g) > 0.1
    k = random_spinor(13, N)
    dk, dl = lat.field(k), lat.field()
    lat.Hopping_Matrix(0, dl, dk)                       # the stencil has run on the old links
    lat.sw_term(g2, KAPPA, C_SW)
    assert np.array_equal(lat.gauge_download(), g2)
    _stencil(orc, lat, g2, k, dk, dl, "%s after sw_term(g2)" % (shape,))
    got, _ = lat.get_clover(True, False)
    err = rel_err(got, orc.sw_term(KAPPA, C_SW))
    print("%s sw_term(g2) rel err %.3e" % (shape, err))
    assert err < TOL, err
    lat.close()


# ------------------------------------------------------------------ (f)
def _recon12_checks(orc, lat, links, what):
    """every stencil form the 12-real read has, fp64 and fp32, against the oracle on `links`"""
    N = orc.Vh
    k = random_spinor(14, N)
    dk, dl = lat.field(k), lat.field()
    _stencil(orc, lat, links, k, dk, dl, what)
    ref = orc.new_field()
    c = -0.37 + 0.91j
    for ieo in (0, 1):
        orc.tm_times_Hopping_Matrix(ieo, ref, k, c)
        lat.tm_times_Hopping_Matrix(ieo, dl, dk, c)
        err = rel_err(dl.download(), ref[:N])
        print("%s tm_times_Hopping_Matrix(%d) rel err %.3e" % (what, ieo, err))
        assert err < TOL, (what, ieo, err)
    orc.op("Qtm_pm_psi", ref, k.copy())
    lat.Qtm_pm_psi(dl, dk)
    err = rel_err(dl.download(), ref[:N])
    print("%s Qtm_pm_psi rel err %.3e" % (what, err))
    assert err < TOL, (what, err)
    k32 = k.astype(np.float32)
    dk32, dl32 = lat.field32(k32), lat.field32()
    for ieo in (0, 1):
        orc.Hopping_Matrix(ieo, ref, k32.astype(np.float64))
        lat.Hopping_Matrix_32(ieo, dl32, dk32)
        err = rel_err(dl32.download().astype(np.float64), ref[:N])
        print("%s Hopping_Matrix_32(%d) rel err %.3e" % (what, ieo, err))
        assert err < TOL32, (what, ieo, err)


@gpu
@pytest.mark.parametrize("block", BLOCKS, ids=BLOCK_IDS)
@pytest.mark.parametrize("shape", GUARD, ids=ids(GUARD))
def test_recon12_guard_after_update_gauge(shape, block):
    """restoresu3 normalises rows 0 and 1 of exp(step P) without orthogonalising them, so after two steps of 0.5 on standard-normal
    momenta row 2 is no longer conj(row0 x row1) of the stored rows: the 12-real read must have been given up by then.  (Before
    links_changed re-evaluated the guard, the "block" 256 cases gave Hopping_Matrix(0) rel err 9.8e-9 and 6.1e-8 here.)"""
    orc, lat, g, mom = _pair(shape)
    assert lat.gauge_su3_deviation() < 1e-13
    lat.set_option("block", block)
    lat.set_option("gauge_recon", 12)
    lat.update_gauge(0.5)
    lat.update_gauge(0.5)
    down = lat.gauge_download()
    dev_host = md.row2_deviation(down)
    print("%s row2 deviation after two steps of 0.5: %.3e" % (shape, dev_host))
    assert dev_host > 1e-9
    _recon12_checks(orc, lat, down, "%s two steps of 0.5" % (shape,))
    dev = lat.gauge_su3_deviation()
    print("%s gauge_su3_deviation %.3e" % (shape, dev))
    assert dev > 1e-9
    _recon12_checks(orc, lat, down, "%s after the measurement" % (shape,))
    lat.close()


@gpu
@pytest.mark.parametrize("block", BLOCKS, ids=BLOCK_IDS)
@pytest.mark.parametrize("shape", GUARD, ids=ids(GUARD))
def test_recon12_guard_after_sw_term_with_host_links(shape, block):
    """sw_term(g_bad) replaces the resident links by ones with a link scaled by 1 + 1e-6 (the construction of
    tests/test_gpu_hopping.py::test_gauge_recon_12_is_exact_for_su3_links_and_refused_otherwise)"""
    orc, lat, g, mom = _pair(shape, upload=False)
    lat.set_option("block", block)
    lat.set_option("gauge_recon", 12)
    bad = g.copy()
    bad[7, 2] *= 1.0 + 1e-6
    assert md.row2_deviation(bad) > 1e-7
    lat.sw_term(bad, KAPPA, C_SW)
    assert np.array_equal(lat.gauge_download(), bad)
    _recon12_checks(orc, lat, bad, "%s sw_term(g_bad)" % (shape,))
    assert lat.gauge_su3_deviation() > 1e-7
    lat.close()


@gpu
@pytest.mark.parametrize("block", BLOCKS, ids=BLOCK_IDS)
@pytest.mark.parametrize("shape", GUARD, ids=ids(GUARD))
def test_recon12_stays_exact_after_a_small_step(shape, block):
    """The control: one step of 0.05 leaves the links SU(3) to rounding, and the stencil under gauge_recon 12 matches the oracle"""
    orc, lat, g, mom = _pair(shape)
    lat.set_option("block", block)
    lat.set_option("gauge_recon", 12)
    lat.update_gauge(0.05)
    down = lat.gauge_download()
    assert md.row2_deviation(down) < 1e-13
    _recon12_checks(orc, lat, down, "%s one step of 0.05" % (shape,))
    dev = lat.gauge_su3_deviation()
    print("%s gauge_su3_deviation after one step of 0.05: %.3e" % (shape, dev))
    assert dev < 1e-13
    lat.close()


# ------------------------------------------------------------------ (g)
def _slabs(local, world, steps, recon12=False):
    """multi_update_gauge by `steps` on `world` T-split ranks held by contexts of one process: links per slab, both halo slabs and
    multi_Hopping_Matrix of both parities == the unsplit oracle.  recon12: with "block" 256 and "gauge_recon" 12 accepted first."""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import multi_Hopping_Matrix, multi_update_gauge
    T, LX, LY, LZ = local
    Tg, XYZ = T * world, LX * LY * LZ
    V = T * XYZ
    Vh = V // 2
    orc = Oracle(Tg, LX, LY, LZ, kappa=KAPPA, mu=MU, theta=THETA, threads=8)
    g = random_gauge(GAUGE_SEED, orc.V)
    mom = _momenta(orc.V)

    def slab(r):
        return g[r * V:(r + 1) * V]

    lats = [Lattice(T, LX, LY, LZ, kappa=KAPPA, mu=MU, theta=THETA, nproc_t=world, proc_t=r) for r in range(world)]
    for r, lat in enumerate(lats):
        up, dn = (r + 1) % world, (r - 1) % world
        lat.set_gauge(np.ascontiguousarray(np.concatenate([slab(r), slab(up)[:XYZ], slab(dn)[V - XYZ:]])))
        lat.momenta_upload(np.ascontiguousarray(mom[r * V:(r + 1) * V]))
        if recon12:
            assert lat.gauge_su3_deviation() < 1e-13
            lat.set_option("block", 256)
            lat.set_option("gauge_recon", 12)
    for step in steps:
        multi_update_gauge(lats, step)
        orc.update_gauge(g, mom, step)
    orc.set_gauge(g)
    down = [lat.gauge_download() for lat in lats]
    for r in range(world):
        up, dn = (r + 1) % world, (r - 1) % world
        got = down[r]
        errs = (rel_err(got[:V], slab(r)), rel_err(got[V:V + XYZ], slab(up)[:XYZ]), rel_err(got[V + XYZ:], slab(dn)[V - XYZ:]))
        print("%s x %d rank %d: links %.3e, t = T slab %.3e, t = -1 slab %.3e" % ((local, world, r) + errs))
        assert max(errs) < TOL, (r, errs)
        assert np.array_equal(got[V:V + XYZ], down[up][:XYZ]) and np.array_equal(got[V + XYZ:], down[dn][V - XYZ:V]), r
    kin = [random_spinor(15, orc.Vh), random_spinor(16, orc.Vh)]
    ref = orc.new_field()
    ls = [lat.field() for lat in lats]
    for ieo in (0, 1):
        orc.Hopping_Matrix(ieo, ref, kin[ieo])
        ks = [lat.field(np.ascontiguousarray(kin[ieo][r * Vh:(r + 1) * Vh])) for r, lat in enumerate(lats)]
        multi_Hopping_Matrix(lats, ieo, ls, ks)
        for r in range(world):
            err = rel_err(ls[r].download(), ref[r * Vh:(r + 1) * Vh])
            print("%s x %d rank %d: multi_Hopping_Matrix(%d) rel err %.3e" % (local, world, r, ieo, err))
            assert err < TOL, (r, ieo, err)
    devs = [lat.gauge_su3_deviation() for lat in lats]
    for lat in lats:
        lat.close()
    return down, devs


@gpu
@pytest.mark.parametrize("local,world", SLABS, ids=["%s_x%d" % ("x".join(map(str, s)), w) for s, w in SLABS])
def test_t_slabs(local, world):
    down, devs = _slabs(local, world, (0.05, -0.02))
    assert max(md.row2_deviation(d) for d in down) < 1e-13 and max(devs) < 1e-13


@gpu
def test_recon12_guard_on_t_slabs():
    """tmhip_multi_update_gauge under "gauge_recon" 12.  A T-split rank runs the 256-thread kernels, and its stencil takes the 12-real
    instance once a time-slice is whole waves (face % 64 == 0): RECON12_SLAB is the smallest non-cubic local shape of that kind."""
    (T, LX, LY, LZ), world = RECON12_SLAB
    assert (LX * LY * LZ // 2) % 64 == 0 and len({LX, LY, LZ}) > 1
    down, devs = _slabs((T, LX, LY, LZ), world, (0.5, 0.5), recon12=True)
    assert min(md.row2_deviation(d) for d in down) > 1e-9 and min(devs) > 1e-9
