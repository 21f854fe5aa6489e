"""GPU: the rows that run on a T-split rank -- clover term and inverse, the clover force chain (sw_spinor_eo / sw_deriv / sw_all) with
deriv_Sb, the plaquette force and sums -- with the ranks as several contexts of one process, on slabs whose three spatial extents are
pairwise different, slab by slab against the CPU oracle (tests/gauge_restate.py for the gauge monomial) of the UNSPLIT lattice.

On a cubic slab an extent used as the wrong stride, a wrap test against the wrong extent, a `face` or `XYZ` built from the wrong
factors and a halo-slab offset are all invisible; a loopback rank is its own neighbour.  The split paths have geometry code of their
own (lex_index / SwEdgeLd::locate / sw_pack_slabs_kernel, the interior launches from i_begin = face, force_pack_kernel and the halo
branch of deriv_Sb_kernel, GaugeGeom::slab), and the launchers of the two plaquette-leaf kernels take forms no other test reaches:

* test_shapes_reach_the_forms (no GPU): sw_tile_order, the slab condition of sw_all_launch and the interior range restated, the
  form every shape below is for asserted, and every block order walked on the CPU: each site block exactly once per parity;
* (b) test_clover_term_on_ranks, (c) test_force_chain_on_ranks on all of SPLIT, (d) test_gauge_monomial_on_ranks on P and Q;
* (e) test_unsplit_block_orders: the tile order with two and four block rows per tile and the slab order with 12 blocks per
  time-slice, unsplit.

Bounds: tests.util.TOL, 4 * TOL behind sw_all (test_gpu_force.py); the sums as in test_gpu_gauge.py.  Every comparison is against
the CPU; only the bit-identity checks across block orders compare two device runs.  Inputs: tmlqcd_amd.synthetic seeds.
"""
import functools

import numpy as np
import pytest

from tests import gauge_restate as gr
from tests.util import TOL, rel_err

gpu = pytest.mark.gpu

KAPPA, MU, C_SW = 0.13, 0.02, 1.4
THETA = (1.0, 0.5, -0.25, 0.125)
GAUGE_SEED, SPINOR_SEED, MOM_SEED = 16, 20, 77
FAC_SW, FAC_SB = 0.7, (0.6, -0.3)                   # sw_spinor_eo; deriv_Sb with ieo = 1, then 0 with the roles swapped
SWALL_ORDERS, SWTERM_ORDERS = (0, 1, 2, 8), (0, 1)
# id: (local (T, LX, LY, LZ), ranks)
SPLIT = {
    "P": ((2, 2, 6, 4), 3),         # face 24; T = 2: no interior launch, both slices are t-faces; up and down neighbours differ
    "Q": ((4, 6, 2, 10), 2),        # face 60: waves straddle time-slices; LZ/2 odd; +-y coincide; interior 120 sites, plain order
    "R": ((4, 6, 8, 32), 2),        # face 768; interior in tile order from t0 = 1: nt 2, nby 2, nty 2, tx 2, 6 tiles on 8 XCDs
    "S": ((4, 8, 16, 12), 2),       # face 768 = 12 blocks, no tile order (LZ/2 = 6): slab order, 16 slots for 12 blocks
    "U": ((4, 2, 8, 64), 2),        # face 512; tile order with two z-rows per block: tyb 2, nby 4, nty 2
}
ORDERED = ("R", "S", "U")           # shapes whose interior launch depends on "swall_order"
TERM_ORDERED = ("R", "U")           # ... and on "swterm_order"
GAUGE = ("P", "Q")                  # (d)
UNSPLIT = {"tyb2": (2, 2, 8, 64), "tyb4": (2, 2, 4, 128), "slab12": (2, 8, 16, 12)}      # (e)


# ------------------------------------------------------------------ the launchers of clover.hip restated
def _tile_order(shape, ib, ie, txw=4):
    """sw_tile_order: the SwOrder of a launch over the e/o sites [ib, ie) and its grid, or None"""
    T, LX, LY, LZ = shape
    face, LZh = LX * LY * LZ // 2, LZ // 2
    rpb = 64 // LZh if LZh > 0 and 64 % LZh == 0 else 0
    if not (rpb > 0 and LY % rpb == 0 and ib % face == 0 and ie % face == 0 and face % 64 == 0):
        return None
    o = {"rpb": rpb, "nby": LY // rpb}
    o["tx"] = txw if LX % txw == 0 else (4 if LX % 4 == 0 else (2 if LX % 2 == 0 else 1))
    o["tyb"] = 1 if rpb >= 4 else (4 // rpb if 4 // rpb <= o["nby"] and o["nby"] % (4 // rpb) == 0 else 1)
    o["nty"] = o["nby"] // o["tyb"]
    o["ntiles"] = (LX // o["tx"]) * o["nty"]
    o["tb"] = o["tx"] * o["tyb"]
    o["t0"], o["nt"] = ib // face, (ie - ib) // face
    o["grid"] = 8 * ((o["ntiles"] + 7) // 8) * o["nt"] * o["tb"] * 2
    return o


def _interior(shape, split):
    """[ib, ie) of the launch over the sites whose plaquettes stay on the rank, and whether it is made at all"""
    T, LX, LY, LZ = shape
    Vh, face = T * LX * LY * LZ // 2, LX * LY * LZ // 2
    ib, ie = (face, Vh - face) if split else (0, Vh)
    return ib, ie, ie > ib and (not split or T > 2)


def _sw_all_form(shape, split, order=2):
    """sw_all_launch: the block order of the interior launch under "swall_order" `order`"""
    ib, ie, launched = _interior(shape, split)
    if not launched:
        return {"order": "none"}
    face = shape[1] * shape[2] * shape[3] // 2
    n = ie - ib
    f = {"order": "plain", "ib": ib, "n": n, "chunk": ((n + 63) // 64 + 7) // 8}
    f["grid"] = f["chunk"] * 16
    if order != 0 and face % 64 == 0 and face // 64 >= 8:
        f.update(order="slab", nbt=face // 64, slab=(face // 64 + 7) // 8)
        f["grid"] = 8 * f["slab"] * (n // face) * 2
    if order >= 2:
        t = _tile_order(shape, ib, ie, order if order >= 4 else 4)
        if t:
            f.update(t, order="tile")
    return f


def _sw_term_form(shape, split, order=1):
    ib, ie, launched = _interior(shape, split)
    if not launched:
        return {"order": "none"}
    n = ie - ib
    f = {"order": "plain", "ib": ib, "n": n, "chunk": ((n + 63) // 64 + 7) // 8}
    f["grid"] = f["chunk"] * 16
    if order:
        t = _tile_order(shape, ib, ie, 4)
        if t:
            f.update(t, order="tile")
    return f


def _walk(shape, f):
    """The (parity, site block) every thread block of a launch in form `f` takes (sw_tile_block, the slab and the plain order of
    sw_all_gather_kernel / sw_term_kernel), and the XCDs (blockIdx.x & 7) that take no block at all."""
    LX = shape[1]
    nblocks = (f["n"] + 63) // 64
    taken, busy = [], set()
    for b in range(f["grid"]):
        q, xcd = b >> 3, b & 7
        par, r = q & 1, q >> 1
        if f["order"] == "tile":
            bx, r = r % f["tb"], r // f["tb"]
            tt, tile = r % f["nt"], (r // f["nt"]) * 8 + xcd
            if tile >= f["ntiles"]:
                continue
            tile_x, tile_y = divmod(tile, f["nty"])
            bxx, bxy = divmod(bx, f["tyb"])
            sb = (tt * LX + tile_x * f["tx"] + bxx) * f["nby"] + tile_y * f["tyb"] + bxy
        elif f["order"] == "slab":
            tt = r // f["slab"]
            rr = xcd * f["slab"] + (r - tt * f["slab"])
            if rr >= f["nbt"]:
                continue
            sb = tt * f["nbt"] + rr
        else:
            sb = xcd * f["chunk"] + r
        if sb * 64 >= f["n"]:
            continue
        taken.append((par, sb))
        busy.add(xcd)
    return taken, nblocks, sorted(set(range(8)) - busy)


def test_shapes_reach_the_forms():
    """The premise of the cases below (a condition, not a measurement): what each shape makes the launchers of clover.hip do."""
    for shape in [s for s, _ in SPLIT.values()] + list(UNSPLIT.values()):
        assert len(set(shape[1:])) == 3 and all(x % 2 == 0 for x in shape), shape
    geo = {k: dict(face=s[1] * s[2] * s[3] // 2, Vh=int(np.prod(s)) // 2, world=w) for k, (s, w) in SPLIT.items()}
    allf = {k: _sw_all_form(s, True) for k, (s, _) in SPLIT.items()}
    term = {k: _sw_term_form(s, True) for k, (s, _) in SPLIT.items()}
    # P: nothing but t-faces, and a ring of three
    assert (geo["P"]["face"], geo["P"]["world"], SPLIT["P"][0][0]) == (24, 3, 2)
    assert _interior(SPLIT["P"][0], True) == (24, 24, False) and allf["P"]["order"] == term["P"]["order"] == "none"
    assert all((r + 1) % 3 != (r - 1) % 3 for r in range(geo["P"]["world"]))
    # Q: a face that is no multiple of the wave, odd LZ/2, LY = 2, a partial last block in plain order
    q = SPLIT["Q"][0]
    assert (geo["Q"]["face"], geo["Q"]["face"] % 64, (q[3] // 2) % 2, q[2]) == (60, 60, 1, 2)
    assert _interior(q, True) == (60, 180, True)
    for f in (allf["Q"], term["Q"]):
        assert (f["order"], f["n"], f["n"] % 64, f["chunk"], f["grid"]) == ("plain", 120, 56, 1, 16)
    # R: the interior in tile order from the second time-slice on, fewer tiles than XCDs
    for f in (allf["R"], term["R"]):
        assert geo["R"]["face"] == 768
        assert (f["order"], f["t0"], f["nt"], f["rpb"], f["nby"], f["tyb"], f["nty"], f["tx"], f["ntiles"]) == ("tile", 1, 2, 4, 2, 1, 2, 2, 6)
        assert _walk(SPLIT["R"][0], f)[2] == [6, 7]                                   # two XCDs take the exit
    # S: no tile order, slab order with four padding slots
    s = allf["S"]
    assert geo["S"]["face"] == 768 and SPLIT["S"][0][3] // 2 == 6 and 64 % 6 != 0
    assert (s["order"], s["slab"], s["nbt"], 8 * s["slab"] - s["nbt"], s["grid"]) == ("slab", 2, 12, 4, 64)
    assert term["S"]["order"] == "plain" and _sw_all_form(SPLIT["S"][0], True, 8)["order"] == "slab"
    # U: two z-rows per block, two block rows per tile
    for f in (allf["U"], term["U"]):
        assert geo["U"]["face"] == 512
        assert (f["order"], f["t0"], f["nt"], f["rpb"], f["tyb"], f["nby"], f["nty"], f["tx"], f["ntiles"]) == ("tile", 1, 2, 2, 2, 4, 2, 2, 2)
    # "swall_order" 0 / 1 on the ordered shapes: plain, slab (S: uneven; R: 12 per slice as well; U: exactly one per XCD)
    for k in ORDERED:
        assert _sw_all_form(SPLIT[k][0], True, 0)["order"] == "plain" and _sw_all_form(SPLIT[k][0], True, 1)["order"] == "slab"
        assert allf[k]["order"] != "plain" and allf[k]["order"] != "none"
    assert [k for k in SPLIT if term[k]["order"] == "tile"] == list(TERM_ORDERED)
    assert [k for k in SPLIT if allf[k]["order"] in ("tile", "slab")] == list(ORDERED)
    assert max(int(np.prod(s)) * w for s, w in SPLIT.values()) == 12288
    # (e) unsplit companions
    u2, u4, u12 = (_sw_all_form(UNSPLIT[k], False) for k in ("tyb2", "tyb4", "slab12"))
    assert (u2["order"], u2["rpb"], u2["tyb"], u2["nby"], u2["nty"], u2["t0"], u2["nt"]) == ("tile", 2, 2, 4, 2, 0, 2)
    assert (u4["order"], u4["rpb"], u4["tyb"], u4["nby"], u4["nty"], u4["ntiles"]) == ("tile", 1, 4, 4, 1, 1)
    assert (u12["order"], u12["slab"], u12["nbt"]) == ("slab", 2, 12)
    for k in ("tyb2", "tyb4"):
        t = _sw_term_form(UNSPLIT[k], False)
        assert (t["order"], t["tyb"]) == ("tile", _sw_all_form(UNSPLIT[k], False)["tyb"])
    # every order of every launch: each site block of each parity exactly once
    cases = [(s, True) for s, _ in SPLIT.values()] + [(s, False) for s in UNSPLIT.values()]
    for shape, split in cases:
        forms = [_sw_all_form(shape, split, o) for o in SWALL_ORDERS] + [_sw_term_form(shape, split, o) for o in SWTERM_ORDERS]
        for f in forms:
            if f["order"] == "none":
                continue
            taken, nblocks, _ = _walk(shape, f)
            assert sorted(taken) == [(p, b) for p in (0, 1) for b in range(nblocks)], (shape, split, f)


# ------------------------------------------------------------------ the unsplit oracle, once per lattice
@functools.lru_cache(maxsize=None)
def _reference(dims):
    """Clover blocks, insertion fields and force of the unsplit lattice `dims` on the CPU oracle (read-only arrays)."""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import synthetic as syn
    orc = Oracle(*dims, kappa=KAPPA, mu=MU, theta=THETA, threads=8)
    orc.set_gauge(syn.gauge_field(GAUGE_SEED, *dims))
    sw = orc.sw_term(KAPPA, C_SW)
    swi, fails = orc.sw_invert(sw, 0, MU)
    assert fails == 0
    orc.set_clover(sw, swi)
    N, V = orc.Vh, orc.V
    fo = []
    for i, par in enumerate((1, 1, 0, 0)):                    # fields 0, 1 on odd sites, 2, 3 on even sites
        b = orc.new_field(); b[:N] = syn.spinor_field_eo(SPINOR_SEED + i, par, *dims); fo.append(b)
    swm, swp = np.zeros((V, 4, 3, 3, 2)), np.zeros((V, 4, 3, 3, 2))
    orc.sw_spinor_eo(0, swm, swp, fo[2], fo[3], FAC_SW)
    orc.sw_spinor_eo(1, swm, swp, fo[0], fo[1], FAC_SW)
    orc.sw_deriv(0, swm, swp, MU)
    clover = np.zeros((orc.VPR, 4, 8))
    orc.sw_all(clover, swm, swp, KAPPA, C_SW)
    force = np.zeros((orc.VPR, 4, 8))
    orc.deriv_Sb(1, fo[0], fo[2], force, FAC_SB[0])
    orc.deriv_Sb(0, fo[2], fo[0], force, FAC_SB[1])
    orc.sw_all(force, swm, swp, KAPPA, C_SW)
    ref = dict(sw=sw, swi=swi, swm=swm, swp=swp, clover=clover[:V], force=force[:V])
    for a in ref.values():
        a.setflags(write=False)
    return ref


def _global(sid):
    (T, LX, LY, LZ), world = SPLIT[sid]
    return (T * world, LX, LY, LZ)


def _ranks(sid):
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    shape, world = SPLIT[sid]
    lats = [Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA, nproc_t=world, proc_t=r) for r in range(world)]
    for r, lat in enumerate(lats):
        lat.set_gauge(syn.gauge_field(GAUGE_SEED, *shape, world, r))
    return lats


def _clover_errs(lat, ref, r, world):
    """get_clover() of rank r against its slab of the unsplit sw / both sets of sw_inv"""
    sw, swi = lat.get_clover()
    V, Vh = lat.V, lat.Vh
    Vgh = world * Vh
    return sw, (rel_err(sw, ref["sw"][r * V:(r + 1) * V]), rel_err(swi[:Vh], ref["swi"][r * Vh:(r + 1) * Vh]),
                rel_err(swi[Vh:], ref["swi"][Vgh + r * Vh:Vgh + (r + 1) * Vh]))


# ------------------------------------------------------------------ (b)
@gpu
@pytest.mark.parametrize("sid", list(SPLIT))
def test_clover_term_on_ranks(sid):
    """sw_term from the resident links + halo slabs and sw_invert(EE, mu != 0) on every rank == the slab of the unsplit oracle; where
    the interior launch has a tile order, the plain order gives the same bits."""
    from tmlqcd_amd import synthetic as syn
    shape, world = SPLIT[sid]
    ref = _reference(_global(sid))
    assert MU != 0.0
    lats = _ranks(sid)
    worst = 0.0
    for r, lat in enumerate(lats):
        lat.sw_term(syn.gauge_field(GAUGE_SEED, *shape, world, r), KAPPA, C_SW)
        lat.sw_invert(0, MU)
        sw, errs = _clover_errs(lat, ref, r, world)
        print("split %s rank %d/%d: sw rel err %.3e, sw_inv(+mu) %.3e, sw_inv(-mu) %.3e" % ((sid, r, world) + errs))
        worst = max(worst, *errs)
        assert max(errs) < TOL, (sid, r, errs)
        if sid in TERM_ORDERED:
            lat.set_option("swterm_order", 0)
            lat.sw_term(None, KAPPA, C_SW)                   # the resident links, plain order
            plain = lat.get_clover(True, False)[0]
            assert np.array_equal(plain, sw), (sid, r)
            assert rel_err(plain, ref["sw"][r * lat.V:(r + 1) * lat.V]) < TOL
    print("split %s clover term: largest rel err %.3e" % (sid, worst))
    for lat in lats:
        lat.close()


# ------------------------------------------------------------------ (c)
@gpu
@pytest.mark.parametrize("sid", list(SPLIT))
def test_force_chain_on_ranks(sid):
    """test_gpu_force.py::test_clover_force_on_two_t_slabs with the shape from the table: the site-local insertion fields per rank, then
    deriv_Sb in both parity roles and sw_all into one derivative field == the slab of the unsplit oracle; every "swall_order" on its
    own gives the same bits."""
    from tmlqcd_amd import synthetic as syn
    from tmlqcd_amd.hip import multi_deriv_Sb, multi_sw_all
    shape, world = SPLIT[sid]
    ref = _reference(_global(sid))
    lats = _ranks(sid)
    fd = []
    worst_pm = 0.0
    for r, lat in enumerate(lats):
        lat.sw_term(None, KAPPA, C_SW); lat.sw_invert(0, MU)
        fr = [lat.field(syn.spinor_field_eo(SPINOR_SEED + i, par, *shape, world, r)) for i, par in enumerate((1, 1, 0, 0))]
        fd.append(fr)
        lat.swpm_zero()
        lat.sw_spinor_eo(0, fr[2], fr[3], FAC_SW)
        lat.sw_spinor_eo(1, fr[0], fr[1], FAC_SW)
        lat.sw_deriv(0, MU)
        gm, gp = lat.get_swpm()
        V = lat.V
        em, ep = rel_err(gm, ref["swm"][r * V:(r + 1) * V]), rel_err(gp, ref["swp"][r * V:(r + 1) * V])
        print("split %s rank %d/%d: swm rel err %.3e, swp %.3e" % (sid, r, world, em, ep))
        worst_pm = max(worst_pm, em, ep)
        assert em < TOL and ep < TOL, (sid, r, em, ep)
        lat.derivative_zero()
    multi_deriv_Sb(lats, 1, [f[0] for f in fd], [f[2] for f in fd], FAC_SB[0])
    multi_deriv_Sb(lats, 0, [f[2] for f in fd], [f[0] for f in fd], FAC_SB[1])
    multi_sw_all(lats, KAPPA, C_SW)
    V = lats[0].V
    worst = 0.0
    for r, lat in enumerate(lats):
        err = rel_err(lat.derivative(), ref["force"][r * V:(r + 1) * V])
        print("split %s rank %d/%d: deriv_Sb + sw_all rel err %.3e" % (sid, r, world, err))
        worst = max(worst, err)
        assert err < 4 * TOL, (sid, r, err)
    if sid in ORDERED:
        first = None
        for order in SWALL_ORDERS:
            for lat in lats:
                lat.set_option("swall_order", order)
                lat.derivative_zero()
            multi_sw_all(lats, KAPPA, C_SW)
            got = [lat.derivative() for lat in lats]
            for r, d in enumerate(got):
                err = rel_err(d, ref["clover"][r * V:(r + 1) * V])
                print("split %s rank %d/%d swall_order %d: sw_all rel err %.3e" % (sid, r, world, order, err))
                worst = max(worst, err)
                assert err < 4 * TOL, (sid, r, order, err)
            if first is None:
                first = got
            for r, d in enumerate(got):
                assert np.array_equal(d, first[r]), (sid, r, order)
    print("split %s force chain: largest rel err swm / swp %.3e, derivative %.3e" % (sid, worst_pm, worst))
    for lat in lats:
        lat.close()


# ------------------------------------------------------------------ (d)
@gpu
@pytest.mark.parametrize("sid", GAUGE)
def test_gauge_monomial_on_ranks(sid):
    """test_gpu_gauge.py::test_on_t_slabs with the shape from the table: after a multi_update_gauge the plaquette force slab by slab ==
    the unsplit restatement, the slab sums add up to the unsplit sums; rectangles reach two slices deep and stay refused."""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import synthetic as syn
    from tmlqcd_amd.hip import TmHipError, multi_update_gauge
    shape, world = SPLIT[sid]
    T = shape[0]
    dims = _global(sid)
    Vg = int(np.prod(dims))
    V = Vg // world
    orc = Oracle(*dims, kappa=KAPPA, mu=MU, threads=4)
    g = syn.gauge_field(GAUGE_SEED, *dims)
    mom = np.random.default_rng(MOM_SEED).standard_normal((Vg, 4, 8))
    lats = _ranks(sid)
    for r, lat in enumerate(lats):
        lat.momenta_upload(np.ascontiguousarray(mom[r * V:(r + 1) * V]))
    multi_update_gauge(lats, 0.05)
    orc.update_gauge(g, mom, 0.05)
    g = np.ascontiguousarray(g[:Vg])
    lam = 0.3
    tot_p, tot_a, worst = 0.0, 0.0, 0.0
    for r, lat in enumerate(lats):
        slab = (r * T, (r + 1) * T)
        lat.derivative_zero()
        lat.gauge_derivative(5.8, glambda=lam)
        err = rel_err(lat.derivative(), gr.gauge_derivative(g, dims, 5.8, glambda=lam, t_slab=slab))
        p, a = lat.measure_plaquette(), lat.measure_gauge_action(lam)
        dp, da = abs(p - gr.measure_plaquette(g, dims, t_slab=slab)), abs(a - gr.measure_gauge_action(g, dims, lam, t_slab=slab))
        print("split %s rank %d/%d: plaquette force rel err %.3e, plaquette sum |diff| %.3e (bound %.3e), action %.3e (bound %.3e)"
              % (sid, r, world, err, dp, TOL * 6 * V, da, TOL * 6 * V * (1 + lam)))
        worst = max(worst, err)
        assert err < TOL, (sid, r, err)
        assert dp <= TOL * 6 * V and da <= TOL * 6 * V * (1 + lam), (sid, r)
        tot_p += p
        tot_a += a
        with pytest.raises(TmHipError):
            lat.gauge_derivative(5.8, c0=1.0 + 8.0 * 0.331, c1=-0.331, use_rectangles=True)
        with pytest.raises(TmHipError):
            lat.measure_rectangles()
    assert abs(tot_p - gr.measure_plaquette(g, dims)) <= TOL * 6 * V * world
    assert abs(tot_a - gr.measure_gauge_action(g, dims, lam)) <= TOL * 6 * V * world * (1 + lam)
    print("split %s plaquette force: largest rel err %.3e" % (sid, worst))
    for lat in lats:
        lat.close()


# ------------------------------------------------------------------ (e)
@gpu
@pytest.mark.parametrize("uid", list(UNSPLIT))
def test_unsplit_block_orders(uid):
    """test_gpu_force.py::test_clover_force_and_clover_term_block_orders on the forms it does not reach: sw_term and sw_all in every
    block order, bit-identical to each other and within the bounds of the oracle."""
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    dims = UNSPLIT[uid]
    ref = _reference(dims)
    lat = Lattice(*dims, kappa=KAPPA, mu=MU, theta=THETA)
    g = syn.gauge_field(GAUGE_SEED, *dims)
    lat.set_gauge(g)
    got = []
    for order in SWTERM_ORDERS:
        lat.set_option("swterm_order", order)
        lat.sw_term(g, KAPPA, C_SW)
        got.append(lat.get_clover(True, False)[0])
        err = rel_err(got[-1], ref["sw"])
        print("unsplit %s swterm_order %d: sw rel err %.3e" % (uid, order, err))
        assert err < TOL, (uid, order, err)
    assert np.array_equal(got[0], got[1])
    lat.sw_invert(0, MU)
    swi = lat.get_clover(False, True)[1]
    assert rel_err(swi, ref["swi"]) < TOL
    fd = [lat.field(syn.spinor_field_eo(SPINOR_SEED + i, par, *dims)) for i, par in enumerate((1, 1, 0, 0))]
    lat.swpm_zero()
    lat.sw_spinor_eo(0, fd[2], fd[3], FAC_SW); lat.sw_spinor_eo(1, fd[0], fd[1], FAC_SW); lat.sw_deriv(0, MU)
    gm, gp = lat.get_swpm()
    assert rel_err(gm, ref["swm"]) < TOL and rel_err(gp, ref["swp"]) < TOL
    first = None
    for order in SWALL_ORDERS:
        lat.set_option("swall_order", order)
        lat.derivative_zero()
        lat.sw_all(KAPPA, C_SW)
        d = lat.derivative()
        err = rel_err(d, ref["clover"])
        print("unsplit %s swall_order %d: sw_all rel err %.3e" % (uid, order, err))
        assert err < 4 * TOL, (uid, order, err)
        if first is None:
            first = d
        assert np.array_equal(d, first), (uid, order)
    lat.close()
