"""GPU: the doublet solvers on the clover operator (tmhip_cg_her_nd_op / tmhip_cg_mms_tm_nd_op, op = TMHIP_ND_OP_QSW_PM) against
the restated solvers (oracle/nd_restate.py) on the restated operator (tests/ndsw_restate.py) and against the reference's own
iteration counts (tests/golden/ref_ndsw_scalars_*.json), on 4^4 and one ragged shape.

1, 5 and 32 shifts, rel_prec 0 / 1 / -1, a run to max_iter; iteration counts within +-1 (what the twisted-mass doublet tests
allow); true residuals recomputed with the restatement; two solves bit-identical; the same results for every polling interval;
op = TMHIP_ND_OP_QTM_PM gives the bits of the un-suffixed calls.
"""
import json
import os

import numpy as np
import pytest

from oracle import nd_restate as nd
from tests import ndsw_restate as sw
from tests.test_gpu_ndsw_shapes import _Setup, _pair_err

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOLVE = [(4, 4, 4, 4), (6, 10, 2, 4)]
SOLVE_IDS = ["4x4x4x4", "6x10x2x4"]
FIVE = [0.02, 0.15, 0.6, 2.5, 9.0]
# name: (shifts, max_iter, eps_sq, rel_prec)
MMS = {
    "one_shift": ([0.1], 1000, 1e-20, 1),
    "five_sorted": (FIVE, 1000, 1e-22, 0),
    "thirty_two": (list(np.logspace(-2, 1, 32)), 25, 1e-22, 0),
    "rel_prec_negative": ([0.05, 0.5], 40, 1e-2, -1),     # with rel_prec 0 the restated run stops after 17 / 18 iterations
    "max_iter": ([0.02, 0.15, 0.6], 12, 1e-22, 0),
}
# name: (start, max_iter, eps_sq, rel_prec); start: a random start vector instead of zero
HER = {
    "zero_start_rel1": (False, 1000, 1e-20, 1),
    "zero_start_rel0": (False, 1000, 1e-16, 0),
    "start_rel1": (True, 1000, 1e-20, 1),
    "max_iter": (False, 15, 1e-20, 1),
}
OP = "Qsw_pm_ndpsi"


@pytest.fixture(scope="module")
def setup():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _Setup(shape, 0)
        return made[shape]
    yield get
    for st in made.values():
        st.lat.close()


def _target(eps_sq, rel_prec, squarenorm):
    return eps_sq * squarenorm if rel_prec > 0 else eps_sq


def _mms_reference(st, name):
    key = ("mms", name)
    if key not in st.refs:
        shifts, max_iter, eps_sq, rel = MMS[name]
        st.refs[key] = nd.cg_mms_tm_nd(st.qpm(sw.FIXTURE), sw.cplx(st.k[0]), sw.cplx(st.k[1]), shifts, max_iter, eps_sq, rel)
    return st.refs[key]


def _mms(lat, qs, qc, case, **kw):
    it, P = lat.cg_mms_tm_nd(qs, qc, *case, **kw)
    got = [(u.download(), d.download()) for u, d in P]
    for u, d in P:
        u.free(); d.free()
    return it, lat.nd_active_shifts(), got


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", list(MMS))
@pytest.mark.parametrize("shape", SOLVE, ids=SOLVE_IDS)
def test_cg_mms_tm_nd_on_the_clover_operator(setup, shape, name, fused):
    st = setup(shape)
    shifts, max_iter, eps_sq, rel = MMS[name]
    it_ref, P_ref, drops, left = _mms_reference(st, name)
    ks, kc = sw.cplx(st.k[0]), sw.cplx(st.k[1])
    if name == "five_sorted":
        assert len(drops) >= 2 and it_ref > 0, (it_ref, drops)
    if name in ("thirty_two", "rel_prec_negative", "max_iter"):
        assert it_ref == -1
    if name == "rel_prec_negative":   # with rel_prec 0 the same run stops early
        assert 0 < nd.cg_mms_tm_nd(st.qpm(sw.FIXTURE), ks, kc, shifts, max_iter, eps_sq, 0)[0] < max_iter
    lat = st.lat
    st.at(sw.FIXTURE)
    lat.set_option("nd_fused", fused)
    qs, qc = lat.field(st.k[0]), lat.field(st.k[1])
    try:
        it, active, got = _mms(lat, qs, qc, MMS[name], op=OP)
        it2, active2, got2 = _mms(lat, qs, qc, MMS[name], op=OP)
    finally:
        qs.free(); qc.free()
        lat.set_option("nd_fused", 1)
    assert (it2, active2) == (it, active)                               # two solves: the same bits
    for (u, d), (u2, d2) in zip(got, got2):
        assert np.array_equal(u, u2) and np.array_equal(d, d2)
    if it_ref == -1:
        assert it == -1, it
    else:
        assert it > 0 and abs(it - it_ref) <= 1, (it, it_ref)
    assert active == left, (active, left, drops)
    tol = 1e-10 if it_ref == -1 else 1e-9
    for s, ((u, d), (ru, rd)) in enumerate(zip(got, P_ref)):
        e = _pair_err(u, d, nd.real(ru), nd.real(rd))
        assert e < tol, (s, shifts[s], e)
    if it_ref > 0:   # the true residual of the base system, with the restated operator
        xu, xd = sw.cplx(got[0][0]), sw.cplx(got[0][1])
        au, ad = st.qpm(sw.FIXTURE)(xu, xd)
        s0 = shifts[0] ** 2
        res = np.vdot(au + s0 * xu - ks, au + s0 * xu - ks).real + np.vdot(ad + s0 * xd - kc, ad + s0 * xd - kc).real
        squarenorm = np.vdot(ks, ks).real + np.vdot(kc, kc).real
        assert res <= 10 * _target(eps_sq, rel, squarenorm), (res, _target(eps_sq, rel, squarenorm))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", list(HER))
@pytest.mark.parametrize("shape", SOLVE, ids=SOLVE_IDS)
def test_cg_her_nd_on_the_clover_operator(setup, shape, name, fused):
    st = setup(shape)
    start, max_iter, eps_sq, rel = HER[name]
    ks, kc = sw.cplx(st.k[0]), sw.cplx(st.k[1])
    x0 = 0.1 * st.k[4] if start else np.zeros_like(st.k[4])
    x0u, x0d = sw.cplx(x0), sw.cplx(x0[::-1].copy())
    key = ("her", name)
    if key not in st.refs:
        st.refs[key] = nd.cg_her_nd(st.qpm(sw.FIXTURE), x0u, x0d, ks, kc, max_iter, eps_sq, rel)
    it_ref, ru, rd = st.refs[key]
    assert (it_ref == -1) == (name == "max_iter"), it_ref
    lat = st.lat
    st.at(sw.FIXTURE)
    lat.set_option("nd_fused", fused)
    qs, qc = lat.field(st.k[0]), lat.field(st.k[1])
    runs = []
    try:
        for _ in range(2):
            pu, pd = lat.field(sw.real(x0u)), lat.field(sw.real(x0d))
            it = lat.cg_her_nd(pu, pd, qs, qc, max_iter, eps_sq, rel, lat.Vh, op=OP)
            runs.append((it, pu.download(), pd.download()))
            pu.free(); pd.free()
    finally:
        qs.free(); qc.free()
        lat.set_option("nd_fused", 1)
    (it, u, d), (it2, u2, d2) = runs
    assert it2 == it and np.array_equal(u, u2) and np.array_equal(d, d2)
    if it_ref == -1:
        assert it == -1, it
        assert _pair_err(u, d, nd.real(ru), nd.real(rd)) < 1e-10
        return
    assert it > 0 and abs(it - it_ref) <= 1, (it, it_ref)
    assert _pair_err(u, d, nd.real(ru), nd.real(rd)) < 1e-9
    xu, xd = sw.cplx(u), sw.cplx(d)
    au, ad = st.qpm(sw.FIXTURE)(xu, xd)
    res = np.vdot(au - ks, au - ks).real + np.vdot(ad - kc, ad - kc).real
    squarenorm = np.vdot(ks, ks).real + np.vdot(kc, kc).real
    assert res <= 10 * _target(eps_sq, rel, squarenorm), res


def test_iteration_counts_of_the_reference():
    """The reference's own 4^4 runs (tools/make_golden_ndsw.py) on its gauge field and sources (those of ref_nd_4x4.npz).  The 8^4
    counts belong to the reference's RANLUX fields, which exist only where the reference library is built: tests/test_ndsw_restate.py
    reproduces them with the restated solvers, and the cases above tie the device to those solvers."""
    from tmlqcd_amd import Lattice
    L = 4
    s = json.load(open(os.path.join(GOLD, "ref_ndsw_scalars_4x4.json")))
    base = np.load(os.path.join(GOLD, "ref_nd_4x4.npz"))
    mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
    lat = Lattice(L, L, L, L, kappa=s["kappa"], mu=0.0)
    try:
        g = np.ascontiguousarray(base["gauge"])
        lat.set_gauge(g)
        lat.sw_term(g, s["kappa"], s["c_sw"])
        lat.sw_invert_nd(s["mshift"])
        assert lat.sw_invert_failures() == 0
        lat.set_nd(mb, eb, c)
        qs, qc = lat.field(np.ascontiguousarray(base["k_s"])), lat.field(np.ascontiguousarray(base["k_c"]))
        gh, gm = s["cg_her_nd"], s["cg_mms_tm_nd"]
        pu, pd = lat.field().zero(), lat.field().zero()
        it = lat.cg_her_nd(pu, pd, qs, qc, gh["max_iter"], gh["eps_sq"], gh["rel_prec"], lat.Vh, op=OP)
        assert abs(it - gh["iters"]) <= 1, (it, gh["iters"])
        n = lat.square_norm(pu, lat.Vh) + lat.square_norm(pd, lat.Vh)
        assert abs(n - gh["sol_norm"]) <= 1e-9 * gh["sol_norm"]
        it, P = lat.cg_mms_tm_nd(qs, qc, gm["shifts"], gm["max_iter"], gm["eps_sq"], gm["rel_prec"], op=OP)
        assert abs(it - gm["iters"]) <= 1, (it, gm["iters"])
        assert lat.nd_active_shifts() == len(gm["shifts"]) - len(gm["drops"])
        for (u, d), want in zip(P, gm["sol_norms"]):
            n = lat.square_norm(u, lat.Vh) + lat.square_norm(d, lat.Vh)
            assert abs(n - want) <= 1e-9 * want
    finally:
        lat.close()


@pytest.mark.parametrize("fused", [1, 0])
def test_polling_interval_does_not_change_the_result(setup, fused):
    st = setup((6, 10, 2, 4))
    lat = st.lat
    st.at(sw.FIXTURE)
    lat.set_option("nd_fused", fused)
    qs, qc = lat.field(st.k[0]), lat.field(st.k[1])
    runs = {}
    try:
        for batch in (1, 4, 7):
            lat.set_option("cg_batch", batch)
            for name in ("five_sorted", "rel_prec_negative"):
                runs[(batch, name)] = _mms(lat, qs, qc, MMS[name], op=OP)
            pu, pd = lat.field().zero(), lat.field().zero()
            it = lat.cg_her_nd(pu, pd, qs, qc, 1000, 1e-20, 1, lat.Vh, op=OP)
            runs[(batch, "her")] = (it, 1, [(pu.download(), pd.download())])
            pu.free(); pd.free()
    finally:
        qs.free(); qc.free()
        lat.set_option("cg_batch", 4)
        lat.set_option("nd_fused", 1)
    for name in ("five_sorted", "rel_prec_negative", "her"):
        it1, act1, x1 = runs[(1, name)]
        for batch in (4, 7):
            it, act, x = runs[(batch, name)]
            assert (it, act) == (it1, act1), (name, batch, it, it1)
            for (u, d), (u1, d1) in zip(x, x1):
                assert np.array_equal(u, u1) and np.array_equal(d, d1), (name, batch)


@pytest.mark.parametrize("fused", [1, 0])
def test_op_zero_is_the_unsuffixed_call(setup, fused):
    """tmhip_cg_her_nd / tmhip_cg_mms_tm_nd are the op = TMHIP_ND_OP_QTM_PM case of the same engine: the same bits, and the
    twisted-mass operator needs no clover term."""
    st = setup((6, 10, 2, 4))
    lat = st.lat
    lat.set_nd(*sw.FIXTURE)
    lat.set_option("nd_fused", fused)
    qs, qc = lat.field(st.k[0]), lat.field(st.k[1])
    try:
        a = _mms(lat, qs, qc, MMS["five_sorted"])
        b = _mms(lat, qs, qc, MMS["five_sorted"], op="Qtm_pm_ndpsi")
        assert a[:2] == b[:2]
        for (u, d), (u1, d1) in zip(a[2], b[2]):
            assert np.array_equal(u, u1) and np.array_equal(d, d1)
        c = _mms(lat, qs, qc, MMS["five_sorted"], op=OP)
        assert not np.array_equal(a[2][0][0], c[2][0][0])               # and the clover operator is another one
        her = []
        for op in (None, "Qtm_pm_ndpsi"):
            pu, pd = lat.field().zero(), lat.field().zero()
            it = lat.cg_her_nd(pu, pd, qs, qc, 1000, 1e-20, 1, lat.Vh, op=op)
            her.append((it, pu.download(), pd.download()))
            pu.free(); pd.free()
        assert her[0][0] == her[1][0] and np.array_equal(her[0][1], her[1][1]) and np.array_equal(her[0][2], her[1][2])
    finally:
        qs.free(); qc.free()
        lat.set_option("nd_fused", 1)
