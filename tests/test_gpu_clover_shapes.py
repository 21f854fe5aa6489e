"""GPU: the clover twisted-mass operators (Qsw_*, Msw_*, their fp32 twins) and cg_her / mixed_cg_her / rg_mixed_cg_her on
Qsw_pm_psi against the CPU oracle on ragged and padded-XCD-grid lattices, in every form the shared stencil launcher takes:
block 64 / 256, chunk / tile / slab order with grids padded to a multiple of eight, the LDS-staged kernel, both "gauge_cache"
instances, partial last waves.  The clover blocks are computed on each side from the links (sw_term / sw_invert), twisted
boundary phases theta = (1, 0.3, -0.2, 0.5).

* test_shapes_reach_the_forms (no GPU): the launcher's choices restated, so a change of shape cannot leave the form it is for;
* operators: every clover entry point at mu = 0.02, mu = 0 (one set of sw_inv) and mu3 = 0.07, and l == k;
* launch forms: every "xcd" x "gauge_cache" (x "lds") form and "minw" 4 on the padded and staged shapes;
* fp32: Hopping_Matrix_32 and Qsw_pm_psi_32 against the fp64 oracle on the rounded input, and the fp32 clover copy going stale;
* solvers: cg_her (unfused, fused on padded tile / chunk / slab grids, staged; every polling interval; a run to max_iter),
  mixed_cg_her, rg_mixed_cg_her, and the split-phase rehearsal (loopback 1 / 3).
"""
import numpy as np
import pytest

from tests.util import TOL, random_gauge, random_spinor, rel_err

gpu = pytest.mark.gpu

KAPPA, C_SW = 0.13, 1.57
MU, MU3 = 0.02, 0.07
THETA = (1.0, 0.3, -0.2, 0.5)
POINTS = {"mu": (MU, 0.0), "mu0": (0.0, 0.0), "mu3": (MU, MU3)}       # (mu, mu3)
TOL_HOP32, TOL_QSW32 = 2e-6, 1e-5                                    # TOL32 of test_gpu_mixed.py; test_gpu_clover.py's Qsw_pm_psi_32 bound
# id: ((T, LX, LY, LZ), "block")
SHAPES = {
    "A": ((2, 2, 2, 2), 0),         # one partial wave; +mu and -mu neighbours coincide
    "B": ((4, 2, 6, 2), 0),         # LZ/2 = 1
    "C": ((6, 10, 2, 4), 0),        # 4 blocks, last wave 48 lanes; cg_her not fusable
    "D": ((10, 10, 6, 14), 0),      # 66 blocks padded to 72, partial last wave, LZ/2 odd, no whole slices: chunk order only
    "E": ((22, 8, 8, 6), 0),        # 66 whole blocks padded to 72, whole slices: tile order with t-group 2; cg_her fusable
    "F": ((8, 6, 12, 16), 0),       # 72 blocks, 9 per slice: with "xcd" 3 the slab order on 128 blocks with padding slabs
    "G": ((4, 4, 16, 8), 256),      # the LDS-staged instances, 4 blocks
    "H": ((22, 6, 16, 16), 256),    # staged, 66 blocks padded to 72, tile order with t-group 2
    "I": ((18, 12, 12, 14), 256),   # 71 blocks padded to 72, partial last wave, not staged: the block-256 gather kernel
}
OPS = ("Qsw_pm_psi", "Qsw_psi", "Qsw_plus_psi", "Qsw_minus_psi", "Qsw_sq_psi", "Msw_psi", "Msw_plus_psi", "Msw_minus_psi")
HEO = tuple(("H_eo_sw_inv_psi", ieo, sign) for ieo in (0, 1) for sign in (+1, -1))
CASES = tuple(("op", n) for n in OPS) + HEO + tuple((n, ieo) for n in ("clover_gamma5", "clover") for ieo in (0, 1)) + \
    (("clover_inv", +1), ("clover_inv", -1), ("Msw_full",))
FORM_CASES = (("op", "Qsw_pm_psi"), ("op", "Qsw_minus_psi")) + HEO
DEFAULTS = {"xcd": 2, "gauge_cache": -1, "minw": 0, "lds": 1, "lds32": 0, "cg_fused_dot": 2, "cg_batch": 4}


def _grid(shape, block, xcd=2, lds=1):
    """launch_one / stg_ok of hopping_impl.inc for an unsplit fp64 launch over all sites of one parity."""
    T, LX, LY, LZ = shape
    Vh, face, YZh, LZh = T * LX * LY * LZ // 2, LX * LY * LZ // 2, LY * LZ // 2, LZ // 2
    bs = block or (64 if Vh < 131072 else 256)                        # tmhip_hop_block
    nb = (Vh + bs - 1) // bs
    g = {"Vh": Vh, "face": face, "bs": bs, "blocks": nb, "grid": nb, "order": "none", "tgrp": 0}
    whole_slices = face % bs == 0
    short_t = whole_slices and T < 24 and YZh * 4 * 1536 > (1 << 20)
    want_slab = xcd == 3 or (xcd == 2 and (YZh * 4 * 1536 > (2 << 20) or short_t))
    if want_slab and nb >= 64 and whole_slices and face // bs >= 8:
        slab = (face // bs + 7) // 8
        g.update(order="slab", grid=8 * slab * T, pad_slabs=8 * slab - face // bs)
    elif xcd and nb >= 64:
        g.update(order="chunk", grid=8 * ((nb + 7) // 8))
        if xcd >= 2 and whole_slices:
            grp = next((c for c in (4, 5, 6, 3, 2) if T % c == 0), 0)
            if grp:
                g.update(order="tile", tgrp=grp)
    g["staged"] = bool(lds and bs == 256 and face % 256 == 0 and Vh % 256 == 0 and 64 % LZh == 0 and YZh >= 64)
    return g


def test_shapes_reach_the_forms():
    """The premise of the cases below (a condition, not a measurement): what each shape makes the launcher do."""
    g = {k: _grid(*v) for k, v in SHAPES.items()}
    assert (g["A"]["Vh"], g["A"]["blocks"]) == (8, 1)
    assert (g["B"]["Vh"], g["B"]["blocks"], SHAPES["B"][0][3] // 2) == (48, 1, 1)
    assert (g["C"]["Vh"], g["C"]["blocks"], g["C"]["Vh"] % 64, g["C"]["order"]) == (240, 4, 48, "none")
    d = g["D"]
    assert (d["Vh"], d["bs"], d["blocks"], d["grid"], d["order"]) == (4200, 64, 66, 72, "chunk")
    assert d["Vh"] % 64 != 0 and d["face"] == 420 and d["face"] % 64 != 0 and (SHAPES["D"][0][3] // 2) % 2 == 1
    e = g["E"]
    assert (e["Vh"], e["bs"], e["blocks"], e["grid"], e["order"], e["tgrp"]) == (4224, 64, 66, 72, "tile", 2)
    assert e["Vh"] % 64 == 0 and (e["face"], e["face"] % 64) == (192, 0)
    assert _grid(*SHAPES["E"], xcd=1)["order"] == "chunk" and _grid(*SHAPES["E"], xcd=1)["grid"] == 72
    f = g["F"]
    assert (f["Vh"], f["blocks"], f["grid"], f["order"], f["face"], f["face"] % 64) == (4608, 72, 72, "tile", 576, 0)
    f3 = _grid(*SHAPES["F"], xcd=3)
    assert (f3["order"], f3["grid"], f3["pad_slabs"]) == ("slab", 128, 7)
    assert _grid(*SHAPES["D"], xcd=3)["order"] == "chunk" and _grid(*SHAPES["E"], xcd=3)["order"] == "tile"   # no slab order there
    assert (g["G"]["Vh"], g["G"]["bs"], g["G"]["blocks"], g["G"]["grid"], g["G"]["staged"]) == (1024, 256, 4, 4, True)
    h = g["H"]
    assert (h["Vh"], h["bs"], h["blocks"], h["grid"], h["order"], h["tgrp"], h["staged"]) == (16896, 256, 66, 72, "tile", 2, True)
    assert h["Vh"] % 256 == 0 and h["face"] % 256 == 0
    assert not _grid(*SHAPES["G"], lds=0)["staged"] and not _grid(*SHAPES["H"], lds=0)["staged"]
    i = g["I"]
    assert (i["Vh"], i["bs"], i["blocks"], i["grid"], i["order"], i["staged"]) == (18144, 256, 71, 72, "chunk", False)
    assert i["Vh"] % 64 != 0 and i["face"] % 256 != 0
    for k in "DEF":   # "block" 64 is what the automatic choice takes on these: the same grids
        assert _grid(SHAPES[k][0], 64) == g[k]
    assert [k for k in sorted(g) if g[k]["staged"]] == ["G", "H"]
    # cg_her fuses its reductions into the stencils only on whole blocks
    assert g["C"]["Vh"] % 64 != 0 and all(g[k]["Vh"] % g[k]["bs"] == 0 for k in "EFH")
    assert max(2 * v["Vh"] for v in g.values()) == 36288 and 2 * g["H"]["Vh"] == 33792


class _Setup:
    """One lattice on both sides: the same gauge, kappa, theta and mu; clover blocks computed on each side from the links."""

    def __init__(self, shape, block, c_sw=C_SW):
        from oracle.oraclebind import Oracle
        from tmlqcd_amd import Lattice
        self.shape, self.block = shape, block
        self.orc = Oracle(*shape, kappa=KAPPA, mu=MU, theta=THETA, threads=8)
        self.lat = Lattice(*shape, kappa=KAPPA, mu=MU, theta=THETA)
        seed = 2000 + sum(shape) * 7 + shape[0]
        self.gauge = random_gauge(seed, self.orc.VPR)
        self.orc.set_gauge(self.gauge)
        self.lat.set_gauge(self.gauge)
        if block:
            self.lat.set_option("block", block)
        self.N = self.orc.Vh
        self.k, self.j, self.q = (random_spinor(seed + i, self.N) for i in (1, 2, 3))   # operator inputs, the solvers' source
        self.k32 = self.k.astype(np.float32)
        self.refs = {}
        self.mu, self.mu3, self.pt = None, 0.0, None
        self.sw_terms(c_sw)

    def sw_terms(self, c_sw):
        self.sw = self.orc.sw_term(KAPPA, c_sw)
        self.lat.sw_term(self.gauge, KAPPA, c_sw)
        self.mu = None
        self.point("mu")

    def point(self, name):
        """Both sides at POINTS[name]: mu (with the inverse blocks rebuilt for it) and mu3."""
        mu, mu3 = POINTS[name]
        if mu != self.mu:
            self.swi, fails = self.orc.sw_invert(self.sw, 0, mu)
            assert fails == 0
            self.orc.set_mu(mu)
            self.orc.set_clover(self.sw, self.swi)
            self.lat.set_mu(mu)
            self.lat.sw_invert(0, mu)
            self.mu = mu
        if mu3 != self.mu3:
            self.orc.set_mu3(mu3)
            self.lat.set_mu3(mu3)
            self.mu3 = mu3
        self.pt = name
        return self

    def restore(self):
        for name, value in DEFAULTS.items():
            self.lat.set_option(name, value)

    # ---- the oracle
    def _new(self):
        return self.orc.new_field()

    def _oracle(self, case):
        orc, N, k, j, mu = self.orc, self.N, self.k, self.j, self.mu
        r = self._new()
        if case[0] == "op":
            orc.op(case[1], r, k.copy())
        elif case[0] == "H_eo_sw_inv_psi":
            orc.Hopping_Matrix(case[1], r, k)
            orc.clover_inv(r, case[2], mu)
        elif case[0] == "clover_gamma5":
            orc.clover_gamma5(case[1], r, k, j, -mu)
        elif case[0] == "clover":
            orc.clover(case[1], r, k, j, mu)
        elif case[0] == "clover_inv":
            r[:N] = k
            orc.clover_inv(r, case[1], mu)
        else:
            ro = self._new()
            orc.Msw_full(r, ro, k, j)
            return np.concatenate([r[:N], ro[:N]])
        return r[:N].copy()

    def reference(self, case):
        key = (self.pt, case)
        if key not in self.refs:
            self.refs[key] = self._oracle(case)
        return self.refs[key]

    def reference32(self):
        """fp64 oracle on the fp32-rounded input (at the point "mu"): Hopping_Matrix of both parities, Qsw_pm_psi."""
        if "fp32" not in self.refs:
            k = self.k32.astype(np.float64)
            out = {}
            for ieo in (0, 1):
                r = self._new()
                self.orc.Hopping_Matrix(ieo, r, k)
                out["Hopping_Matrix_32_%d" % ieo] = r[:self.N].copy()
            r = self._new()
            self.orc.op("Qsw_pm_psi", r, k.copy())
            out["Qsw_pm_psi_32"] = r[:self.N].copy()
            self.refs["fp32"] = out
        return self.refs["fp32"]

    def cg_reference(self):
        """orc.cg_her on Qsw_pm_psi at the point "mu": (iterations, residual history, solution)."""
        if "cg" not in self.refs:
            P = self._new()
            it, hist = self.orc.cg_her(P, self.q.copy(), 2000, 1e-20, 1, self.N, "Qsw_pm_psi")
            assert it > 5, it
            self.refs["cg"] = (it, hist.copy(), P[:self.N].copy())
        return self.refs["cg"]

    # ---- the device
    def device(self, cases):
        lat, mu = self.lat, self.mu
        dk, dj, dl, do = lat.field(self.k), lat.field(self.j), lat.field(), lat.field()
        out = {}
        try:
            for case in cases:
                if case[0] == "op":
                    lat.op(case[1], dl, dk)
                elif case[0] == "H_eo_sw_inv_psi":
                    lat.H_eo_sw_inv_psi(dl, dk, case[1], case[2], mu)
                elif case[0] == "clover_gamma5":
                    lat.clover_gamma5(case[1], dl, dk, dj, -mu)
                elif case[0] == "clover":
                    lat.clover(case[1], dl, dk, dj, mu)
                elif case[0] == "clover_inv":
                    dl.upload(self.k)
                    lat.clover_inv(dl, case[1], mu)
                else:
                    lat.Msw_full(dl, do, dk, dj)
                    out[case] = np.concatenate([dl.download(), do.download()])
                    continue
                out[case] = dl.download()
        finally:
            for f in (dk, dj, dl, do):
                f.free()
        return out

    def device32(self):
        lat = self.lat
        dk, dl = lat.field32(self.k32), lat.field32()
        out = {}
        try:
            for ieo in (0, 1):
                lat.Hopping_Matrix_32(ieo, dl, dk)
                out["Hopping_Matrix_32_%d" % ieo] = dl.download().astype(np.float64)
            lat.Qsw_pm_psi_32(dl, dk)
            out["Qsw_pm_psi_32"] = dl.download().astype(np.float64)
        finally:
            dk.free(); dl.free()
        return out


@pytest.fixture(scope="module")
def setup():
    made = {}

    def get(sid, block=None):
        shape, blk = SHAPES[sid]
        key = (shape, blk if block is None else block)
        if key not in made:
            made[key] = _Setup(*key)
        return made[key]
    yield get
    for st in made.values():
        st.lat.close()


def _check(st, cases, tag):
    got = st.device(cases)
    errs = {c: rel_err(got[c], st.reference(c)) for c in cases}
    bad = {c: e for c, e in errs.items() if not e < TOL}
    assert not bad, (st.shape, st.block, st.pt, tag, bad)


def _check32(st, tag, worst):
    got, ref = st.device32(), st.reference32()
    errs = {n: rel_err(got[n], ref[n]) for n in ref}
    for n, e in errs.items():
        worst[n] = max(worst.get(n, 0.0), e)
    print("fp32 %s block %d %s: %s" % ("x".join(map(str, st.shape)), st.block, tag, " ".join("%s %.3e" % ne for ne in sorted(errs.items()))))
    bad = {n: e for n, e in errs.items() if not e < (TOL_QSW32 if n == "Qsw_pm_psi_32" else TOL_HOP32)}
    assert not bad, (st.shape, st.block, tag, bad)


# ---------------------------------------------------------------- 1. operators
@gpu
@pytest.mark.parametrize("point", list(POINTS))
@pytest.mark.parametrize("sid", list(SHAPES))
def test_operators_match_oracle(setup, sid, point):
    st = setup(sid).point(point)
    mu = st.mu
    sw, swi = st.lat.get_clover()
    n = st.orc.V if mu != 0.0 else st.orc.V // 2          # mu = 0: only the +mu set exists (clover_invert.c:225)
    assert rel_err(sw, st.sw) < TOL and rel_err(swi[:n], st.swi[:n]) < TOL, (st.shape, point)
    assert mu != 0.0 or not swi[n:].any()
    _check(st, CASES, "operators")
    if point == "mu3":   # mu3 really changes the operator
        with_mu3 = st.reference(("op", "Qsw_plus_psi"))
        assert rel_err(with_mu3, st.point("mu").reference(("op", "Qsw_plus_psi"))) > 1e-3


@gpu
@pytest.mark.parametrize("sid", ["C", "E"])
def test_Qsw_minus_psi_in_place(setup, sid):
    """l == k (invert_clover_eo.c:128): k enters the last launch only through the element-wise epilogue."""
    st = setup(sid).point("mu")
    dl = st.lat.field(st.k)
    try:
        st.lat.op("Qsw_minus_psi", dl, dl)
        assert rel_err(dl.download(), st.reference(("op", "Qsw_minus_psi"))) < TOL
    finally:
        dl.free()


# ---------------------------------------------------------------- 2. launch forms
FORMS = [("D", 0), ("D", 64), ("E", 0), ("E", 64), ("F", 0), ("F", 64), ("I", 256), ("G", 256), ("H", 256)]


@gpu
@pytest.mark.parametrize("sid,block", FORMS, ids=["%s_b%d" % f for f in FORMS])
def test_operators_in_every_launch_form(setup, sid, block):
    st = setup(sid, block).point("mu")
    lat = st.lat
    try:
        for lds in ((1, 0) if sid in "GH" else (1,)):      # "lds" 0: the gather kernel at block 256
            lat.set_option("lds", lds)
            for xcd in (0, 1, 2, 3, 4):
                for gc in (0, 1):
                    lat.set_option("xcd", xcd)
                    lat.set_option("gauge_cache", gc)
                    _check(st, FORM_CASES, {"lds": lds, "xcd": xcd, "gauge_cache": gc})
            lat.set_option("xcd", 2)
            lat.set_option("gauge_cache", -1)
            lat.set_option("minw", 4)
            _check(st, FORM_CASES, {"lds": lds, "minw": 4})
            lat.set_option("minw", 0)
    finally:
        st.restore()


# ---------------------------------------------------------------- 3. fp32 twins
@gpu
@pytest.mark.parametrize("sid", ["B", "C", "D", "E", "G", "H", "I"])
def test_fp32_twins_match_fp64_oracle(setup, sid):
    st = setup(sid).point("mu")
    lat = st.lat
    worst = {}
    try:
        _check32(st, "default", worst)
        if sid in "DH":
            for xcd in (0, 1, 3, 4):
                lat.set_option("xcd", xcd)
                _check32(st, "xcd %d" % xcd, worst)
            lat.set_option("xcd", 2)
        if sid in "GH":
            lat.set_option("lds32", 1)
            for xcd in ((0, 1, 2, 3, 4) if sid == "H" else (2,)):
                lat.set_option("xcd", xcd)
                _check32(st, "lds32 1 xcd %d" % xcd, worst)
    finally:
        st.restore()
    print("fp32 maxima %s %s block %d: %s" % (sid, "x".join(map(str, st.shape)), st.block, " ".join("%s %.3e" % ne for ne in sorted(worst.items()))))


@gpu
def test_fp32_clover_copy_follows_sw_term():
    """Qsw_pm_psi_32 converts the clover blocks once; sw_term / sw_invert after that must invalidate the fp32 copy."""
    st = _Setup(*SHAPES["C"])
    try:
        old = st.reference32()["Qsw_pm_psi_32"]
        assert rel_err(st.device32()["Qsw_pm_psi_32"], old) < TOL_QSW32
        st.refs.clear()
        st.sw_terms(1.0)
        new = st.reference32()["Qsw_pm_psi_32"]
        assert rel_err(old, new) > 100 * TOL_QSW32        # a stale copy cannot pass
        assert rel_err(st.device32()["Qsw_pm_psi_32"], new) < TOL_QSW32
    finally:
        st.lat.close()


# ---------------------------------------------------------------- 4. solvers on Qsw_pm_psi
def _check_cg(st, tag):
    """The acceptance of test_gpu_clover.py::test_clover_cg_with_reductions_fused_into_the_stencils."""
    it_ref, hist_ref, P_ref = st.cg_reference()
    lat, N = st.lat, st.N
    dq, dp = lat.field(st.q), lat.field().zero()
    try:
        it, hist = lat.cg_her(dp, dq, 2000, 1e-20, 1, N, op="Qsw_pm_psi")
        sol = dp.download()
    finally:
        dq.free(); dp.free()
    assert abs(it - it_ref) <= 1, (st.shape, tag, it, it_ref)
    m = min(len(hist), len(hist_ref)) - 1
    assert m > 0 and np.allclose(hist[:m], hist_ref[:m], rtol=1e-6), (st.shape, tag)
    assert rel_err(sol, P_ref) < 1e-9, (st.shape, tag)


# (shape, "xcd", "cg_batch"): C unfused (cg_dot_kernel), E fused on the padded tile grid and on the chunk grid, F on the slab grid
# with padding slabs, H the staged kernel at block 256 on a padded grid
CG = [("C", 2, 4), ("E", 2, 4), ("E", 1, 4), ("F", 3, 4), ("H", 2, 4), ("E", 2, 1), ("E", 2, 7), ("E", 1, 1), ("E", 1, 7)]


@gpu
@pytest.mark.parametrize("fused", [2, 0])
@pytest.mark.parametrize("sid,xcd,batch", CG, ids=["%s_xcd%d_batch%d" % c for c in CG])
def test_cg_her_matches_oracle(setup, sid, xcd, batch, fused):
    st = setup(sid).point("mu")
    lat = st.lat
    try:
        lat.set_option("xcd", xcd)
        lat.set_option("cg_batch", batch)
        lat.set_option("cg_fused_dot", fused)
        _check_cg(st, {"xcd": xcd, "cg_batch": batch, "cg_fused_dot": fused})
    finally:
        st.restore()


@gpu
def test_cg_her_stops_at_max_iter(setup):
    st = setup("E").point("mu")
    N = st.N
    P = st.orc.new_field()
    it_ref, hist_ref = st.orc.cg_her(P, st.q.copy(), 7, 1e-30, 1, N, "Qsw_pm_psi")
    dq, dp = st.lat.field(st.q), st.lat.field().zero()
    try:
        it, hist = st.lat.cg_her(dp, dq, 7, 1e-30, 1, N, op="Qsw_pm_psi")
        sol = dp.download()
    finally:
        dq.free(); dp.free()
    assert (it_ref, len(hist_ref)) == (-1, 7) and (it, len(hist)) == (-1, 7), (it_ref, it, len(hist_ref), len(hist))
    assert np.allclose(hist[:6], hist_ref[:6], rtol=1e-6) and rel_err(sol, P[:N]) < 1e-9


@gpu
@pytest.mark.parametrize("solver", ["mixed_cg_her", "rg_mixed_cg_her"])
@pytest.mark.parametrize("sid", ["D", "E"])
def test_mixed_solvers_reach_fp64_residual(setup, sid, solver):
    """The bounds of test_gpu_clover.py::test_clover_cg_and_mixed_cg."""
    st = setup(sid).point("mu")
    lat, orc, N, q = st.lat, st.orc, st.N, st.q
    eps_sq = 1e-20
    _, _, P_ref = st.cg_reference()
    dq, dp = lat.field(q), lat.field().zero()
    try:
        if solver == "mixed_cg_her":
            it, _ = lat.mixed_cg_her(dp, dq, 5000, eps_sq, 1, N, op="Qsw_pm_psi")
        else:
            it, _ = lat.rg_mixed_cg_her(dp, dq, 5000, eps_sq, 1, N, delta=0.1, op="Qsw_pm_psi")
        sol = dp.download()
    finally:
        dq.free(); dp.free()
    assert it > 0, it
    full = orc.new_field(); full[:N] = sol
    chk = orc.new_field(); orc.op("Qsw_pm_psi", chk, full)
    res = ((chk[:N] - q) ** 2).sum() / (q ** 2).sum()      # the true fp64 residual, by the oracle
    assert res <= eps_sq, (st.shape, solver, res)
    assert rel_err(sol, P_ref) < 1e-8, (st.shape, solver)


@gpu
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("sid", ["D", "E"])
def test_split_phase_rehearsal(setup, sid, mode):
    """A T-split rank rehearsed on one GPU (1: device-to-device copies, 3: the direct carrier onto oneself): on D waves straddle
    time-slices (the per-lane choice of the skipped hop), on E they do not."""
    st = setup(sid).point("mu")
    st.cg_reference()
    st.lat.set_loopback(mode)
    try:
        _check(st, (("op", "Qsw_pm_psi"),), {"loopback": mode})
        _check_cg(st, {"loopback": mode})
    finally:
        st.lat.set_loopback(0)
