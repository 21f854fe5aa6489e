"""GPU: which operator id which solver takes -- every solver entry point of the library, called through lat.lib with every id in
-1 .. 13 (the doublet entry points: -1 .. 2), max_iter = 2 and fields of the kind the id's row names, against accept / refuse sets
written here as literals, independent of the C list (tmlqcd_amd/csrc/op_table.h).

4x4x4x4, two contexts.  CLOVER: gauge, sw_term, sw_invert(EE, mu) with mu != 0 (so Qsw_minus_psi, id 10, finds the -mu set of sw_inv
it asks for) and, for the doublet's clover row, set_nd and sw_invert_nd.  PLAIN: gauge only.

On CLOVER a call returns 0 exactly for the solver's set; where it returns non-zero the solution field(s) -- for chrono_guess the two
stored vectors too, which a refusal at entry leaves alone while the first operator application came after step 1 had rewritten the
older one -- are byte-identical to before; and every accepted id is refused with fields of the other kind.  On PLAIN every clover row
is refused by every solver that otherwise takes it.

The correction monomials' clover row (apply_Z, ratcor_* on Qsw_pm_psi) asks for more than a valid clover term: the inverse must be
the one of sw_invert(EE, 0.), and apply_Z's solves run at the context's mu.  Their cases therefore run inside `ratcor_state`, which
puts CLOVER into that state (mu = 0, sw_invert(EE, 0.)) and back; accprec is generous so that an accepted ratcor_* call ends after its
first application of Z instead of failing its series."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from tmlqcd_amd import Lattice
from tmlqcd_amd.hip import FIELD_EO, FIELD_FULL

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAPPA, MU, CSW, MUBAR, EPSBAR = 0.125, 0.05, 1.0, 0.1, 0.05
IDS, ND_IDS = range(-1, 14), range(-1, 3)
FULL_ROWS, CLOVER_ROWS, ND_CLOVER_ROWS = {6, 12}, {5, 9, 10, 11}, {1}
ACCEPT = {"cg_her": {0, 1, 2, 3, 4, 5}, "cg_her_sync": {0, 1, 2, 3, 4, 5}, "chrono_guess": {0, 1, 2, 3, 4, 5},
          "mixed_cg_her": {0, 5}, "rg_mixed_cg_her": {0, 5}, "cg_mms_tm": {0, 5, 6},
          "apply_Z": {0, 5}, "ratcor_heatbath": {0, 5}, "ratcor_acc": {0, 5},
          "bicgstab_complex": {1, 2, 3, 4, 7, 8, 9, 10, 11, 12}}
ND_ACCEPT = {n: {0, 1} for n in ("cg_her_nd_op", "cg_mms_tm_nd_op", "Ptilde_ndpsi", "apply_Z_nd", "ndratcor_heatbath", "ndratcor_acc")}
RATCOR = ("apply_Z", "ratcor_heatbath", "ratcor_acc")
MAX_ITER, EPS_SQ = 2, 1.0e-20
SHIFTS, RMU, A, ACCPREC = (0.1, 0.2), (0.3, 0.4), 1.1, 1.0e30
PTILDE = (1.0, 0.5, 0.25)


class Ctx:
    """a lattice with a pool of fields; `fresh` hands out fields of one kind with known content"""

    def __init__(self, clover):
        gauge = np.load(os.path.join(GOLD, "ref_mms_4x4.npz"))["gauge"]
        self.lat = lat = Lattice(4, 4, 4, 4, kappa=KAPPA, mu=MU)
        lat.set_gauge(gauge)
        if clover:
            lat.sw_term(gauge, KAPPA, CSW)
            lat.sw_invert(0, MU)
            lat.set_nd(MUBAR, EPSBAR)
            lat.sw_invert_nd(MUBAR * MUBAR - EPSBAR * EPSBAR)
        rng = np.random.default_rng(20260)
        self.host = {k: [rng.standard_normal((n, 4, 3, 2)) for _ in range(6)] for k, n in ((FIELD_EO, lat.Vh), (FIELD_FULL, lat.V))}
        self.dev = {k: [lat.field(kind=k) for _ in range(6)] for k in self.host}

    def fresh(self, kind, n):
        for f, h in zip(self.dev[kind][:n], self.host[kind][:n]):
            f.upload(h)
        return self.dev[kind][:n]

    def unchanged(self, kind, idx):
        return all(np.array_equal(self.dev[kind][i].download(), self.host[kind][i]) for i in idx)


@pytest.fixture(scope="module")
def clover():
    return Ctx(True)


@pytest.fixture(scope="module")
def plain():
    return Ctx(False)


@contextlib.contextmanager
def ratcor_state(ctx, on):
    if on:
        ctx.lat.set_mu(0.0)
        ctx.lat.sw_invert(0, 0.0)
    try:
        yield
    finally:
        if on:
            ctx.lat.set_mu(MU)
            ctx.lat.sw_invert(0, MU)


def _d(*x):
    return (C.c_double * len(x))(*x)


def call(ctx, name, op, kind):
    """one call of entry point `name` with operator id `op` on fields of `kind`: (return code, indices of the pool fields that hold
    the solution(s), indices of the stored vectors of chrono_guess)"""
    lat, lib = ctx.lat, ctx.lat.lib
    f = ctx.fresh(kind, 6)
    N = lat.V if kind == FIELD_FULL else lat.Vh
    it, it2, e, na = C.c_int(), C.c_int(), C.c_double(), C.c_int()
    vp = C.c_void_p
    if name in ("cg_her", "cg_her_sync"):
        lat.set_option("cg_sync", int(name == "cg_her_sync"))
        try:
            return lib.tmhip_cg_her(lat.h, f[0].h, f[1].h, MAX_ITER, EPS_SQ, 0, N, op, C.byref(it), None, 0), [0], []
        finally:
            lat.set_option("cg_sync", 0)
    if name == "chrono_guess":
        return lib.tmhip_chrono_guess(lat.h, f[0].h, f[1].h, lat._handles(f[2:4]), 2, op, N, None, None), [0], [2, 3]
    if name == "mixed_cg_her":
        return lib.tmhip_mixed_cg_her(lat.h, f[0].h, f[1].h, MAX_ITER, EPS_SQ, 0, N, op, 5.0e-5, 100, C.byref(it), C.byref(it2)), [0], []
    if name == "rg_mixed_cg_her":
        return lib.tmhip_rg_mixed_cg_her(lat.h, f[0].h, f[1].h, MAX_ITER, EPS_SQ, 0, N, op, 5.0e-5, C.byref(it), None, None, None), [0], []
    if name == "cg_mms_tm":
        return lib.tmhip_cg_mms_tm(lat.h, (vp * 2)(f[0].h, f[1].h), f[2].h, _d(*SHIFTS), 2, MAX_ITER, EPS_SQ, 0, N, op, C.byref(it), None), [0, 1], []
    if name == "bicgstab_complex":
        return lib.tmhip_bicgstab_complex(lat.h, f[0].h, f[1].h, MAX_ITER, EPS_SQ, 0, N, op, C.byref(it), None, 0), [0], []
    if name == "apply_Z":
        return lib.tmhip_apply_Z(lat.h, f[0].h, f[1].h, _d(*SHIFTS), _d(*RMU), A, 2, MAX_ITER, EPS_SQ, 0, op, C.byref(e), C.byref(it)), [0], []
    if name in ("ratcor_heatbath", "ratcor_acc"):
        fn = getattr(lib, "tmhip_" + name)
        return fn(lat.h, f[0].h, _d(*SHIFTS), _d(*RMU), A, 2, MAX_ITER, ACCPREC, 0, op, C.byref(e), C.byref(na), C.byref(it)), [0], []
    if name == "cg_her_nd_op":
        return lib.tmhip_cg_her_nd_op(lat.h, f[0].h, f[1].h, f[2].h, f[3].h, MAX_ITER, EPS_SQ, 0, N, op, C.byref(it)), [0, 1], []
    if name == "cg_mms_tm_nd_op":
        return lib.tmhip_cg_mms_tm_nd_op(lat.h, (vp * 2)(f[0].h, f[1].h), (vp * 2)(f[2].h, f[3].h), f[4].h, f[5].h, _d(*SHIFTS), 2, MAX_ITER, EPS_SQ, 0,
                                         op, C.byref(it)), [0, 1, 2, 3], []
    if name == "Ptilde_ndpsi":
        return lib.tmhip_Ptilde_ndpsi(lat.h, f[0].h, f[1].h, _d(*PTILDE), 3, f[2].h, f[3].h, 0.01, 1.0, op), [0, 1], []
    if name == "apply_Z_nd":
        return lib.tmhip_apply_Z_nd(lat.h, f[0].h, f[1].h, f[2].h, f[3].h, _d(*SHIFTS), _d(*RMU), A, 2, MAX_ITER, EPS_SQ, 0, op, C.byref(e),
                                    C.byref(it)), [0, 1], []
    assert name in ("ndratcor_heatbath", "ndratcor_acc"), name
    fn = getattr(lib, "tmhip_" + name)
    return fn(lat.h, f[0].h, f[1].h, _d(*SHIFTS), _d(*RMU), A, 2, MAX_ITER, ACCPREC, 0, op, C.byref(e), C.byref(na), C.byref(it)), [0, 1], []


def row_kind(op):
    return FIELD_FULL if op in FULL_ROWS else FIELD_EO


@pytest.mark.parametrize("name", sorted(ACCEPT))
def test_single_flavour_solver_takes_exactly_its_rows(clover, name):
    with ratcor_state(clover, name in RATCOR):
        for op in IDS:
            kind = row_kind(op)
            rc, sol, stored = call(clover, name, op, kind)
            print(name, "op", op, "rc", rc)
            assert (rc == 0) == (op in ACCEPT[name]), (name, op, rc)
            if rc != 0:
                assert clover.unchanged(kind, sol), (name, op, "solution written by a refused call")
                assert clover.unchanged(kind, stored), (name, op, "stored vectors written by a refused call")
        for op in sorted(ACCEPT[name]):
            other = FIELD_EO if op in FULL_ROWS else FIELD_FULL
            rc, sol, stored = call(clover, name, op, other)
            assert rc != 0, (name, op, "accepted on fields of the other kind")
            assert clover.unchanged(other, sol + stored), (name, op)


@pytest.mark.parametrize("name", sorted(ND_ACCEPT))
def test_doublet_solver_takes_exactly_its_rows(clover, name):
    for op in ND_IDS:
        rc, sol, _ = call(clover, name, op, FIELD_EO)
        print(name, "op", op, "rc", rc)
        assert (rc == 0) == (op in ND_ACCEPT[name]), (name, op, rc)
        if rc != 0:
            assert clover.unchanged(FIELD_EO, sol), (name, op, "solution written by a refused call")
    for op in sorted(ND_ACCEPT[name]):
        rc, sol, _ = call(clover, name, op, FIELD_FULL)
        assert rc != 0, (name, op, "accepted on FULL fields")
        assert clover.unchanged(FIELD_FULL, sol), (name, op)


def test_clover_rows_need_a_clover_term(plain):
    for name, rows in sorted(ACCEPT.items()):
        for op in sorted(rows & CLOVER_ROWS):
            assert call(plain, name, op, FIELD_EO)[0] != 0, (name, op)
    for name, rows in sorted(ND_ACCEPT.items()):
        for op in sorted(rows & ND_CLOVER_ROWS):
            assert call(plain, name, op, FIELD_EO)[0] != 0, (name, op)
