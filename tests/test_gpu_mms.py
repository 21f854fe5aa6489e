"""GPU: the single-flavour multi-shift CG (tmhip_cg_mms_tm, mms.hip) against the reference's own solver/cg_mms_tm.c
(tests/golden/ref_mms_*, tools/make_golden_mms.py) and its conventions: shift drop, stopping tests, return value, refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tmlqcd_amd import Lattice
from tmlqcd_amd.hip import MMS_OPS, TmHipError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F = np.load(os.path.join(GOLD, "ref_mms_4x4.npz"))
S = json.load(open(os.path.join(GOLD, "ref_mms_scalars_4x4.json")))


def _rel(a, b):
    return np.sqrt(np.sum((a - b) ** 2) / np.sum(b ** 2))


def lattice_for(case, gauge=None, dims=(4, 4, 4, 4)):
    lat = Lattice(*dims, kappa=S["kappa"], mu=case["g_mu"])
    g = F["gauge"] if gauge is None else gauge
    lat.set_gauge(g)
    if case["op"] == "Qsw_pm_psi":
        lat.sw_term(g, S["kappa"], S["c_sw"])
        lat.sw_invert(0, case["g_mu"])
    return lat


def source(lat, case):
    return lat.full_field(F["q_full"]) if case["op"] == "Q_pm_psi" else lat.field(F["q_eo"])


@pytest.mark.parametrize("name", sorted(S["cases"]))
def test_cases_against_the_reference(name):
    case = S["cases"][name]
    lat = lattice_for(case)
    q = source(lat, case)
    it, reached, P = lat.cg_mms_tm(q, case["shifts"], case["max_iter"], case["eps_sq"], case["rel_prec"], op=case["op"])
    ref_it = case["iters"]
    assert (it == -1) == (ref_it == -1) and abs(it - ref_it) <= 1, (it, ref_it)
    assert lat.mms_active_shifts() == case["active_at_exit"]
    assert abs(reached - case["reached_prec"]) <= 0.5 * case["reached_prec"], (reached, case["reached_prec"])
    if case["iters"] != -1:
        tgt = case["eps_sq"] * (np.sum(F["q_eo"] ** 2) if case["rel_prec"] else 1.0)
        assert reached <= tgt
    for k in range(len(case["shifts"])):
        assert _rel(P[k].download(), F["%s_P%d" % (name, k)]) < 1e-9, k
    assert np.array_equal(q.download(), F["q_full"] if case["op"] == "Q_pm_psi" else F["q_eo"])   # Q is not modified
    lat.close()


@pytest.mark.parametrize("name", ["qtm", "qsw"])
def test_true_residual_of_every_kept_shift(name):
    """|(A + shifts[s]^2) P_s - Q|^2 with the device operator, for every shift that was not dropped"""
    case = S["cases"][name]
    lat = lattice_for(case)
    q = source(lat, case)
    it, reached, P = lat.cg_mms_tm(q, case["shifts"], case["max_iter"], case["eps_sq"], case["rel_prec"], op=case["op"])
    Q = F["q_eo"]
    ap = lat.field()
    for k in range(lat.mms_active_shifts()):
        lat.op(case["op"], ap, P[k])
        res = ap.download() + case["shifts"][k] ** 2 * P[k].download() - Q
        assert np.sum(res ** 2) <= 1e3 * case["eps_sq"], (k, np.sum(res ** 2))
    lat.close()


def _run(lat, q, shifts, max_iter, eps_sq, rel_prec, op="Qtm_pm_psi"):
    it, reached, P = lat.cg_mms_tm(q, shifts, max_iter, eps_sq, rel_prec, op=op)
    return it, reached, [p.download() for p in P]


def test_one_and_32_shifts_and_unsorted():
    case = S["cases"]["qtm"]
    lat = lattice_for(case)
    q = lat.field(F["q_eo"])
    it1, _, P1 = _run(lat, q, [0.02], 1000, 1e-22, 0)
    it5, _, P5 = _run(lat, q, case["shifts"], 1000, 1e-22, 0)
    assert it1 == it5 and _rel(P1[0], P5[0]) < 1e-12   # the first shift is the CG itself
    sh32 = [0.02 + 0.3 * k for k in range(32)]
    it32, _, P32 = _run(lat, q, sh32, 1000, 1e-22, 0)
    assert it32 == it1 and lat.mms_active_shifts() < 32
    uns = [0.02, 2.5, 0.15, 9.0, 0.6]
    itu, _, Pu = _run(lat, q, uns, 1000, 1e-22, 0)
    assert itu == it5
    for k, s in enumerate(uns):
        j = case["shifts"].index(s)
        assert _rel(Pu[k], P5[j]) < 1e-9
    lat.close()


def test_rel_prec_and_exact_convergence_at_max_iter():
    case = S["cases"]["qtm"]
    lat = lattice_for(case)
    q = lat.field(F["q_eo"])
    n = case["iters"]
    it0, r0, _ = _run(lat, q, case["shifts"], 1000, 1e-22, 0)
    assert it0 == n and r0 <= 1e-22
    it_neg, _, _ = _run(lat, q, case["shifts"], n + 5, 1e-22, -1)          # no stopping test: runs to max_iter - 1
    assert it_neg == -1
    it_exact, r_exact, _ = _run(lat, q, case["shifts"], n, 1e-22, 0)       # converges exactly at iteration max_iter - 1
    assert it_exact == -1 and r_exact <= 1e-22
    qq = float(np.sum(F["q_eo"] ** 2))
    it_rel, r_rel, _ = _run(lat, q, case["shifts"], 1000, 1e-22 / qq, 2)  # rel_prec > 0, not only 1
    assert it_rel == n and r_rel <= 1e-22 * (1 + 1e-12)
    lat.close()


def test_bit_identical_on_repeat():
    for name in ("qtm", "qsw", "qpm_full"):
        case = S["cases"][name]
        lat = lattice_for(case)
        q = source(lat, case)
        a = _run(lat, q, case["shifts"], 1000, case["eps_sq"], 0, op=case["op"])
        b = _run(lat, q, case["shifts"], 1000, case["eps_sq"], 0, op=case["op"])
        assert a[0] == b[0] and a[1] == b[1]
        assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
        lat.close()


def test_refusals():
    case = S["cases"]["qtm"]
    lat = lattice_for(case)
    q = lat.field(F["q_eo"])
    with pytest.raises(TmHipError):
        lat.cg_mms_tm(q, [0.1 * (k + 1) for k in range(33)], 100, 1e-20, 0)
    with pytest.raises(TmHipError):
        lat.cg_mms_tm(q, [], 100, 1e-20, 0)
    with pytest.raises(TmHipError):   # an EO source with the full-lattice operator: N does not match op
        lat.cg_mms_tm(q, [0.1], 100, 1e-20, 0, op="Q_pm_psi", P=[lat.field()])
    it = C.c_int()                    # cg_her takes the e/o operators only
    assert lat.lib.tmhip_cg_her(lat.h, lat.field().h, q.h, 10, 1e-20, 0, lat.Vh, MMS_OPS["Q_pm_psi"], C.byref(it), None, 0) != 0
    lat.set_loopback(True)            # the single-rank rehearsal of a T-split rank
    with pytest.raises(TmHipError):
        lat.cg_mms_tm(q, [0.1, 0.2], 100, 1e-20, 0)
    lat.close()
