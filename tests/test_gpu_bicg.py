"""GPU: BiCGstab on the device (tmhip_bicgstab_complex, bicgstab.hip) -- the two three-field complex singles against NumPy, the fused
kernels bit for bit against the sequence of singles they replace, the solver per operator against the reference's own
solver/bicgstab_complex.c (tests/golden/ref_bicg_*, tools/make_golden_bicg.py) with both settings of "bicg_fused", and the refusals.

Shapes: 4^4 and 8x6x4x12, whose VOLUME/2 = 1152 is no multiple of the 1024 sites a block walks (two blocks per plane, the second
ragged).  Iteration counts are pinned for the KIND_M operators only (tests/bicg_restate.py); every converged case must meet the
stopping bound times the fixture's margin with the CPU oracle's operator on the downloaded solution and, at 4^4, lie within
2 sqrt(bound) / sigma_min(A) of the reference's solution."""
import json
import os

import numpy as np
import pytest

from oracle.nd_restate import cplx
from tests import bicg_restate as br
from tests.util import random_gauge
from tmlqcd_amd import Lattice
from tmlqcd_amd.hip import TmHipError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F4 = np.load(os.path.join(GOLD, "ref_bicg_4x4.npz"))
S = {"4x4": json.load(open(os.path.join(GOLD, "ref_bicg_scalars_4x4.json"))),
     "8x6x4x12": json.load(open(os.path.join(GOLD, "ref_bicg_scalars_8x6x4x12.json")))}
SHAPES = {"4x4": (4, 4, 4, 4), "8x6x4x12": (8, 6, 4, 12)}
EPS = np.finfo(np.float64).eps
_GAUGE = {}


def gauge_of(tag):
    if tag not in _GAUGE:
        _GAUGE[tag] = np.load(os.path.join(GOLD, "ref_mms_4x4.npz"))["gauge"] if tag == "4x4" else random_gauge(123456, int(np.prod(SHAPES[tag])))
    return _GAUGE[tag]


def rnd(seed, n):
    return np.random.default_rng(seed).standard_normal((n, 4, 3, 2))


def new_fields(lat, full, seeds):
    n = lat.V if full else lat.Vh
    hosts = [rnd(s, n) for s in seeds]
    return hosts, [lat.full_field(h) if full else lat.field(h) for h in hosts]


# ---- 1. the two singles against NumPy
# A value is made of at most three roundings on top of products that carry one each; two correct evaluations in different orders (or
# with and without a fused multiply-add) differ by at most 8 eps times the sum of the magnitudes of the terms.
@pytest.mark.parametrize("tag", sorted(SHAPES))
@pytest.mark.parametrize("full", [False, True])
def test_singles_against_numpy(tag, full):
    lat = Lattice(*SHAPES[tag])
    N = lat.V if full else lat.Vh
    c1, c2 = 0.7 - 0.3j, -0.45 + 1.1j
    (r, s, u), (fr, fs, fu) = new_fields(lat, full, (1, 2, 3))
    lat.assign_add_mul_add_mul(fr, fs, fu, c1, c2, N)
    want = cplx(r) + (c1 * cplx(s) + c2 * cplx(u))
    scale = np.abs(cplx(r)) + abs(c1) * np.abs(cplx(s)) + abs(c2) * np.abs(cplx(u))
    assert np.all(np.abs(cplx(fr.download()) - want) <= 8 * EPS * scale)
    assert np.array_equal(fs.download(), s) and np.array_equal(fu.download(), u)
    fr.upload(r)
    lat.assign_mul_bra_add_mul_ket_add(fr, fs, fu, c1, c2, N)
    want = cplx(u) + c2 * (cplx(r) + c1 * cplx(s))
    scale = np.abs(cplx(u)) + abs(c2) * (np.abs(cplx(r)) + abs(c1) * np.abs(cplx(s)))
    assert np.all(np.abs(cplx(fr.download()) - want) <= 8 * EPS * scale)
    # element-wise, so R may be S (the header says so): R += c1 R + c2 U and R = c2 (R + c1 R) + U
    fr.upload(r)
    lat.assign_add_mul_add_mul(fr, fr, fu, c1, c2, N)
    want = cplx(r) + (c1 * cplx(r) + c2 * cplx(u))
    scale = (1 + abs(c1)) * np.abs(cplx(r)) + abs(c2) * np.abs(cplx(u))
    assert np.all(np.abs(cplx(fr.download()) - want) <= 8 * EPS * scale)
    fr.upload(r)
    lat.assign_mul_bra_add_mul_ket_add(fr, fr, fu, c1, c2, N)
    want = cplx(u) + c2 * (cplx(r) + c1 * cplx(r))
    scale = np.abs(cplx(u)) + abs(c2) * (1 + abs(c1)) * np.abs(cplx(r))
    assert np.all(np.abs(cplx(fr.download()) - want) <= 8 * EPS * scale)
    if not full:   # a prefix of an EO field: the sites behind N stay
        fr.upload(r)
        lat.assign_add_mul_add_mul(fr, fs, fu, c1, c2, 100)
        got = fr.download()
        assert np.array_equal(got[100:], r[100:]) and not np.array_equal(got[:100], r[:100])
    lat.close()


# ---- 2. the fused kernels with host scalars against the sequence of singles: the same bits
def parts(f, full):
    return [f.even(), f.odd()] if full else [f]


@pytest.mark.parametrize("tag", sorted(SHAPES))
@pytest.mark.parametrize("full", [False, True])
def test_fused_kernels_carry_the_bits_of_the_singles(tag, full):
    lat = Lattice(*SHAPES[tag])
    N, n = (lat.V if full else lat.Vh), lat.Vh
    alpha, omega, beta = 0.31 + 0.07j, 0.66 - 0.21j, -0.4 + 0.9j
    hosts, (P, r, p, s, t, hatr, v) = new_fields(lat, full, (11, 12, 13, 14, 15, 16, 17))
    _, (P2, r2, p2, s2) = new_fields(lat, full, (11, 12, 13, 14))
    # K4
    lat.assign_add_mul_add_mul(P2, p, s, alpha, omega, N)
    rho_s, err_s = 0.0, 0.0
    for a, b, c, h in zip(parts(r2, full), parts(s, full), parts(t, full), parts(hatr, full)):
        lat.assign(a, b, n)
        lat.assign_diff_mul(a, c, omega, n)
        rho_s += lat.scalar_prod(h, a, n)
        err_s += lat.square_norm(a, n)
    rho, err = lat.bicg_update(P, r, p, s, t, hatr, alpha, omega, N)
    assert np.array_equal(P.download(), P2.download()) and np.array_equal(r.download(), r2.download())
    assert not np.array_equal(P.download(), hosts[0])
    assert rho == rho_s and err == err_s, (rho, rho_s, err, err_s)
    P.upload(hosts[0])
    rho_b, err_b = lat.bicg_update(P, r, p, s, t, hatr, alpha, omega, N)      # r is an output only: the second call sees the same inputs
    assert (rho_b, err_b) == (rho, err) and np.array_equal(P.download(), P2.download()) and np.array_equal(r.download(), r2.download())
    # K3
    ts_s, tt_s = 0.0, 0.0
    for a, b in zip(parts(t, full), parts(s, full)):
        ts_s += lat.scalar_prod(a, b, n)
        tt_s += lat.square_norm(a, n)
    ts, tt = lat.bicg_pair_dot(t, s, N)
    assert ts == ts_s and tt == tt_s, (ts, ts_s, tt, tt_s)
    assert lat.bicg_pair_dot(t, s, N) == (ts, tt)
    # K2
    for a, b, c in zip(parts(s2, full), parts(r, full), parts(v, full)):
        lat.assign(a, b, n)
        lat.assign_diff_mul(a, c, alpha, n)
    lat.bicg_sub(s, r, v, alpha, N)
    assert np.array_equal(s.download(), s2.download()) and not np.array_equal(s.download(), hosts[3])
    # K5
    lat.assign_mul_bra_add_mul_ket_add(p2, v, r, -omega, beta, N)
    lat.bicg_dir(p, v, r, omega, beta, N)
    assert np.array_equal(p.download(), p2.download()) and not np.array_equal(p.download(), hosts[2])
    lat.close()


# ---- 3. the solver against the reference, per operator
def lattice_for(tag, case):
    lat = Lattice(*SHAPES[tag], kappa=S[tag]["kappa"], mu=case["g_mu"])
    g = gauge_of(tag)
    lat.set_gauge(g)
    if case["op"] in br.CLOVER:
        lat.sw_term(g, S[tag]["kappa"], S[tag]["c_sw"])
        lat.sw_invert(0, case["g_mu"])
    return lat


CASES = [(tag, name) for tag in sorted(S) for name in sorted(S[tag]["cases"])]


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("tag,name", CASES)
def test_solver_against_the_reference(tag, name, fused):
    sc, case = S[tag], S[tag]["cases"][name]
    full = case["op"] == "D_psi"
    lat = lattice_for(tag, case)
    lat.set_option("bicg_fused", fused)
    Q, P0 = br.case_fields(case, lat.V)
    N = lat.V if full else lat.Vh
    q, p = (lat.full_field(Q), lat.full_field(P0)) if full else (lat.field(Q), lat.field(P0))
    ref_it = case["iters"]
    max_iter = case["max_iter"] if case["kind"] == "M" or ref_it == -1 else 10 * ref_it
    it, hist = lat.bicgstab_complex(p, q, max_iter, case["eps_sq"], case["rel_prec"], N, op=case["op"])
    sol = p.download()
    assert np.array_equal(q.download(), Q)                      # Q is not modified
    lat.close()
    if ref_it == -1:
        assert it == -1 and len(hist) == max_iter + 1 and np.all(hist > 0)   # the max_iter cut
        return
    if case["kind"] == "M":
        assert it == ref_it, (it, ref_it)
    assert 0 < it <= max_iter
    bound = br.bound_of(case, Q)
    assert len(hist) == it + 1 and hist[-1] <= bound and np.all(hist[1:-1] > bound), hist
    orc = br.oracle_for(SHAPES[tag], gauge_of(tag), sc["kappa"], sc["c_sw"], case)
    true = float(np.sum(np.abs(cplx(Q) - br.operator(orc, case["op"])(cplx(sol))) ** 2))
    assert true <= bound * sc["margin"], (true, bound)
    if tag == "4x4":
        dist = np.sqrt(np.sum((sol - F4[name + "_P"]) ** 2))
        assert dist <= 2.0 * np.sqrt(bound) / case["sigma_min"], (dist, bound, case["sigma_min"])


def test_solver_repeats_bit_for_bit():
    case = S["8x6x4x12"]["cases"]["mtm_plus_sym"]
    lat = lattice_for("8x6x4x12", case)
    Q, P0 = br.case_fields(case, lat.V)
    for fused in (1, 0):
        lat.set_option("bicg_fused", fused)
        out = []
        for rep in range(2):
            q, p = lat.field(Q), lat.field(P0)
            it, hist = lat.bicgstab_complex(p, q, case["max_iter"], case["eps_sq"], case["rel_prec"], lat.Vh, op=case["op"])
            out.append((it, hist.copy(), p.download()))
        assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    lat.close()


# ---- 4. refusals: a message, P and the count untouched
def test_refusals():
    import ctypes as C
    tag, case = "4x4", S["4x4"]["cases"]["mtm_plus_sym"]
    lat = lattice_for(tag, case)
    Q, _ = br.case_fields(case, lat.V)
    P0 = rnd(5, lat.Vh)
    q, p = lat.field(Q), lat.field(P0)
    qf, pf = lat.full_field(rnd(6, lat.V)), lat.full_field(rnd(7, lat.V))

    def refused(P, Qf, N, op):
        before = P.download()
        with pytest.raises(TmHipError):
            lat.bicgstab_complex(P, Qf, 50, 1e-18, 1, N, op=op)
        assert np.array_equal(P.download(), before)

    refused(pf, qf, lat.V, "Mtm_plus_sym_psi")        # FULL fields with an e/o operator
    refused(p, q, lat.Vh, "D_psi")                    # EO fields with the full-lattice operator
    refused(p, q, lat.V, "Mtm_plus_sym_psi")          # N does not match the operator
    refused(pf, qf, lat.Vh, "D_psi")
    refused(p, q, lat.Vh, "Qsw_plus_psi")             # no clover term on this context
    refused(p, q, lat.Vh, "Msw_plus_psi")
    p32, q32 = lat.field32(), lat.field32()           # fp32 is not built
    it = C.c_int(-7)
    assert lat.lib.tmhip_bicgstab_complex(lat.h, p32.h, q32.h, 50, 1e-18, 1, lat.Vh, 7, C.byref(it), None, 0) != 0 and it.value == -7
    for op in (0, 5, 6, 13, -1):                      # cg_her's and cg_mms_tm's operators are not BiCGstab's
        assert lat.lib.tmhip_bicgstab_complex(lat.h, p.h, q.h, 50, 1e-18, 1, lat.Vh, op, C.byref(it), None, 0) != 0 and it.value == -7
    assert lat.lib.tmhip_cg_her(lat.h, p.h, q.h, 10, 1e-20, 0, lat.Vh, 7, C.byref(it), None, 0) != 0    # ... and the other way round
    with pytest.raises(TmHipError):
        lat.assign_add_mul_add_mul(p, q, qf, 1.0, 1.0, lat.Vh)    # fields of two kinds
    with pytest.raises(TmHipError):
        lat.assign_mul_bra_add_mul_ket_add(pf, qf, qf, 1.0, 1.0, lat.Vh)   # FULL fields take N = VOLUME
    with pytest.raises(TmHipError):
        lat.set_option("bicg_fused", 2)
    it_ok, _ = lat.bicgstab_complex(p, q, 1000, 1e-18, 1, lat.Vh, op="Mtm_plus_sym_psi")   # the context still works
    assert it_ok > 0
    lat.set_loopback(True)                            # the single-rank rehearsal of a T-split rank
    refused(p, q, lat.Vh, "Mtm_plus_sym_psi")
    with pytest.raises(TmHipError):
        lat.bicg_pair_dot(p, q, lat.Vh)
    lat.close()
