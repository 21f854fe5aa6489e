"""GPU: the chronological solver guess -- the complex linalg singles, their batched forms, tmhip_chrono_guess on both paths
(option csg_batch) against the reference's outputs (tests/golden/ref_csg_4x4.npz) and the NumPy restatement (tests/csg_restate.py),
the solves it shortens, and the five drop-in symbols.

Lattices: 4^4 (Vh = 128, part of one 1024-site block), 8x6x6x8 (Vh = 1152, one full block and a tail), 8^4 (Vh = 2048, two blocks).
Tolerances: TOL relative to the sum of |terms| for a scalar product, TOL relative to max |field| for an element-wise update, and
cond(G) * TOL for whatever has passed the small solve -- cond(G) from the fixture, or from the restatement where there is none."""
import json
import os

import numpy as np
import pytest

from oracle.nd_restate import cplx, real
from oracle.oraclebind import Oracle
from tests import csg_restate
from tests.hostprog import run_child
from tests.util import TOL, random_gauge, random_spinor, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SHAPES = [(4, 4, 4, 4), (8, 6, 6, 8), (8, 8, 8, 8)]
KAPPA = 0.125


def carr(pairs):
    a = np.asarray(pairs, dtype=np.float64)
    return a[..., 0] + 1j * a[..., 1]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def lat(request):
    from tmlqcd_amd import Lattice
    la = Lattice(*request.param, kappa=KAPPA, mu=0.05)
    yield la
    la.close()


@pytest.fixture(scope="module")
def hosts(lat):
    """21 random fields per lattice, made once"""
    return [random_spinor(500 + k, lat.Vh) for k in range(21)]


# ---- 1. the singles
def test_scalar_prod(lat, hosts):
    S, R = hosts[0], hosts[1]
    fs, fr = lat.field(S), lat.field(R)
    for N in (lat.Vh, lat.Vh - 3, 1):
        zs, zr = cplx(S[:N]), cplx(R[:N])
        got, want = lat.scalar_prod(fs, fr, N), np.vdot(zs, zr)
        print("scalar_prod N %d: |got - want| %.3e, sum |terms| %.3e" % (N, abs(got - want), np.sum(np.abs(zs) * np.abs(zr))))
        assert abs(got - want) <= TOL * np.sum(np.abs(zs) * np.abs(zr))
    assert lat.scalar_prod(fs, fr, 0) == 0
    ss = lat.scalar_prod(fs, fs, lat.Vh)
    assert ss.imag == 0.0
    assert abs(ss.real - lat.square_norm(fs, lat.Vh)) <= TOL * ss.real
    assert lat.scalar_prod(fs, fr, lat.Vh, 1) == lat.scalar_prod(fs, fr, lat.Vh, 0)   # one rank: nothing to add


def test_assign_diff_mul_and_mul(lat, hosts):
    S, R = hosts[2], hosts[3]
    c = 0.7 - 1.3j
    fs, fr = lat.field(S), lat.field(R)
    lat.assign_diff_mul(fr, fs, c, lat.Vh)
    assert rel_err(fr.download(), real(cplx(R) - c * cplx(S))) < TOL
    fr.upload(R)
    N = lat.Vh - 5
    lat.assign_diff_mul(fr, fs, c, N)
    got = fr.download()
    assert rel_err(got[:N], real(cplx(R[:N]) - c * cplx(S[:N]))) < TOL and np.array_equal(got[N:], R[N:])
    lat.assign_diff_mul(fr, fs, c, 0)
    assert np.array_equal(fr.download(), got)
    out = lat.field(R)
    lat.mul(out, c, fs, lat.Vh)
    assert rel_err(out.download(), real(c * cplx(S))) < TOL
    lat.mul(fs, c, fs, lat.Vh)                                     # in place
    assert np.array_equal(fs.download(), out.download())
    lat.mul(fs, 2.0, fs, 0)
    assert np.array_equal(fs.download(), out.download())


# ---- 2. batched products: the bits of the singles
@pytest.mark.parametrize("n", [1, 3, 6, 7, 8, 9, 20])   # 6 | 7: the boundary of a group of the product kernel; 20: the maximum
def test_multi_scalar_prod(lat, hosts, n):
    fs = [lat.field(h) for h in hosts[:n]]
    fr = lat.field(hosts[20])
    for N in (lat.Vh, lat.Vh - 3):
        multi = lat.multi_scalar_prod(fs, fr, N)
        single = np.array([lat.scalar_prod(f, fr, N) for f in fs])
        assert np.array_equal(multi, single)
        assert np.array_equal(multi, lat.multi_scalar_prod(fs, fr, N))
    assert np.array_equal(lat.multi_scalar_prod(fs, fr, 0), np.zeros(n))


# ---- 3. batched updates against the sequence of singles
@pytest.mark.parametrize("n", [1, 5, 20])
def test_multi_assign_diff_mul_and_lincomb(lat, hosts, n):
    rng = np.random.default_rng(77 + n)
    cs = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    fs = lat.field(hosts[20])
    batch, single = [lat.field(h) for h in hosts[:n]], [lat.field(h) for h in hosts[:n]]
    lat.multi_assign_diff_mul(batch, fs, cs, lat.Vh)
    for f, c in zip(single, cs):
        lat.assign_diff_mul(f, fs, c, lat.Vh)
    for i in range(n):
        want = single[i].download()
        assert rel_err(batch[i].download(), want) < TOL, i
        assert rel_err(want, real(cplx(hosts[i]) - cs[i] * cplx(hosts[20]))) < TOL, i
    P, Q = lat.field(hosts[20]), lat.field(hosts[20])
    lat.lincomb(P, batch, cs, lat.Vh)
    lat.mul(Q, cs[n - 1], single[n - 1], lat.Vh)
    for i in range(n - 2, -1, -1):
        lat.assign_add_mul(Q, single[i], cs[i], lat.Vh)
    scale = sum(abs(cs[i]) * np.abs(batch[i].download()).max() for i in range(n))      # the size of the terms that were added up
    assert np.abs(P.download() - Q.download()).max() < TOL * scale


# ---- 4. chrono_guess against the reference's outputs
@pytest.fixture(scope="module")
def gold():
    f = np.load(os.path.join(GOLD, "ref_csg_4x4.npz"))
    s = json.load(open(os.path.join(GOLD, "ref_csg_scalars_4x4.json")))
    return f, s, np.ascontiguousarray(np.load(os.path.join(GOLD, s["gauge_from"]))["gauge"])


@pytest.fixture(scope="module")
def lat4(gold):
    from tmlqcd_amd import Lattice
    f, s, gauge = gold
    la = Lattice(s["T"], s["L"], s["L"], s["L"], kappa=s["kappa"], mu=s["mu"])
    la.set_gauge(gauge)
    yield la
    la.close()


def _guess(la, batch, before, phi, op="Qtm_pm_psi"):
    la.set_option("csg_batch", batch)
    vs = [la.field(np.ascontiguousarray(v)) for v in before]
    trial = la.field(phi)                      # any content: it is overwritten
    G, bn = la.chrono_guess(trial, la.field(phi), vs, op)
    la.set_option("csg_batch", 1)
    return trial.download(), [v.download() for v in vs], G, bn


@pytest.mark.parametrize("n", [1, 2, 5])
def test_chrono_guess_fixture(gold, lat4, n):
    f, s, _ = gold
    c = s["cases"][str(n)]
    bound = c["cond"] * TOL
    Gr, br = carr(c["G"]), carr(c["bn"])
    res = {}
    for batch in (0, 1):
        trial, after, G, bn = res[batch] = _guess(lat4, batch, f["n%d_before" % n], np.ascontiguousarray(f["n%d_phi" % n]))
        errs = {"trial": rel_err(trial, f["n%d_trial" % n]), "history": max(rel_err(after[i], f["n%d_after" % n][i]) for i in range(n)),
                "G": np.abs(G - Gr).max() / np.abs(Gr).max(), "bn": np.abs(bn - br).max() / np.abs(br).max()}
        print("n %d csg_batch %d cond %.3g:" % (n, batch, c["cond"]), errs)
        assert all(e <= bound for e in errs.values()), errs
    assert rel_err(res[0][0], res[1][0]) <= bound
    assert max(rel_err(a, b) for a, b in zip(res[0][1], res[1][1])) <= bound
    assert np.abs(res[0][2] - res[1][2]).max() <= bound * np.abs(Gr).max() and np.abs(res[0][3] - res[1][3]).max() <= bound * np.abs(br).max()


def test_chrono_guess_empty(gold, lat4):
    f = gold[0]
    phi = np.ascontiguousarray(f["n1_phi"])
    for batch in (0, 1):
        lat4.set_option("csg_batch", batch)
        trial = lat4.field(phi)
        G, bn = lat4.chrono_guess(trial, lat4.field(phi), [])
        assert not trial.download().any() and G.shape == (0, 0)
        trial.upload(phi)
        lat4.chrono_guess(trial, lat4.field(phi), [lat4.field(np.ascontiguousarray(f["n1_before"][0]))], N=0)
        assert not trial.download().any()
    lat4.set_option("csg_batch", 1)
    with pytest.raises(Exception):
        lat4.chrono_guess(trial, lat4.field(phi), [trial] * 21)


def test_chrono_guess_restatement_ragged():
    """8x6x6x8 and nine vectors: a full block and a tail, and more vectors than one group of the product kernel holds"""
    from tmlqcd_amd import Lattice
    shape, mu, n = (8, 6, 6, 8), 0.05, 9
    V = int(np.prod(shape))
    gauge = random_gauge(31, V)
    orc = Oracle(*shape, kappa=KAPPA, mu=mu)
    orc.set_gauge(gauge)

    def A(x):
        l = np.zeros((orc.Vh, 4, 3, 2))
        orc.op("Qtm_pm_psi", l, real(x))
        return cplx(l)
    b = csg_restate.rhs_fields(V // 2, n + 1, 99)
    before = [real(csg_restate.normalised(cplx(x))) for x in b[:n]]
    vs = [cplx(v) for v in before]
    trial_r, Gr, br, yr = csg_restate.chrono_guess(A, vs, cplx(b[n]))
    cond = np.linalg.cond(Gr)
    assert cond < 1e4
    bound = cond * TOL
    la = Lattice(*shape, kappa=KAPPA, mu=mu)
    la.set_gauge(gauge)
    for batch in (0, 1):
        trial, after, G, bn = _guess(la, batch, before, b[n])
        errs = {"trial": rel_err(trial, real(trial_r)), "history": max(rel_err(after[i], real(vs[i])) for i in range(n)),
                "G": np.abs(G - Gr).max() / np.abs(Gr).max(), "bn": np.abs(bn - br).max() / np.abs(br).max()}
        print("8x6x6x8 n %d csg_batch %d cond %.3g:" % (n, batch, cond), errs)
        assert all(e <= bound for e in errs.values()), errs
    la.close()


# ---- 5. chrono_add_solution (the rotation of the list is the drop-in's: test_dropin_symbols)
def test_chrono_add_solution(lat, hosts):
    x, slot = lat.field(hosts[4]), lat.field(hosts[5])
    lat.chrono_add_solution(slot, x)
    assert abs(lat.square_norm(slot, lat.Vh) - 1.0) <= TOL
    assert rel_err(slot.download(), hosts[4] / np.sqrt(np.sum(hosts[4] ** 2))) < TOL


# ---- 6. the solves: the monomial's statements for six right-hand sides, the reference's iteration counts
@pytest.mark.parametrize("L", [4, 8])
def test_solve_iterations(gold, L):
    from tmlqcd_amd import Lattice
    s = json.load(open(os.path.join(GOLD, "ref_csg_scalars_%dx%d.json" % (L, L))))
    gauge = gold[2] if L == 4 else random_gauge(s["seed"], L ** 4)
    la = Lattice(L, L, L, L, kappa=s["kappa"], mu=s["mu"])
    la.set_gauge(gauge)
    N = la.Vh
    b = csg_restate.rhs_fields(N, s["nrhs"], s["spinor_seed"])
    slots = [la.field(b[0]) for _ in range(s["csg_N"])]
    idx, n = [-1] * s["csg_N"], 0
    trial, zero = la.field(b[0]), la.field(b[0])
    for k, want in enumerate(s["iters"]):
        phi = la.field(b[k])
        assert n == want["n"]
        G, bn = la.chrono_guess(trial, phi, [slots[j] for j in idx[:n]], s["op"])
        zero.zero()
        it_zero, _ = la.cg_her(zero, phi, s["max_iter"], s["eps_sq"], s["rel_prec"], N, s["op"])
        it_guess, _ = la.cg_her(trial, phi, s["max_iter"], s["eps_sq"], s["rel_prec"], N, s["op"])
        print("%d^4 k %d n %d: from zero %d (reference %d), from the guess %d (reference %d)" % (L, k, n, it_zero, want["zero"], it_guess, want["guess"]))
        assert abs(it_zero - want["zero"]) <= 1 and abs(it_guess - want["guess"]) <= 1
        assert it_guess <= it_zero
        slot, n = csg_restate.add_solution(idx, n, s["csg_N"])
        la.chrono_add_solution(slots[slot], trial)
    la.close()


# ---- 7. the drop-in symbols, in a process of their own
@pytest.mark.parametrize("mode", ["coherent", "resident"])
def test_dropin_symbols(mode):
    out = run_child("csg_dropin_child.py", mode)
    print(out)
    assert out["index_sequence_ok"] and out["zero_trials_ok"]
    assert out["clover_iters"] == out["clover_iters_core"] and len(out["clover_iters"]) == 3
    assert out["bounds"]["linalg"] == TOL and out["bounds"]["guess"] < 1e3 * TOL and out["bounds"]["foreign"] < 1e3 * TOL
    for k, v in out["errs"].items():
        assert v <= out["bounds"][k.split("_")[0]], (k, v)


def test_dropin_refuses_a_list_of_21():
    r = run_child("csg_dropin_child.py", "too_long", check=False)
    assert r.returncode not in (0, -6, -11, 134, 139), (r.returncode, r.stderr[-2000:])
    assert "more than 20 vectors" in r.stderr
