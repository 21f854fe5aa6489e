"""CPU: the NumPy restatement of the chronological guess (tests/csg_restate.py) pinned to the reference's own outputs on the 4^4
fixture (tests/golden/ref_csg_4x4.npz, ref_csg_scalars_4x4.json; tools/make_golden_csg.py), the operator taken from the CPU oracle.
Agreement is asked to cond(G) * TOL, cond(G) read from the fixture: the small solve amplifies rounding by that factor."""
import json
import os

import numpy as np
import pytest

from oracle.nd_restate import cplx, real
from oracle.oraclebind import Oracle
from tests import csg_restate
from tests.util import TOL, rel_err

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NS = (1, 2, 5)


def carr(pairs):
    a = np.asarray(pairs, dtype=np.float64)
    return a[..., 0] + 1j * a[..., 1]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "ref_csg_4x4.npz")), json.load(open(os.path.join(GOLD, "ref_csg_scalars_4x4.json")))


@pytest.fixture(scope="module")
def A(fx):
    f, s = fx
    orc = Oracle(s["T"], s["L"], s["L"], s["L"], kappa=s["kappa"], mu=s["mu"])
    orc.set_gauge(np.ascontiguousarray(np.load(os.path.join(GOLD, s["gauge_from"]))["gauge"]))

    def apply(x):
        l = np.zeros((orc.Vh, 4, 3, 2))
        orc.op(s["op"], l, real(x))
        return cplx(l)
    return apply


def test_fixture_sizes_and_coverage(fx):
    f, s = fx
    names = ("ref_csg_4x4.npz", "ref_csg_scalars_4x4.json", "ref_csg_scalars_8x8.json")
    assert sum(os.path.getsize(os.path.join(GOLD, n)) for n in names) < 1 << 20
    assert {"n%d_%s" % (n, w) for n in NS for w in ("phi", "trial", "before", "after")} == set(f.files)
    s8 = json.load(open(os.path.join(GOLD, "ref_csg_scalars_8x8.json")))
    for sc in (s, s8):
        assert set(sc["cases"]) == {str(n) for n in NS}
        for n in NS:
            c = sc["cases"][str(n)]
            assert np.asarray(c["G"]).shape == (n, n, 2) and np.asarray(c["bn"]).shape == (n, 2) and np.asarray(c["y"]).shape == (n, 2)
            assert c["cond"] < 1e3, "right-hand sides that span fewer dimensions than the list make G singular"
            assert 0 < c["iters_guess"] <= c["iters_zero"]
        assert len(sc["add_sequence_N3"]) == 7
    assert s8["mu"] == 0.01 and s["mu"] == 0.05
    for n in NS:
        assert f["n%d_before" % n].shape == (n, 128, 4, 3, 2)
    assert np.array_equal(f["n1_before"], f["n1_after"]) and not np.array_equal(f["n5_before"][:4], f["n5_after"][:4])
    assert np.array_equal(f["n5_before"][4], f["n5_after"][4])          # the newest vector is the pivot and stays


@pytest.mark.parametrize("n", NS)
def test_guess_reproduces_the_reference(fx, A, n):
    f, s = fx
    c = s["cases"][str(n)]
    bound = c["cond"] * TOL
    vs = [cplx(v) for v in f["n%d_before" % n]]
    trial, G, bn, y = csg_restate.chrono_guess(A, vs, cplx(f["n%d_phi" % n]))
    for i in range(n):
        assert rel_err(real(vs[i]), f["n%d_after" % n][i]) < TOL, i
    Gr, br, yr = carr(c["G"]), carr(c["bn"]), carr(c["y"])
    assert np.abs(G - Gr).max() <= TOL * np.abs(Gr).max()
    assert np.abs(bn - br).max() <= TOL * np.abs(br).max()
    assert np.abs(y - yr).max() <= bound * np.abs(yr).max()
    assert rel_err(real(trial), f["n%d_trial" % n]) < bound


@pytest.mark.parametrize("n", NS)
def test_small_solve_alone(fx, n):
    """lu_solve on the reference's G and bn gives the reference's LUSolve output, and numpy's solution, to cond(G) * TOL"""
    c = fx[1]["cases"][str(n)]
    G, bn, yr = carr(c["G"]), carr(c["bn"]), carr(c["y"])
    y = csg_restate.lu_solve(G, bn)
    assert np.abs(y - yr).max() <= c["cond"] * TOL * np.abs(yr).max()
    assert np.abs(y - np.linalg.solve(G, bn)).max() <= c["cond"] * TOL * np.abs(yr).max()
    assert abs(np.linalg.cond(G) - c["cond"]) <= 1e-6 * c["cond"]


def test_small_solve_pivots():
    """a matrix whose rows must change place (the large entry of column 1 sits in the last row), here and in the library's solver"""
    from tmlqcd_amd import hip
    G = np.array([[2.0, 1.0, 0.5], [1.0, 0.5, 3.0], [0.5, 4.0, 1.0]], dtype=np.complex128) * (1 + 0.25j)
    b = np.array([1.0, 2.0 - 1j, 0.5j])
    want = np.linalg.solve(G, b)
    assert np.abs(csg_restate.lu_solve(G, b) - want).max() < np.linalg.cond(G) * TOL
    assert np.abs(hip.csg_solve(G, b) - want).max() < np.linalg.cond(G) * TOL


@pytest.mark.parametrize("n", NS)
def test_library_small_solve(fx, n):
    """tmhip_csg_solve (host code of the library) on the reference's G and bn against the reference's LUSolve output"""
    from tmlqcd_amd import hip
    c = fx[1]["cases"][str(n)]
    yr = carr(c["y"])
    assert np.abs(hip.csg_solve(carr(c["G"]), carr(c["bn"])) - yr).max() <= c["cond"] * TOL * np.abs(yr).max()


def test_index_rotation(fx):
    for sc in (fx[1], json.load(open(os.path.join(GOLD, "ref_csg_scalars_8x8.json")))):
        idx, n = [-1, -1, -1], 0
        for want in sc["add_sequence_N3"]:
            slot, n = csg_restate.add_solution(idx, n, 3)
            assert idx == want["index_array"] and n == want["n"] and slot == idx[n - 1]
    assert csg_restate.add_solution([7], 0, 0) == (None, 0)
    idx = [0]
    assert csg_restate.add_solution(idx, 1, 1) == (0, 1) and idx == [0]
