"""CPU: the NumPy restatement of the online measurements (tests/meas_restate.py) against the reference's own values
(tests/golden/ref_meas_scalars_*.json, made by tools/make_golden_meas.py from the reference's files compiled in place).  The GPU
tests compare the device with this restatement on shapes the fixtures do not cover, so it is pinned here first.
Bound throughout: 1e-13 x sum_abs, the sum over sites or lines of the absolute contribution (the scale rule of the tr-log and Q tests)."""
import json
import os

import numpy as np
import pytest

from tests import gauge_restate as gr
from tests import meas_restate as mr
from tests.util import random_gauge, random_spinor

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED_6x4 = 65


def load(tag):
    s = json.load(open(os.path.join(GOLD, "ref_meas_scalars_%s.json" % tag)))
    dims = (s["T"], s["L"], s["L"], s["L"])
    V = int(np.prod(dims))
    if tag == "4x4":
        gauge = np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"][:V])
    else:
        assert s["gauge"] == "tests.util.random_gauge(%d, V)" % SEED_6x4
        gauge = random_gauge(SEED_6x4, V)
    even, odd = random_spinor(s["prop_seeds"][0], V // 2), random_spinor(s["prop_seeds"][1], V // 2)
    return s, dims, gauge, even, odd


@pytest.fixture(scope="module", params=["4x4", "6x4"])
def fx(request):
    return load(request.param)


def test_slice_sums_match_the_reference(fx):
    s, dims, _, even, odd = fx
    for dir_, names in ((0, ("pp", "pa", "p4")), (3, ("pp",))):
        r = mr.slice_sums(even, odd, dims, dir_)
        for k in names:
            want, scale = np.array(s["slices"]["dir%d" % dir_][k]), np.array(s["sum_abs"]["dir%d" % dir_][k])
            assert want.shape == (dims[dir_],)
            assert np.all(np.abs(r[k] - want) <= 1e-13 * scale), (dir_, k, np.abs(r[k] - want), scale)
            assert np.all(np.abs(r["sum_abs_" + k] - scale) <= 1e-13 * scale)
            assert s["restate_vs_ref"]["slices_dir%d" % dir_][k] <= 1e-13 * scale.max()


def test_slice_pp_adds_up_to_the_squared_norm(fx):
    _, dims, _, even, odd = fx
    nrm = float((even ** 2).sum() + (odd ** 2).sum())
    for dir_ in (0, 3):
        r = mr.slice_sums(even, odd, dims, dir_)
        assert abs(r["pp"].sum() - nrm) <= 1e-13 * nrm
        assert np.array_equal(r["pp"], r["sum_abs_pp"])
        assert np.all(np.abs(r["pa"]) <= r["pp"]) and np.all(np.abs(r["p4"]) <= r["pp"])     # term by term, what the GPU bound relies on


def test_one_bilinear_gives_pa_and_p4(fx):
    """pa and p4 are twice the real part and minus twice the imaginary part of B = sum_c conj(psi_c) psi_{c+6}: what the kernel computes once"""
    _, dims, _, even, odd = fx
    psi = mr.eo_to_lexic(even, odd, dims)
    B = (np.conj(psi[..., :2, :]) * psi[..., 2:, :]).sum(axis=(-1, -2))
    _, pa, p4 = mr.site_bilinears(psi)
    assert np.allclose(pa, 2 * B.real, rtol=0, atol=1e-12) and np.allclose(p4, -2 * B.imag, rtol=0, atol=1e-12)


def test_onlinemeas_text_is_rebuilt_byte_for_byte(fx):
    s, dims, _, even, odd = fx
    d0, d3 = s["slices"]["dir0"], s["slices"]["dir3"]
    assert mr.onlinemeas_text(d0["pp"], d0["pa"], d0["p4"], s["t0"], s["kappa"], dims) == s["onlinemeas_text"]
    assert mr.pionnorm_text(d3["pp"], s["z0"], dims) == s["pionnorm_text"]
    # ... and from the restatement's own sums (the file prints six digits)
    r = mr.slice_sums(even, odd, dims, 0)
    assert mr.onlinemeas_text(r["pp"], r["pa"], r["p4"], s["t0"], s["kappa"], dims) == s["onlinemeas_text"]
    assert s["onlinemeas_text"].count("\n") == 3 * (dims[0] // 2 + 1)


def test_polyakov_loop_matches_the_reference(fx):
    s, dims, gauge, _, _ = fx
    for dir_ in range(4):
        v, sa = mr.polyakov_loop(gauge, dims, dir_)
        lines = int(np.prod(dims)) // dims[dir_]
        assert sa == pytest.approx(s["sum_abs"]["polyakov"][str(dir_)], rel=1e-12)
        for key in ("dir%d" % dir_, "loop%d" % dir_):
            if key in s["polyakov"]:
                assert abs(v - complex(*s["polyakov"][key])) <= 1e-13 * sa / (3 * lines), (key, v, s["polyakov"][key])
    assert set(s["polyakov"]) == {"dir0", "dir3", "loop2", "loop3"}
    # the two routines of the reference agree on direction 3, and the files hold what polyakov_loop_dir computed
    assert abs(complex(*s["polyakov"]["dir3"]) - complex(*s["polyakov"]["loop3"])) <= 1e-13 * s["sum_abs"]["polyakov"]["3"]
    for dir_ in (0, 3):
        assert mr.polyakov_line(0, dir_, complex(*s["polyakov"]["dir%d" % dir_])) == s["polyakovloop_dir%d_text" % dir_]


def test_polyakov_loop_of_unit_links_is_one():
    dims = (4, 6, 2, 4)
    g = np.zeros((int(np.prod(dims)), 4, 3, 3, 2))
    for c in range(3):
        g[:, :, c, c, 0] = 1.0
    for dir_ in range(4):
        assert mr.polyakov_loop(g, dims, dir_)[0] == 1.0 + 0.0j


def test_oriented_plaquettes_match_the_reference(fx):
    s, dims, gauge, _, _ = fx
    V = int(np.prod(dims))
    v, sa = mr.oriented_plaquettes(gauge, dims)
    for p in range(6):
        assert sa[p] == pytest.approx(s["sum_abs"]["oriented"][p], rel=1e-12)
        assert abs(v[p] - s["oriented"][p]) <= 1e-13 * sa[p] / (3 * V), (p, v[p], s["oriented"][p])
    assert mr.oriented_line(s["traj"], s["oriented"]) == s["oriented_line"]
    assert mr.oriented_line(s["traj"], v) == s["oriented_line"]


def test_the_six_planes_add_up_to_measure_plaquette(fx):
    """measure_plaquette = sum over planes and sites of Re tr P / 3; a plane of measure_oriented_plaquettes is that / VOLUME"""
    s, dims, gauge, _, _ = fx
    V = int(np.prod(dims))
    v, sa = mr.oriented_plaquettes(gauge, dims)
    assert abs(sum(v) * V - gr.measure_plaquette(gauge, dims)) <= 1e-13 * sum(sa) / 3
    assert abs(sum(s["oriented"]) * V - gr.measure_plaquette(gauge, dims)) <= 1e-13 * sum(sa) / 3
