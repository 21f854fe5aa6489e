"""CPU: tests/flow_restate.py (the Wilson gradient flow and the clover field strength restated in NumPy) pinned to the reference's
own outputs (tests/golden/ref_flow_*, tools/make_golden_flow.py).

The deviation of the restatement from the reference is MEASURED: d_link is the largest absolute link difference after the six steps
of the fixture, d_E / d_Q / d_P likewise; the generator stored them as `restate_vs_ref`, this test recomputes them and asserts that
they have not grown (twice the stored value or two units in the last place of the quantity, whichever is larger: another libm may
round acos / sin / cos differently).  The GPU tests derive their bounds from these numbers.  Any coefficient or ordering mistake in
the integrator shows at 1e-6 or above, so a d_link above 1e-12 means the restatement is wrong, not the tolerance."""
import json
import os

import numpy as np
import pytest

from tests import flow_restate as fr
from tests import gauge_restate as gr
from tests.util import random_gauge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ULP = 2.0 ** -52


def _load(tag):
    return json.load(open(os.path.join(GOLD, "ref_flow_scalars_%s.json" % tag)))


def _gauge(tag):
    if tag == "4x4":
        return np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"][:256]), (4, 4, 4, 4)
    return random_gauge(64, 6 * 64), (6, 4, 4, 4)


@pytest.fixture(scope="module", params=["4x4", "6x4"])
def flowed(request):
    """(fixture scalars, dims, [links after 0..6 steps of the restatement])"""
    s = _load(request.param)
    g, dims = _gauge(request.param)
    fields = [g]
    for _ in range(s["nsteps"]):
        fields.append(fr.step_gradient_flow(fields[-1], dims, s["eps"]))
    return request.param, s, dims, fields


def test_fixture_sizes_and_content():
    largest = max(os.path.getsize(os.path.join(GOLD, n)) for n in os.listdir(GOLD) if not n.startswith("ref_flow"))
    assert os.path.getsize(os.path.join(GOLD, "ref_flow_4x4.npz")) <= largest
    f = np.load(os.path.join(GOLD, "ref_flow_4x4.npz"))
    assert sorted(f.files) == ["links_step1", "links_step6"] and f["links_step1"].shape == (256, 4, 3, 3, 2)
    for tag in ("4x4", "6x4"):
        s = _load(tag)
        assert (s["eps"], s["nsteps"], s["tmax"], s["traj"]) == (0.02, 6, 0.1, 7) and len(s["steps"]) == 7
        assert s["steps"][0] == s["resident"]
        assert s["gradflow_text"].startswith(fr.GRADFLOW_HEADER) and s["gradflow_text"].count("\n") == 1 + len(s["rows"])
        assert s["restate_vs_ref"]["d_link"] < 1e-12
    assert _load("6x4")["gauge"] == "tests.util.random_gauge(64, V)"


def test_projection():
    m = np.random.default_rng(1).standard_normal((50, 3, 3)) + 1j * np.random.default_rng(2).standard_normal((50, 3, 3))
    p = fr.project_traceless_antiherm(m)
    assert np.array_equal(p, -np.conj(np.swapaxes(p, -1, -2)))                 # anti-hermitian, element for element
    assert np.abs(np.trace(p, axis1=-2, axis2=-1)).max() < 4 * ULP
    want = 0.5 * (m - np.conj(np.swapaxes(m, -1, -2)))                          # note the factor 0.5
    want = want - np.trace(want, axis1=-2, axis2=-1)[:, None, None] / 3.0 * np.eye(3)
    assert np.abs(p - want).max() < 8 * ULP
    assert np.abs(fr.project_traceless_antiherm(p) - p).max() < 4 * ULP       # idempotent


@pytest.mark.parametrize("scale", [0.25, 0.05, 1e-6])
def test_cayley_hamilton_is_the_exponential(scale):
    """== expm_su3 (Taylor, 24 terms) to 1e-14 on random anti-hermitian input of norm <= 1.5 or so (where the Taylor sum itself is good
    to rounding; a flow step has |Z| ~ eps * 6); both signs of c0 and both branches of xi0 occur"""
    A = fr.random_antiherm(3, 400, scale)
    c0 = (1j * np.linalg.det(A)).real
    assert (c0 < 0).any() and (c0 > 0).any()
    e = fr.cayley_hamilton_exponent(A)
    assert np.abs(e - gr.expm_su3(A)).max() < 1e-14
    assert np.abs(e @ np.conj(np.swapaxes(e, -1, -2)) - np.eye(3)).max() < 1e-14


def test_cayley_hamilton_special_cases():
    z = np.zeros((2, 3, 3), dtype=complex)
    assert np.array_equal(fr.cayley_hamilton_exponent(z), np.broadcast_to(np.eye(3, dtype=complex), z.shape))   # c0 == 0 && c1 == 0
    a = np.zeros((1, 3, 3), dtype=complex)                                     # c0 / c0max = 1 up to rounding: the fmin clamp, no NaN
    a[0] = np.diag([1j, 1j, -2j]) * 0.3
    e = fr.cayley_hamilton_exponent(a)
    assert np.isfinite(e).all() and np.abs(e - gr.expm_su3(a)).max() < 1e-14
    e = fr.cayley_hamilton_exponent(-a)                                        # and its c0 < 0 mirror
    assert np.isfinite(e).all() and np.abs(e - gr.expm_su3(-a)).max() < 1e-14


def _grown(now, stored, magnitude):
    return now > max(2.0 * stored, 2.0 * ULP * magnitude)


def test_links_and_scalars_against_the_reference(flowed):
    tag, s, dims, fields = flowed
    d = {"d_link": 0.0, "d_P": 0.0, "d_E": 0.0, "d_Q": 0.0}
    if tag == "4x4":
        f = np.load(os.path.join(GOLD, "ref_flow_4x4.npz"))
        d1 = float(np.abs(fields[1] - f["links_step1"]).max())
        d["d_link"] = float(np.abs(fields[6] - f["links_step6"]).max())
        print("4x4 links: after 1 step %.3e, after 6 steps %.3e" % (d1, d["d_link"]))
        assert d1 <= max(d["d_link"], 8 * ULP)
    per_step = []
    for n, want in enumerate(s["steps"]):
        p, e, q = fr.observables(fields[n], dims)
        per_step.append((abs(p - want["P"]), abs(e - want["E"]), abs(q - want["Q"])))
    d["d_P"], d["d_E"], d["d_Q"] = per_step[-1]
    stored = s["restate_vs_ref"]
    print(tag, "restatement vs reference now", d, "stored", stored)
    assert (d["d_link"] if tag == "4x4" else 0.0) < 1e-12
    if tag == "4x4":
        assert not _grown(d["d_link"], stored["d_link"], 1.0)
    assert not _grown(d["d_P"], stored["d_P"], 1.0)
    assert not _grown(d["d_E"], stored["d_E"], abs(s["steps"][-1]["E"]))
    assert not _grown(d["d_Q"], stored["d_Q"], s["sum_abs_q"])
    for dp, de, dq in per_step:                                                # every step, not only the last
        assert dp <= 8 * ULP and de <= 8 * ULP * abs(s["steps"][-1]["E"]) and dq <= 8 * ULP * s["sum_abs_q"]
    assert abs(fr.sum_abs_q(fields[0], dims) - s["sum_abs_q"]) <= 1e-13 * s["sum_abs_q"]


def test_measurement_loop_against_the_reference(flowed):
    tag, s, dims, fields = flowed
    rows = fr.gradient_flow(fields[0], dims, s["eps"], s["tmax"])
    want = np.array(s["rows"])
    assert rows.shape == want.shape
    assert np.array_equal(rows[:, 0], want[:, 0])                              # t is accumulated, bit for bit
    scale = np.array([1.0, 1.0, 36.0, abs(want[:, 3]).max(), 36.0, 1.0, abs(want[:, 3]).max() / (2 * s["eps"]), s["sum_abs_q"]])
    assert (np.abs(rows - want) <= 16 * ULP * scale).all()
    text = fr.gradflow_text(s["traj"], rows)
    assert text.splitlines()[0] + "\n" == fr.GRADFLOW_HEADER == s["gradflow_text"].splitlines()[0] + "\n"
    assert fr.gradflow_text(s["traj"], want) == s["gradflow_text"]           # the reference's own file, byte for byte
    for a, b in zip(text.splitlines()[1:], s["gradflow_text"].splitlines()[1:]):
        assert a.split()[:2] == b.split()[:2] and a.endswith(" ") and b.endswith(" ")
        assert np.abs(np.array(a.split()[2:], dtype=float) - np.array(b.split()[2:], dtype=float)).max() <= 2e-12


def test_flow_properties_on_an_odd_shape():
    """extent 2 (x + mu == x - mu), all extents different: the plaquette rises, the links stay unitary, and halving the step changes
    the result at third order"""
    dims = (4, 6, 2, 10)
    g = random_gauge(5, int(np.prod(dims)))
    p0 = fr.observables(g, dims)[0]
    g1 = fr.step_gradient_flow(g, dims, 0.04, 2)
    assert fr.observables(g1, dims)[0] > p0
    U = g1[..., 0] + 1j * g1[..., 1]
    assert np.abs(U @ np.conj(np.swapaxes(U, -1, -2)) - np.eye(3)).max() < 1e-13
    g2 = fr.step_gradient_flow(g, dims, 0.02, 4)
    g4 = fr.step_gradient_flow(g, dims, 0.01, 8)
    ratio = np.abs(g1 - g2).max() / np.abs(g2 - g4).max()
    print("order ratio", ratio)
    assert 6.0 <= ratio <= 10.0
