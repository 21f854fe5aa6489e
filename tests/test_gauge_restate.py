"""CPU: tests/gauge_restate.py (the gauge monomial restated in NumPy) pinned to the reference's own outputs
(tests/golden/ref_gauge_*, tools/make_golden_gauge.py), and -- independent of any fixture -- its force checked to be the derivative
of its action."""
import json
import os

import numpy as np
import pytest

from tests import gauge_restate as gr
from tests.util import TOL, random_gauge, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ["wilson", "iwasaki", "em_wilson", "em_iwasaki"]


@pytest.fixture(scope="module")
def fx4():
    return (np.load(os.path.join(GOLD, "ref_gauge_4x4.npz")), json.load(open(os.path.join(GOLD, "ref_gauge_scalars_4x4.json"))),
            np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"])


def test_fixture_sizes_and_coverage(fx4):
    f, s, _ = fx4
    assert sum(os.path.getsize(os.path.join(GOLD, n)) for n in ("ref_gauge_4x4.npz", "ref_gauge_scalars_4x4.json", "ref_gauge_scalars_6x4.json")) < 1 << 20
    assert sorted(f.files) == sorted(CASES)
    c = s["cases"]
    assert c["iwasaki"]["c1"] == -0.331 and abs(c["iwasaki"]["c0"] - (1 + 8 * 0.331)) < 1e-15 and c["iwasaki"]["use_rectangles"] == 1
    assert c["em_wilson"]["glambda"] == 0.3 and c["em_iwasaki"]["glambda"] == 0.3 and s["beta"] == 6.0
    assert s["plaquetteEnergy_after_lambda"] == s["measure_gauge_action_lambda"]      # measure_gauge_action.c:187


def _scalars_match(s, g, dims):
    V = int(np.prod(dims))
    bound6, bound12 = TOL * 6 * V, TOL * 12 * V          # every term is at most 1 after the / 3
    assert abs(gr.measure_plaquette(g, dims) - s["measure_plaquette"]) <= bound6
    assert abs(gr.measure_gauge_action(g, dims, 0.0) - s["measure_gauge_action_0"]) <= bound6
    assert abs(gr.measure_gauge_action(g, dims, s["lambda"]) - s["measure_gauge_action_lambda"]) <= bound6 * (1 + s["lambda"])
    assert abs(gr.measure_rectangles(g, dims) - s["measure_rectangles"]) <= bound12
    for name, c in s["cases"].items():
        e = gr.gauge_energy(g, dims, s["beta"], c["c0"], c["c1"], bool(c["use_rectangles"]), c["glambda"])
        assert abs(e - c["energy0"]) <= s["beta"] * (abs(c["c0"]) * bound6 * (1 + c["glambda"]) + abs(c["c1"]) * bound12), name


def test_scalars_4x4(fx4):
    f, s, g = fx4
    _scalars_match(s, g, (4, 4, 4, 4))


@pytest.mark.parametrize("name", CASES)
def test_derivative_4x4(fx4, name):
    f, s, g = fx4
    c = s["cases"][name]
    V = 256
    d = gr.seed_derivative(V) + gr.gauge_derivative(g, (4, 4, 4, 4), s["beta"], c["c0"], c["c1"], bool(c["use_rectangles"]), c["glambda"])
    assert rel_err(d, f[name]) < TOL


def test_non_hypercubic_6x4():
    s = json.load(open(os.path.join(GOLD, "ref_gauge_scalars_6x4.json")))
    dims = (6, 4, 4, 4)
    V = 6 * 64
    g = random_gauge(64, V)
    assert s["gauge"] == "tests.util.random_gauge(64, V)"
    _scalars_match(s, g, dims)
    for name, c in s["cases"].items():
        d = gr.seed_derivative(V) + gr.gauge_derivative(g, dims, s["beta"], c["c0"], c["c1"], bool(c["use_rectangles"]), c["glambda"])
        got, want = gr.checksums(d), c["checksums"]
        scale = float(np.abs(d).max()) * d.size       # each checksum is a sum of d.size terms of at most this size (the weights are O(1..4))
        for k in want:
            assert abs(got[k] - want[k]) <= TOL * scale * (scale / d.size if k == "sum_sq" else 4.0), (name, k)


def test_t_slab_view_is_the_slice_of_the_full_result():
    dims = (6, 2, 4, 2)
    V = int(np.prod(dims))
    g = random_gauge(5, V)
    full = gr.gauge_derivative(g, dims, 5.5, glambda=0.1)
    XYZ = 16
    parts = [gr.gauge_derivative(g, dims, 5.5, glambda=0.1, t_slab=(2 * r, 2 * r + 2)) for r in range(3)]
    assert np.array_equal(np.concatenate(parts), full)
    assert all(p.shape == (2 * XYZ, 4, 8) for p in parts)
    tot = sum(gr.measure_gauge_action(g, dims, 0.1, t_slab=(2 * r, 2 * r + 2)) for r in range(3))
    assert abs(tot - gr.measure_gauge_action(g, dims, 0.1)) <= TOL * 6 * V


LAMBDA = [np.array(m, dtype=complex) for m in (
    [[0, 1, 0], [1, 0, 0], [0, 0, 0]], [[0, -1j, 0], [1j, 0, 0], [0, 0, 0]], [[1, 0, 0], [0, -1, 0], [0, 0, 0]],
    [[0, 0, 1], [0, 0, 0], [1, 0, 0]], [[0, 0, -1j], [0, 0, 0], [1j, 0, 0]], [[0, 0, 0], [0, 0, 1], [0, 1, 0]],
    [[0, 0, 0], [0, 0, -1j], [0, 1j, 0]], np.diag([1, 1, -2]) / np.sqrt(3.0))]


@pytest.mark.parametrize("dims", [(4, 4, 4, 4), (4, 2, 6, 2)])
@pytest.mark.parametrize("rect", [False, True])
def test_force_is_the_derivative_of_the_action(dims, rect):
    """update_gauge moves a link as U <- exp(step * _make_su3(P)) U with _make_su3(P) = i sum_a P_a lambda_a, and update_momenta takes
    P_a -= step * derivative_a; H = P^2 / 2 - E with E = gauge_energy (gauge_acc returns E_old - E_new as its part of dH) is conserved
    when derivative_a = -d/d eps E(exp(i eps lambda_a) U).  Central difference, step eps:
      truncation <= eps^2 / 6 * max |f'''|, f''' = sum over the loops through the link of beta c Re tr(X^3 ...) / 3 with
                    |tr(X^3 W)| <= ||lambda_a||^3 * 3 for unitary W and ||lambda_a|| <= 2 / sqrt(3) (a = 8): 6 plaquettes weighted
                    c0 (1 + |lambda|), 18 rectangles weighted |c1|.  That counts a loop that holds the link ONCE.  Where an extent is 2
                    a rectangle whose long side lies in that direction returns to its start after two steps and holds the link
                    twice (as U and as U^dagger); it is then quadratic in exp(eps X) and its third derivative has 2^3 = 8 terms of
                    the single-link size.  On such a lattice every loop count is taken times 8 (more than needed, but a bound)
      rounding   <= 4 * 2^-52 * (bound on |E|) / eps: E is a sum of 6 V (12 V) terms of at most beta c0 (beta |c1|)
    With eps = 1e-4 both are a few 1e-8 to 1e-6 next to derivative entries of order 10."""
    rng = np.random.default_rng(11)
    V = int(np.prod(dims))
    g = random_gauge(3, V)
    beta, lam = 5.7, 0.2
    c1 = -0.331 if rect else 0.0
    c0 = 1.0 - 8.0 * c1 if rect else 1.0
    eps = 1.0e-4
    d = gr.gauge_derivative(g, dims, beta, c0, c1, rect, lam)
    norm3 = (2.0 / np.sqrt(3.0)) ** 3
    twice = 8.0 if min(dims) == 2 else 1.0
    bound = eps ** 2 / 6.0 * beta * twice * (6 * c0 * (1 + lam) + 18 * abs(c1)) * norm3 \
        + 4 * 2.0 ** -52 * beta * (c0 * (1 + lam) * 6 * V + abs(c1) * 12 * V) / eps
    assert bound < 1e-5      # (the derivative entries are of order 10)
    U = g[..., 0] + 1j * g[..., 1]
    for _ in range(4):
        ix, mu, a = int(rng.integers(V)), int(rng.integers(4)), int(rng.integers(8))
        e = []
        for sgn in (+1, -1):
            w, v = np.linalg.eigh(LAMBDA[a])
            rot = (v * np.exp(1j * sgn * eps * w)) @ v.conj().T
            U2 = U.copy()
            U2[ix, mu] = rot @ U[ix, mu]
            g2 = np.stack([U2.real, U2.imag], axis=-1)
            e.append(gr.gauge_energy(g2, dims, beta, c0, c1, rect, lam))
        fd = (e[0] - e[1]) / (2 * eps)
        assert abs(-fd - d[ix, mu, a]) <= bound, (ix, mu, a, fd, d[ix, mu, a], bound)
