"""GPU: the Wilson gradient flow and the clover field strength on the device-resident links (flow.hip) against the reference's own
outputs (tests/golden/ref_flow_*), against the NumPy restatement (tests/flow_restate.py) on other shapes, as an integrator of third
order, through the measurement loop, and through the drop-in.

Bounds.  They are derived from the deviation of the restatement from the reference that the fixture stores (`restate_vs_ref`,
measured after 6 steps = 18 stages; tests/test_flow_restate.py keeps it from growing):
  links   8 * max(d_link, 2^-50): the factor 8 covers the device's FMA contraction and the different association inside the staple
          sums, the clover leaves and the exponential, over 18 stages.  Any coefficient or ordering mistake in the integrator shows at
          1e-6 or above (5e-7 between eps = 0.01 and 0.005 at t = 0.08 on a 4^4 random field), so the bound must come out below 1e-9,
          which is asserted as well.
  E, P    8 * max(d, 1e-15 * magnitude)
  Q       1e-13 * sum_abs_q, the sum over the sites of |the site's contribution|: the scale rule of the tr-log tests.
Measured on one MI355X (also in the header of profiles/r12_flow_speed.log): on the 4^4 fixture after 6 steps the links differ from the
reference by 2.7e-15 at most (bound 1.7e-14), P by 1.1e-16 (3.2e-15), E by 8.9e-16 (2.1e-14), Q by 2.8e-17 (1.1e-13); on the other
shapes the links by 1.4e-15 at most after 2 steps; the integrator-order ratio is 7.86."""
import json
import os

import numpy as np
import pytest

from tests import flow_restate as fr
from tests import gauge_restate as gr
from tests.hostprog import run_child
from tests.util import random_gauge

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _scalars(tag):
    return json.load(open(os.path.join(GOLD, "ref_flow_scalars_%s.json" % tag)))


class Bounds:
    def __init__(self, s, sum_abs_q=None):
        r = s["restate_vs_ref"]
        self.r = r
        self.link = 8.0 * max(r["d_link"], 2.0 ** -50)
        self.q = 1e-13 * (s["sum_abs_q"] if sum_abs_q is None else sum_abs_q)
        assert self.link < 1e-9

    def e(self, v):
        return 8.0 * max(self.r["d_E"], 1e-15 * abs(v))

    def p(self, v):
        return 8.0 * max(self.r["d_P"], 1e-15 * abs(v))

    def check(self, what, got, want):
        """got / want: (P, E, Q) or (E, Q)"""
        names = ("P", "E", "Q")[-len(got):]
        bd = {"P": self.p, "E": self.e, "Q": lambda v: self.q}
        for n, a, b in zip(names, got, want):
            print("%s %s: gpu %.16e want %.16e |diff| %.3e bound %.3e" % (what, n, a, b, abs(a - b), bd[n](b)))
        for n, a, b in zip(names, got, want):
            assert abs(a - b) <= bd[n](b), (what, n)

    def check_links(self, what, got, want):
        d = float(np.abs(got - want).max())
        print("%s links: max |diff| %.3e bound %.3e" % (what, d, self.link))
        assert d <= self.link, what


@pytest.fixture(scope="module")
def fx4():
    s = _scalars("4x4")
    g = np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"][:256])
    return s, np.load(os.path.join(GOLD, "ref_flow_4x4.npz")), g


def test_against_the_reference_fixtures_4x4(fx4):
    """E, Q of the resident links, P, E, Q after each of six steps at eps = 0.02 and the links after steps 1 and 6 == the reference;
    the resident links are bit-identical before and after."""
    from tmlqcd_amd import Lattice
    s, f, g = fx4
    b = Bounds(s)
    lat = Lattice(4, 4, 4, 4)
    lat.set_gauge(g)
    before = lat.gauge_download()
    b.check("resident", lat.measure_field_strength(), (s["resident"]["E"], s["resident"]["Q"]))
    lat.flow_begin()
    b.check("t = 0", lat.flow_observables(), tuple(s["steps"][0][k] for k in "PEQ"))
    assert np.array_equal(lat.flow_links(), g)
    for n in range(1, s["nsteps"] + 1):
        lat.flow_step(s["eps"])
        b.check("step %d" % n, lat.flow_observables(), tuple(s["steps"][n][k] for k in "PEQ"))
        if n in (1, s["nsteps"]):
            b.check_links("step %d" % n, lat.flow_links(), f["links_step%d" % n])
    lat.flow_end()
    assert np.array_equal(lat.gauge_download(), before) and np.array_equal(before[:256], g)
    lat.close()


def warm_gauge(seed, V, amp=0.4):
    """Links exp(i amp a_k lambda_k) with Gaussian a: different at every site and far from unity, but with a plaquette that does not
    cancel (P about 0.5).  On a hot field P is a sum of O(1) terms that cancels to 1e-3 (7.5e-4 on 2^4) while its rounding error
    stays that of the terms, so the bound on P, which is relative to |P|, says nothing there."""
    u = gr.expm_su3(gr.make_su3(amp * np.random.default_rng(seed).standard_normal((V, 4, 8))))
    return np.ascontiguousarray(np.stack([u.real, u.imag], axis=-1))


@pytest.mark.parametrize("dims", [(4, 6, 2, 10), (2, 2, 2, 2), (6, 4, 4, 4), (8, 6, 4, 12)])
def test_shapes_against_the_restatement(dims, fx4):
    """(4, 6, 2, 10): 480 sites = 7.5 blocks of 64, an extent of 2 where x + mu == x - mu, all extents different; (2, 2, 2, 2): every
    neighbour is the same site twice over; (6, 4, 4, 4): first against the reference's 6x4 scalars on its hot field; (8, 6, 4, 12):
    several blocks per row.  Two steps at eps = 0.03 on warm links as uploaded, then again after an update_gauge on the device: the
    flow starts from the resident links of the moment."""
    from tmlqcd_amd import Lattice
    T, LX, LY, LZ = dims
    V = int(np.prod(dims))
    lat = Lattice(T, LX, LY, LZ)
    if dims == (6, 4, 4, 4):
        s6 = _scalars("6x4")
        b6 = Bounds(s6)
        lat.set_gauge(random_gauge(64, V))
        b6.check("6x4 resident vs reference", lat.measure_field_strength(), (s6["resident"]["E"], s6["resident"]["Q"]))
        lat.flow_begin()
        for n in range(1, s6["nsteps"] + 1):
            lat.flow_step(s6["eps"])
            b6.check("6x4 step %d vs reference" % n, lat.flow_observables(), tuple(s6["steps"][n][k] for k in "PEQ"))
    g = warm_gauge(64, V)
    lat.set_gauge(g)
    eps = 0.03
    for moved in (False, True):
        if moved:
            lat.momenta_upload(np.random.default_rng(8).standard_normal((V, 4, 8)))
            lat.update_gauge(0.05)
            g = np.ascontiguousarray(lat.gauge_download()[:V])
        tag = "%s moved %d" % (dims, moved)
        b = Bounds(fx4[0], fr.sum_abs_q(g, dims))
        want = fr.observables(g, dims)
        b.check(tag + " resident", lat.measure_field_strength(), want[1:])
        lat.flow_begin()                                                       # (a second begin restarts from the resident links)
        b.check(tag + " t = 0", lat.flow_observables(), want)
        gf = g
        for n in (1, 2):
            lat.flow_step(eps)
            gf = fr.step_gradient_flow(gf, dims, eps)
            b.check_links(tag + " step %d" % n, lat.flow_links(), gf)
            b.check(tag + " step %d" % n, lat.flow_observables(), fr.observables(gf, dims))
        assert np.array_equal(lat.gauge_download()[:V], g)
    lat.flow_end()
    lat.close()


def test_integrator_order(fx4):
    """4^4, flow to t = 0.08 with eps = 0.04, 0.02, 0.01: the ratio of successive maximal link differences lies in [6, 10] (third order
    gives 8; the restatement gave 7.6 and 7.7 on such a field), P rises at every step, the flowed links stay unitary to 1e-13."""
    from tmlqcd_amd import Lattice
    V = 256
    lat = Lattice(4, 4, 4, 4)
    lat.set_gauge(random_gauge(64, V))
    ends = []
    for eps, n in ((0.04, 2), (0.02, 4), (0.01, 8)):
        lat.flow_begin()
        p = [lat.flow_observables()[0]]
        for _ in range(n):
            lat.flow_step(eps)
            p.append(lat.flow_observables()[0])
        assert all(b > a for a, b in zip(p, p[1:])), p
        u = lat.flow_links()
        U = u[..., 0] + 1j * u[..., 1]
        dev = float(np.abs(U @ np.conj(np.swapaxes(U, -1, -2)) - np.eye(3)).max())
        det = float(np.abs(np.linalg.det(U) - 1.0).max())
        print("eps %.2f: P %.6f -> %.6f, unitarity %.3e, |det - 1| %.3e" % (eps, p[0], p[-1], dev, det))
        assert dev < 1e-13 and det < 1e-13
        ends.append(u)
    lat.flow_end()
    lat.close()
    d1, d2 = float(np.abs(ends[0] - ends[1]).max()), float(np.abs(ends[1] - ends[2]).max())
    print("link differences %.3e %.3e ratio %.3f" % (d1, d2, d1 / d2))
    assert 6.0 <= d1 / d2 <= 10.0


def test_measurement_loop(fx4):
    """gradient_flow(0.02, 0.1) == the rows of the reference's own loop: as many rows, t bit for bit, the other columns within the
    bounds propagated through the row's arithmetic (W divides the difference of two E by 2 eps); too few rows are refused."""
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    s, _, g = fx4
    b = Bounds(s)
    lat = Lattice(4, 4, 4, 4)
    lat.set_gauge(g)
    rows = lat.gradient_flow(s["eps"], s["tmax"])
    want = np.array(s["rows"])
    assert rows.shape == want.shape
    assert np.array_equal(rows[:, 0], want[:, 0])
    for r, w in zip(rows, want):
        t = w[0]
        bp, be = b.p(w[1]), b.e(w[3])
        bound = np.array([0.0, bp, 36 * bp, be, t * t * 36 * bp, t * t * be, t * t * (2 * be + t * 2 * be / (2 * s["eps"])), b.q])
        bound[1:] += 4 * 2.0 ** -52 * np.abs(w[1:])                            # the row's own arithmetic
        print("t %.2f |diff|" % t, np.abs(r - w), "bound", bound)
        assert (np.abs(r - w) <= bound).all()
    assert np.array_equal(lat.gradient_flow(s["eps"], s["tmax"]), rows)        # and again, bit for bit
    with pytest.raises(TmHipError):
        lat.gradient_flow(s["eps"], s["tmax"], max_rows=len(want) - 1)
    assert np.array_equal(lat.gradient_flow(s["eps"], s["tmax"], max_rows=len(want)), rows)
    assert np.array_equal(lat.gauge_download()[:256], g)
    lat.close()


def test_reproducible_and_refusals(fx4):
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    from tmlqcd_amd.hip import TmHipError
    dims = (4, 6, 2, 10)
    V = int(np.prod(dims))
    lat = Lattice(*dims)
    calls = (lat.measure_field_strength, lat.flow_begin, lambda: lat.flow_step(0.01), lat.flow_observables, lat.flow_links, lat.flow_end,
             lambda: lat.gradient_flow(0.01, 0.02))
    for call in calls:                                                         # no resident links
        with pytest.raises(TmHipError):
            call()
    lat.set_gauge(random_gauge(3, V))
    for call in (lambda: lat.flow_step(0.01), lat.flow_observables, lat.flow_links):   # no flow_begin
        with pytest.raises(TmHipError):
            call()
    runs = []
    for _ in range(2):
        lat.flow_begin()
        obs = []
        for _ in range(3):
            lat.flow_step(0.025)
            obs.append(lat.flow_observables())
        runs.append((lat.flow_links(), obs, lat.measure_field_strength()))
        lat.flow_end()                                                         # flow_end then flow_begin works again
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    with pytest.raises(TmHipError):
        lat.flow_step(0.01)                                                    # ended
    lat.close()
    # a T-split context (one rank of two, the single-process form of the T-slab tests): refused, nothing launched
    T, L = 2, 4
    split = Lattice(T, L, L, L, nproc_t=2, proc_t=0)
    split.set_gauge(syn.gauge_field(16, T, L, L, L, 2, 0))
    for call in (split.measure_field_strength, split.flow_begin, lambda: split.flow_step(0.01), split.flow_observables, split.flow_links,
                 split.flow_end, lambda: split.gradient_flow(0.01, 0.02)):
        with pytest.raises(TmHipError):
            call()
    split.close()
    live = Lattice(4, 4, 4, 4)                                                 # closing a context with a live flow frees its buffers
    live.set_gauge(fx4[2])
    live.flow_begin()
    live.flow_step(0.01)
    live.close()


@pytest.mark.parametrize("mode", ["coherent", "resident"])
def test_through_the_drop_in(mode, tmp_path, fx4):
    """A host program in miniature (tests/flow_dropin_child.py): measure_clover_field_strength_observables(g_gauge_field, &fso) ==
    the fixture; tmlqcd_hip_gradient_flow_measurement(7, 0.02, 0.1) writes gradflow.000007 into the working directory with the
    reference's header byte for byte, t to the printed precision and the other columns within the bounds; in resident mode, after a
    device-side update_gauge, the moved links are the ones measured while the host's stay behind."""
    s = fx4[0]
    b = Bounds(s)
    out = run_child("flow_dropin_child.py", mode, cwd=str(tmp_path))
    print(out)
    b.check("drop-in resident links", (out["E"], out["Q"]), (s["resident"]["E"], s["resident"]["Q"]))
    text = open(os.path.join(str(tmp_path), "gradflow.%06d" % s["traj"])).read()
    ref = s["gradflow_text"]
    assert text.splitlines(True)[0] == ref.splitlines(True)[0] == fr.GRADFLOW_HEADER
    got_lines, ref_lines = text.splitlines(True)[1:], ref.splitlines(True)[1:]
    assert len(got_lines) == len(ref_lines)
    for a, w, row in zip(got_lines, ref_lines, s["rows"]):
        assert a.endswith(" \n") and a.split()[:2] == w.split()[:2]           # traj, and t to the printed precision
        t = row[0]
        bp, be = b.p(row[1]), b.e(row[3])
        bound = np.array([bp, 36 * bp, be, t * t * 36 * bp, t * t * be, t * t * (2 * be + t * 2 * be / (2 * s["eps"])), b.q]) + 1e-12
        assert (np.abs(np.array(a.split()[2:], dtype=float) - np.array(w.split()[2:], dtype=float)) <= bound).all()   # (12 printed digits)
    assert out["host_links_unchanged"] and out["calls_served"] >= 2
    if mode == "resident":
        bm = Bounds(s, out["moved_sum_abs_q"])
        bm.check("drop-in moved links", (out["moved_E"], out["moved_Q"]), (out["moved_want_E"], out["moved_want_Q"]))
        assert abs(out["moved_want_E"] - s["resident"]["E"]) > 1e6 * bm.e(out["moved_want_E"])   # the two fields are told apart
        assert out["moved_calls"] == 1


def test_drop_in_ends_the_program_on_an_unopenable_file(tmp_path):
    """as the reference's fatal_error does: a message and a non-zero exit status, no abort, no fault"""
    r = run_child("flow_dropin_child.py", "unopenable", cwd=str(tmp_path), check=False)
    assert r.returncode not in (0, -6, -11, 134, 139), (r.returncode, r.stderr[-2000:])
    assert "Couldn't open gradflow.000009" in r.stderr and "returned without" not in r.stdout
