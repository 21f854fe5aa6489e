"""GPU: the online measurements of meas.hip -- per-slice bilinears of a propagator, Polyakov loop, oriented plaquettes -- against the
reference's own values (tests/golden/ref_meas_scalars_*), against the NumPy restatement (tests/meas_restate.py, pinned to the reference
by tests/test_meas_restate.py) on other shapes, and through the drop-in.

Bounds.
  slice sums   per slice 2 (N + 24) 2^-53 pp[s] for all three quantities, N = LX LY LZ sites per time-slice (dir 0) or T LX LY per
               z-slice (dir 3): the worst case between two summation orders over N sites of 24 non-negative products each, and
               |pa|, |p4| <= pp term by term.
  Polyakov     1e-13 sum_abs / (3 lines), sum_abs = the sum of |tr| over the lines (from the fixture or the restatement)
  plaquettes   1e-13 sum_abs / (3 V) per plane, sum_abs = the sum of |Re tr P| over the sites
Shapes (T, LX, LY, LZ): 4^4 (XYZ/2 = 32: one wave could hold two time-slices of a parity), (6,4,4,4), (6,4,2,6) (V/2 = 144: the site
stride is padded, XYZ/2 = 24), (4,8,8,8) (a time-slice of a parity is exactly one block of 256), (4,12,12,12) (864 = 3.4 blocks per
slice, ragged end; 1728 lines along t), (8,6,6,10) (LZ/2 = 5 in the z decode, 255 of 256 threads per pass of the z-slice kernel).
Measured on one MI355X (also in the header of profiles/r13_meas_speed.log): over all cases the slice sums reach 0.037 of their bound,
the Polyakov loop 6e-4 and the oriented plaquettes 1.3e-3 of theirs."""
import json
import os

import numpy as np
import pytest

from tests import gauge_restate as gr
from tests import meas_restate as mr
from tests.hostprog import last_json, run_child
from tests.util import random_gauge, random_spinor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SEED_6x4 = 65
SHAPES = [(6, 4, 2, 6), (4, 8, 8, 8), (4, 12, 12, 12), (8, 6, 6, 10)]
_cache = {}


def fixture_fields(tag):
    """(scalars, dims, gauge, even, odd) of a reference fixture"""
    if tag not in _cache:
        s = json.load(open(os.path.join(GOLD, "ref_meas_scalars_%s.json" % tag)))
        dims = (s["T"], s["L"], s["L"], s["L"])
        V = int(np.prod(dims))
        if tag == "4x4":
            gauge = np.ascontiguousarray(np.load(os.path.join(GOLD, "ref_fields_4x4.npz"))["gauge"][:V])
        else:
            gauge = random_gauge(SEED_6x4, V)
        _cache[tag] = (s, dims, gauge, random_spinor(s["prop_seeds"][0], V // 2), random_spinor(s["prop_seeds"][1], V // 2))
    return _cache[tag]


def shape_fields(dims):
    """(gauge, even, odd, restated slice sums dir 0 / dir 3) of a shape, computed once"""
    if dims not in _cache:
        V = int(np.prod(dims))
        even, odd = random_spinor(11 + V, V // 2), random_spinor(12 + V, V // 2)
        _cache[dims] = (random_gauge(13 + V, V), even, odd, {0: mr.slice_sums(even, odd, dims, 0), 3: mr.slice_sums(even, odd, dims, 3)})
    return _cache[dims]


def slice_bound(pp, dims, dir_):
    n = int(np.prod(dims)) // dims[dir_]
    return 2.0 * (n + 24) * 2.0 ** -53 * np.asarray(pp)


def check_slices(what, got, want, pp, dims, dir_):
    bound = slice_bound(pp, dims, dir_)
    d = np.abs(np.asarray(got) - np.asarray(want))
    ratio = d[bound > 0] / bound[bound > 0]                                   # (an empty slice has pp = 0 = bound and must give exactly 0)
    print("%s dir %d: max |diff| / bound = %.3f (max |diff| %.3e)" % (what, dir_, float(ratio.max()) if ratio.size else 0.0, float(d.max())))
    assert d.shape == (dims[dir_],) and np.all(d <= bound), (what, dir_, d, bound)


def run_slices(lat, fe, fo, want0, want3, dims, what):
    """both directions, with pa / p4 and without, against the given sums"""
    pp, pa, p4 = lat.slice_correlators(fe, fo, 0)
    for k, v in (("pp", pp), ("pa", pa), ("p4", p4)):
        check_slices(what + " " + k, v, want0[k], want0["pp"], dims, 0)
    check_slices(what + " pp alone", lat.slice_correlators(fe, fo, 0, pa_p4=False), want0["pp"], want0["pp"], dims, 0)
    pz, paz, p4z = lat.slice_correlators(fe, fo, 3)
    check_slices(what + " pp", pz, want3["pp"], want3["pp"], dims, 3)
    check_slices(what + " pp alone", lat.slice_correlators(fe, fo, dir=3, pa_p4=False), want3["pp"], want3["pp"], dims, 3)
    if "pa" in want3:
        check_slices(what + " pa", paz, want3["pa"], want3["pp"], dims, 3)
        check_slices(what + " p4", p4z, want3["p4"], want3["pp"], dims, 3)
    return pp, pa, p4, pz


@pytest.mark.parametrize("tag", ["4x4", "6x4"])
def test_slice_sums_against_the_reference(tag):
    from tmlqcd_amd import Lattice
    s, dims, _, even, odd = fixture_fields(tag)
    lat = Lattice(*dims)
    fe, fo = lat.field(even), lat.field(odd)
    run_slices(lat, fe, fo, s["slices"]["dir0"], s["slices"]["dir3"], dims, tag + " vs reference")
    lat.close()


@pytest.mark.parametrize("dims", SHAPES)
def test_slice_sums_against_the_restatement(dims):
    from tmlqcd_amd import Lattice
    _, even, odd, want = shape_fields(dims)
    lat = Lattice(*dims)
    fe, fo = lat.field(even), lat.field(odd)
    run_slices(lat, fe, fo, want[0], want[3], dims, "%s vs restatement" % (dims,))
    lat.close()


def test_slice_sums_properties():
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import FIELD_FULL, TmHipError
    dims = (8, 6, 6, 10)
    T, LX, LY, LZ = dims
    V = int(np.prod(dims))
    _, even, odd, want = shape_fields(dims)
    lat = Lattice(*dims)
    fe, fo = lat.field(even), lat.field(odd)
    # two calls agree bit for bit
    a, b = lat.slice_correlators(fe, fo, 0), lat.slice_correlators(fe, fo, 0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    a, b = lat.slice_correlators(fe, fo, 3), lat.slice_correlators(fe, fo, 3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # sum_s pp[s] == |even|^2 + |odd|^2: the same V x 24 non-negative products in another order
    nrm = lat.square_norm(fe, V // 2) + lat.square_norm(fo, V // 2)
    for dir_ in (0, 3):
        tot = float(lat.slice_correlators(fe, fo, dir_, pa_p4=False).sum())
        print("dir %d: sum pp %.16e norms %.16e" % (dir_, tot, nrm))
        assert abs(tot - nrm) <= 2.0 * (V + 24) * 2.0 ** -53 * nrm
    # a field that lives on one time-slice and one z-slice only: exact zeros everywhere else
    t1, z1 = 5, 7
    lex = np.zeros((T, LX, LY, LZ, 4, 3, 2))
    lex[t1, :, :, z1] = random_spinor(99, LX * LY).reshape(LX, LY, 4, 3, 2)
    e1, o1 = mr.split_eo(lex, dims)
    g0, g3 = mr.slice_sums(e1, o1, dims, 0), mr.slice_sums(e1, o1, dims, 3)
    f1e, f1o = lat.field(e1), lat.field(o1)
    pp, pa, p4, pz = run_slices(lat, f1e, f1o, g0, g3, dims, "one slice")
    for v, keep in ((pp, t1), (pa, t1), (p4, t1), (pz, z1)):
        assert v[keep] != 0.0 and np.all(np.delete(v, keep) == 0.0), v
    # refusals: fp32 field, FULL field, a direction that is neither t nor z
    f32 = lat.field32(even.astype(np.float32))
    full = lat.full_field()
    for args in ((f32, fo, 0), (fe, f32, 3), (full, fo, 0), (fe, fo, 1), (fe, fo, 2), (fe, fo, -1)):
        with pytest.raises(TmHipError):
            lat.slice_correlators(*args)
    assert full.kind == FIELD_FULL
    # ... and a refused call leaves the next one intact
    check_slices("after refusals pp", lat.slice_correlators(fe, fo, 0)[0], want[0]["pp"], want[0]["pp"], dims, 0)
    lat.close()


@pytest.mark.parametrize("mode", [1, 3])
def test_slice_sums_on_a_looped_back_context(mode):
    """the multi-GPU code path on one GPU (tmhip_comm_set_loopback): the sums are site-local and are not refused"""
    from tmlqcd_amd import Lattice
    dims = (6, 4, 2, 6)
    _, even, odd, want = shape_fields(dims)
    lat = Lattice(*dims)
    lat.set_gauge(random_gauge(5, int(np.prod(dims))))
    lat.set_loopback(mode)
    try:
        fe, fo, tmp = lat.field(even), lat.field(odd), lat.field()
        lat.Hopping_Matrix(0, tmp, fo)                                        # a split-phase stencil has run on this context
        run_slices(lat, fe, fo, want[0], want[3], dims, "loopback %d" % mode)
        lat.sync()
    finally:
        lat.set_loopback(0)
    lat.close()


def test_slice_sums_on_a_t_split_rank():
    """one rank of two along T (the single-process form of the T-slab tests): its local T time-slices, its share of every z-slice"""
    from tmlqcd_amd import Lattice
    dims = (4, 8, 8, 8)
    _, even, odd, want = shape_fields(dims)
    lex = np.zeros((int(np.prod(dims)), 4, 3, 2))
    t, x, y, z = np.unravel_index(np.arange(lex.shape[0]), dims)
    par = (t + x + y + z) & 1
    lex[par == 0], lex[par == 1] = even, odd
    half = (2,) + dims[1:]
    tot3 = np.zeros(dims[3])
    for proc_t in (0, 1):
        loc = lex.reshape(dims + (4, 3, 2))[2 * proc_t:2 * proc_t + 2]
        e, o = mr.split_eo(loc, half)
        w0, w3 = mr.slice_sums(e, o, half, 0), mr.slice_sums(e, o, half, 3)
        lat = Lattice(*half, nproc_t=2, proc_t=proc_t)
        fe, fo = lat.field(e), lat.field(o)
        pp, pa, p4, pz = run_slices(lat, fe, fo, w0, w3, half, "rank %d of 2" % proc_t)
        check_slices("rank %d local slices vs the unsplit lattice" % proc_t, pp, want[0]["pp"][2 * proc_t:2 * proc_t + 2],
                     want[0]["pp"][2 * proc_t:2 * proc_t + 2], half, 0)
        tot3 += pz
        lat.close()
    check_slices("z-slices added over the ranks", tot3, want[3]["pp"], want[3]["pp"], dims, 3)


# ------------------------------------------------------------------------------------------------ Polyakov loop
def check_polyakov(what, got, want, sum_abs, lines):
    bound = 1e-13 * sum_abs / (3 * lines)
    print("%s: gpu %r want %r |diff| %.3e bound %.3e" % (what, got, want, abs(got - want), bound))
    assert abs(got - want) <= bound, what
    return bound


@pytest.mark.parametrize("tag", ["4x4", "6x4"])
def test_polyakov_loop_against_the_reference(tag):
    from tmlqcd_amd import Lattice
    s, dims, gauge, _, _ = fixture_fields(tag)
    V = int(np.prod(dims))
    lat = Lattice(*dims)
    lat.set_gauge(gauge)
    for dir_ in range(4):
        got = lat.polyakov_loop(dir_)
        lines = V // dims[dir_]
        for key in ("dir%d" % dir_, "loop%d" % dir_):
            if key in s["polyakov"]:
                check_polyakov("%s %s vs reference" % (tag, key), got, complex(*s["polyakov"][key]), s["sum_abs"]["polyakov"][str(dir_)], lines)
        v, sa = mr.polyakov_loop(gauge, dims, dir_)
        check_polyakov("%s dir %d vs restatement" % (tag, dir_), got, v, sa, lines)
        assert lat.polyakov_loop(dir_) == got                                  # bit-identical on a second call
    lat.close()


@pytest.mark.parametrize("dims", [(4, 12, 12, 12), (8, 6, 6, 10)])
def test_polyakov_loop_shapes_and_moved_links(dims):
    """all four directions against the restatement; then, after an update_gauge on the device and without a download in between, the
    moved links are the ones measured"""
    from tmlqcd_amd import Lattice
    V = int(np.prod(dims))
    g = shape_fields(dims)[0]
    lat = Lattice(*dims)
    lat.set_gauge(g)
    before = {}
    for dir_ in range(4):
        v, sa = mr.polyakov_loop(g, dims, dir_)
        before[dir_] = lat.polyakov_loop(dir_)
        check_polyakov("%s dir %d" % (dims, dir_), before[dir_], v, sa, V // dims[dir_])
    lat.momenta_upload(np.random.default_rng(8).standard_normal((V, 4, 8)))
    lat.update_gauge(0.05)
    after = {dir_: lat.polyakov_loop(dir_) for dir_ in range(4)}
    moved = np.ascontiguousarray(lat.gauge_download()[:V])
    for dir_ in range(4):
        v, sa = mr.polyakov_loop(moved, dims, dir_)
        bound = check_polyakov("%s dir %d moved" % (dims, dir_), after[dir_], v, sa, V // dims[dir_])
        assert abs(after[dir_] - before[dir_]) > 1e6 * bound
    lat.close()


def test_polyakov_loop_unit_links_and_refusals():
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    from tmlqcd_amd.hip import TmHipError
    dims = (6, 4, 2, 6)
    V = int(np.prod(dims))
    lat = Lattice(*dims)
    with pytest.raises(TmHipError):
        lat.polyakov_loop(0)                                                   # no resident links
    unit = np.zeros((V, 4, 3, 3, 2))
    for c in range(3):
        unit[:, :, c, c, 0] = 1.0
    lat.set_gauge(unit)
    for dir_ in (0, 1, 3):
        assert lat.polyakov_loop(dir_) == 1.0 + 0.0j
    for dir_ in (2, 4, -1):                                                    # an extent of 2; no such direction
        with pytest.raises(TmHipError):
            lat.polyakov_loop(dir_)
    assert lat.polyakov_loop(3) == 1.0 + 0.0j
    lat.close()
    T, L = 4, 4
    split = Lattice(T, L, L, L, nproc_t=2, proc_t=0)
    split.set_gauge(syn.gauge_field(16, T, L, L, L, 2, 0))
    for call in (lambda: split.polyakov_loop(3), split.measure_oriented_plaquettes):
        with pytest.raises(TmHipError):
            call()
    split.close()


# ------------------------------------------------------------------------------------------------ oriented plaquettes
def check_oriented(what, lat, g, dims, ref=None, ref_sum_abs=None):
    V = int(np.prod(dims))
    got = lat.measure_oriented_plaquettes()
    want, sa = mr.oriented_plaquettes(g, dims)
    for p in range(6):
        for tag, w, scale in (("restatement", want[p], sa[p]),) + ((("reference", ref[p], ref_sum_abs[p]),) if ref else ()):
            bound = 1e-13 * scale / (3 * V)
            print("%s plane %d vs %s: gpu %.16e want %.16e |diff| %.3e bound %.3e" % (what, p, tag, got[p], w, abs(got[p] - w), bound))
            assert abs(got[p] - w) <= bound, (what, p, tag)
    # the six planes add up to measure_plaquette: sum over planes and sites of Re tr P / 3 there, / (3 V) per plane here
    total = lat.measure_plaquette()
    print("%s: V sum(planes) %.16e measure_plaquette %.16e" % (what, V * sum(got), total))
    assert abs(V * sum(got) - total) <= 1e-13 * sum(sa) / 3
    assert lat.measure_oriented_plaquettes() == got                            # bit-identical on a second call
    return got


@pytest.mark.parametrize("tag", ["4x4", "6x4"])
def test_oriented_plaquettes_against_the_reference(tag):
    from tmlqcd_amd import Lattice
    s, dims, gauge, _, _ = fixture_fields(tag)
    lat = Lattice(*dims)
    lat.set_gauge(gauge)
    check_oriented(tag, lat, gauge, dims, s["oriented"], s["sum_abs"]["oriented"])
    lat.close()


@pytest.mark.parametrize("dims", SHAPES)
def test_oriented_plaquettes_shapes(dims):
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    g = shape_fields(dims)[0]
    lat = Lattice(*dims)
    with pytest.raises(TmHipError):
        lat.measure_oriented_plaquettes()                                      # no resident links
    lat.set_gauge(g)
    check_oriented("%s" % (dims,), lat, g, dims)
    lat.close()


# ------------------------------------------------------------------------------------------------ drop-in
def _child(mode, cwd):
    return run_child("meas_dropin_child.py", mode, cwd=str(cwd), check=False)      # (the tests read its stderr too)


@pytest.mark.parametrize("mode", ["coherent", "resident"])
def test_through_the_drop_in(mode, tmp_path):
    """A host program in miniature (tests/meas_dropin_child.py) on the 4^4 fixture: the raw sums of tmlqcd_hip_slice_correlators on host
    spinors, the onlinemeas text rebuilt from them (six printed digits: equality of the text), two appended lines of
    oriented_plaquettes_measurement, the two-line file of tmlqcd_hip_polyakov_loop_dir(0, 0) then (1, 0), and -1 for dir 1."""
    s, dims, gauge, _, _ = fixture_fields("4x4")
    V = int(np.prod(dims))
    r = _child(mode, tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    out = last_json(r)
    print(out)
    d0, d3 = s["slices"]["dir0"], s["slices"]["dir3"]
    for k in ("pp", "pa", "p4"):
        check_slices("drop-in " + k, out[k], d0[k], d0["pp"], dims, 0)
    check_slices("drop-in pp", out["pz"], d3["pp"], d3["pp"], dims, 3)
    assert out["slices_repeat"]
    assert mr.onlinemeas_text(out["pp"], out["pa"], out["p4"], s["t0"], s["kappa"], dims) == s["onlinemeas_text"]
    assert mr.pionnorm_text(out["pz"], s["z0"], dims) == s["pionnorm_text"]
    # oriented plaquettes: the fixture's line, then a second one
    lines = open(os.path.join(str(tmp_path), "oriented_plaquettes.data")).read().splitlines(True)
    assert len(lines) == 2 and lines[0] == s["oriented_line"]
    assert lines[1] == mr.oriented_line(s["traj"] + 1, s["oriented"])
    for p in range(6):
        assert abs(out["oriented"][p] - s["oriented"][p]) <= 1e-13 * s["sum_abs"]["oriented"][p] / (3 * V)
    # Polyakov loop: return values, the two-line file of direction 0, the one-line file of direction 3, none for direction 1
    assert out["rc"] == [0, 0, 0, -1] and "Wrong direction" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path), "polyakovloop_dir1"))
    for dir_, n in ((0, 2), (3, 1)):
        text = open(os.path.join(str(tmp_path), "polyakovloop_dir%d" % dir_)).read().splitlines(True)
        ref = s["polyakovloop_dir%d_text" % dir_]
        assert len(text) == n
        f, w = text[0].split(), ref.split()
        assert f[:2] == w[:2] and len(text[0]) == len(ref) and text[0].count("\t") == 3
        bound = 1e-13 * s["sum_abs"]["polyakov"][str(dir_)] / (3 * (V // dims[dir_]))
        assert abs(complex(float(f[2]), float(f[3])) - complex(float(w[2]), float(w[3]))) <= bound      # (the 16 printed digits)
        if n == 2:
            assert text[1].split()[:2] == ["1", "0"] and text[1].split()[2:] == f[2:]
    for dir_ in range(4):
        v, sa = mr.polyakov_loop(gauge, dims, dir_)
        check_polyakov("drop-in dir %d" % dir_, complex(*out["polyakov"][dir_]), v, sa, V // dims[dir_])
    assert out["calls_served"] >= 12


def test_drop_in_on_unopenable_files(tmp_path):
    """a directory in the place of the output file: oriented_plaquettes_measurement ends the program with the reference's message (as
    fatal_error does: a non-zero exit status, no abort, no fault), tmlqcd_hip_polyakov_loop_dir prints its message and returns -1"""
    a = tmp_path / "a"
    a.mkdir()
    r = _child("unopenable_oriented", a)
    assert r.returncode not in (0, -6, -11, 134, 139), (r.returncode, r.stderr[-2000:])
    assert "Couldn't open oriented_plaquettes.data for appending during measurement 3!" in r.stderr and "returned without" not in r.stdout
    b = tmp_path / "b"
    b.mkdir()
    r = _child("unopenable_polyakov", b)
    assert r.returncode == 0, r.stderr[-2000:]
    assert last_json(r) == {"rc": -1}
    assert "Could not open file polyakovloop_dir3 for writing" in r.stderr
