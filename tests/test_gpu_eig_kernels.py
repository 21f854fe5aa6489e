"""GPU: the three kernels of the eigensolver alone (tmlqcd_amd/csrc/eig.hip) -- tmhip_basis_rotate, tmhip_eig_dots and
tmhip_eig_project -- against NumPy and against the existing single entry points.

Vector lengths: 8 sites per plane (2^4: less than one wave), 48 (4x2x6x2: no multiple of 64) and 4200 (10x10x6x14: a partial
last block of the four-element stream kernels and of the one-element rotation); one segment (an EO field), two (a doublet) and
a FULL field (24 planes).

Bounds.  basis_rotate: an output is a sum of n products added in ascending order, relative error <= 4 n eps of |V| |Y| (n
eps for the sum, the rest headroom for the products), taken against the largest output magnitude; vectors k .. n-1 untouched
bit for bit.  eig_dots: the bits of tmhip_scalar_prod of the same pair (a doublet: of the up value + the down value), and the
same bits on a second call.  eig_project: 4 (j + 1) eps relative in the same sense; its |w|^2 against tmhip_square_norm of the
result to the bound of the trajectory tests' reductions (1e-13 relative, tests.util.TOL).
"""
import numpy as np
import pytest

from tests.util import TOL

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SHAPES = [(2, 2, 2, 2), (4, 2, 6, 2), (10, 10, 6, 14)]
IDS = ["8", "48", "4200"]
NK = [(3, 1), (24, 12), (24, 23), (64, 32), (5, 5)]
NV = [1, 6, 7, 24, 64]


@pytest.fixture(scope="module")
def lats():
    from tmlqcd_amd import Lattice
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Lattice(*shape)
        return made[shape]
    yield get
    for lat in made.values():
        lat.close()


def _host(rng, n, sites):
    return rng.standard_normal((n, sites, 4, 3, 2))


def _c(a):
    return a[..., 0] + 1j * a[..., 1]


def _fields(lat, host, kind):
    return [lat.field(h, kind=kind) for h in host]


def _layout(lat, form):
    """(kind, sites per host array, N of the call) of the three forms"""
    from tmlqcd_amd.hip import FIELD_EO, FIELD_FULL
    return (FIELD_FULL, lat.V, lat.V) if form == "full" else (FIELD_EO, lat.Vh, lat.Vh)


@pytest.mark.parametrize("form", ["eo", "nd", "full"])
@pytest.mark.parametrize("n,k", NK, ids=["%dx%d" % nk for nk in NK])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_basis_rotate(lats, shape, n, k, form):
    lat = lats(shape)
    kind, sites, N = _layout(lat, form)
    rng = np.random.default_rng(100 * n + k + sites)
    nseg = 2 if form == "nd" else 1
    extra = 2                                  # fields of the same basis behind the n that are rotated: "vectors n .. m"
    host = [_host(rng, n + extra, sites) for _ in range(nseg)]
    Y = rng.standard_normal((n, k))
    segs = [_fields(lat, h, kind) for h in host]
    lat.basis_rotate(list(zip(*[s[:n] for s in segs])) if nseg == 2 else segs[0][:n], Y, N)
    try:
        for h, fs in zip(host, segs):
            got = np.stack([f.download() for f in fs])
            want = np.einsum("ik,i...->k...", Y, h[:n])
            scale = np.einsum("ik,i...->k...", np.abs(Y), np.abs(h[:n])).max()
            err = np.abs(got[:k] - want).max() / scale
            print(shape, form, n, k, "relative error / (n eps) =", err / (n * EPS))
            assert err <= 4 * n * EPS
            assert np.array_equal(got[k:], h[k:])          # k .. n-1 and the fields behind them: bit for bit
    finally:
        for fs in segs:
            for f in fs:
                f.free()


@pytest.mark.parametrize("form", ["eo", "nd"])
@pytest.mark.parametrize("nv", NV)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_eig_dots_carry_the_bits_of_scalar_prod(lats, shape, nv, form):
    lat = lats(shape)
    rng = np.random.default_rng(7 * nv + lat.Vh)
    nseg = 2 if form == "nd" else 1
    segs = [_fields(lat, _host(rng, nv, lat.Vh), 0) for _ in range(nseg)]
    w = [lat.field(_host(rng, 1, lat.Vh)[0]) for _ in range(nseg)]
    try:
        vs = list(zip(*segs)) if nseg == 2 else segs[0]
        got = lat.eig_dots(vs, tuple(w) if nseg == 2 else w[0])
        again = lat.eig_dots(vs, tuple(w) if nseg == 2 else w[0])
        assert np.array_equal(got.view(np.float64), again.view(np.float64))
        for i in range(nv):
            parts = [lat.scalar_prod(segs[s][i], w[s], lat.Vh) for s in range(nseg)]
            want = parts[0] if nseg == 1 else complex(parts[0].real + parts[1].real, parts[0].imag + parts[1].imag)
            assert got[i].real == want.real and got[i].imag == want.imag, (i, got[i], want)
    finally:
        for f in [f for fs in segs for f in fs] + w:
            f.free()


def test_eig_dots_on_a_full_field(lats):
    """24 planes in one launch: against NumPy (tmhip_scalar_prod takes one-parity fields), and the same bits twice"""
    lat = lats(SHAPES[1])
    rng = np.random.default_rng(3)
    hv, hw = _host(rng, 7, lat.V), _host(rng, 1, lat.V)[0]
    vs, w = _fields(lat, hv, 1), lat.full_field(hw)
    try:
        got = lat.eig_dots(vs, w, lat.V)
        assert np.array_equal(got.view(np.float64), lat.eig_dots(vs, w, lat.V).view(np.float64))
        for i in range(7):
            want = np.vdot(_c(hv[i]), _c(hw))
            bound = 12 * lat.V * EPS * np.sum(np.abs(_c(hv[i])) * np.abs(_c(hw)))
            assert abs(got[i] - want) <= bound
    finally:
        for f in vs + [w]:
            f.free()


@pytest.mark.parametrize("form", ["eo", "nd", "full"])
@pytest.mark.parametrize("nv", [1, 7, 24, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_eig_project(lats, shape, nv, form):
    lat = lats(shape)
    kind, sites, N = _layout(lat, form)
    rng = np.random.default_rng(11 * nv + sites)
    nseg = 2 if form == "nd" else 1
    hv = [_host(rng, nv, sites) for _ in range(nseg)]
    hw = [_host(rng, 1, sites)[0] for _ in range(nseg)]
    h = (rng.standard_normal(nv) + 1j * rng.standard_normal(nv)) / np.sqrt(nv)
    segs = [_fields(lat, x, kind) for x in hv]
    w = [lat.field(x, kind=kind) for x in hw]
    try:
        vs = list(zip(*segs)) if nseg == 2 else segs[0]
        nrm = lat.eig_project(vs, tuple(w) if nseg == 2 else w[0], h, N)
        total, dev_total = 0.0, 0.0
        for s in range(nseg):
            got = _c(w[s].download())
            want = _c(hw[s]) - np.einsum("i,i...->...", h, _c(hv[s]))
            scale = (np.abs(_c(hw[s])) + np.einsum("i,i...->...", np.abs(h), np.abs(_c(hv[s])))).max()
            err = np.abs(got - want).max() / scale
            print(shape, form, nv, "relative error / ((j + 1) eps) =", err / (nv * EPS))
            assert err <= 4 * nv * EPS
            total += np.vdot(got, got).real
            halves = (w[s].even(), w[s].odd()) if form == "full" else (w[s],)
            dev_total += sum(lat.square_norm(x, lat.Vh) for x in halves)
        assert abs(nrm - dev_total) <= TOL * dev_total
        assert abs(nrm - total) <= TOL * total
    finally:
        for f in [f for fs in segs for f in fs] + w:
            f.free()


def test_pieces_refuse_what_they_cannot_take(lats):
    from tmlqcd_amd.hip import TmHipError
    lat = lats(SHAPES[1])
    rng = np.random.default_rng(5)
    vs = _fields(lat, _host(rng, 3, lat.Vh), 0)
    try:
        with pytest.raises(TmHipError):
            lat.eig_project(vs, vs[1], np.ones(3))              # w is one of the v_i
        with pytest.raises(TmHipError):
            lat.basis_rotate(vs, np.ones((3, 4)))               # k > n
        with pytest.raises(TmHipError):
            lat.basis_rotate([vs[0], vs[0], vs[1]], np.ones((3, 1)))   # the same field twice
        with pytest.raises(TmHipError):
            lat.eig_dots(vs, vs[0], lat.Vh + 1)                 # N past the field
    finally:
        for f in vs:
            f.free()
