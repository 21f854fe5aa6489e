"""GPU: the 3D Laplacian on colour vectors (tmhip_laph_apply and its reducing and filter forms) and the batched Lanczos pieces
(tmhip_laph_dots / _project / _normalise / _rotate) of tmlqcd_amd/csrc/laph.hip.

Shapes (T, LX, LY, LZ): (2,2,2,2) every extent 2, x+mu and x-mu one site, 8 sites per slice (less than a wave); (4,2,6,2) 24 sites;
(6,10,2,4) 80 sites, more than a wave, no multiple of 64; (4,4,4,16) 256 sites, one full block; (10,10,6,14) 840 sites, four blocks
with a partial last wave.  The golden outputs are the reference's object code on 4^4 and 8x6x4x12 (tools/make_golden_laph.py).

Bounds.  The operator, all forms: tests.util.TOL (1e-13, max |difference| / max |reference|).  The per-slice <in, out> and the dots:
a sum of N = 3 SPACEVOLUME products, |error| <= N eps |v| |w|.  Projection: nv + 1 terms per element, 4 (nv + 1) eps relative to the
largest magnitude involved; its |w|^2 and the norms: N eps relative.  Rotation: 4 n eps of |Y| |V| per element.  A frozen slice stays
as it was bit for bit, and a second call gives the same bits.
"""
import numpy as np
import pytest

from tests import laph_restate as lr
from tests.util import TOL, random_gauge, rel_err

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SHAPES = [(2, 2, 2, 2), (4, 2, 6, 2), (6, 10, 2, 4), (4, 4, 4, 16), (10, 10, 6, 14)]
IDS = ["x".join(str(d) for d in s) for s in SHAPES]
GOLDEN = {"4x4": (4, 4, 4, 4), "8x6x4x12": (8, 6, 4, 12)}


@pytest.fixture(scope="module")
def lats():
    from tmlqcd_amd import Lattice
    made = {}

    def get(shape, seed=11):
        if shape not in made:
            lat = Lattice(*shape)
            g = random_gauge(seed, lat.V)
            lat.set_gauge(g)
            made[shape] = (lat, g)
        return made[shape]
    yield get
    for lat, _ in made.values():
        lat.close()


def _field(rng, lat):
    return rng.standard_normal((lat.T, lat.V // lat.T, 3, 2))


@pytest.mark.parametrize("tag", sorted(GOLDEN))
def test_apply_matches_the_reference_object_code(tag):
    import os
    from tmlqcd_amd import Lattice
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = np.load(os.path.join(gold, "ref_laph_%s.npz" % tag))
    dims = GOLDEN[tag]
    V = int(np.prod(dims))
    g = np.load(os.path.join(gold, "ref_mms_4x4.npz"))["gauge"][:V] if tag == "4x4" else random_gauge(123456, V)
    lat = Lattice(*dims)
    try:
        lat.set_gauge(np.ascontiguousarray(g))
        k, l = lat.cvfield(z["k"]), lat.cvfield()
        lat.laph_apply(l, k)
        assert np.array_equal(k.download(), z["k"])
        err = rel_err(l.download(), z["l"])
        print("laph_apply %s vs the reference: %.3e" % (tag, err))
        assert err < TOL
    finally:
        lat.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_apply_ranges_forms_and_dots(lats, shape):
    lat, g = lats(shape)
    rng = np.random.default_rng(5)
    T = lat.T
    kh, ph = _field(rng, lat), _field(rng, lat)
    ref = lr.apply_field(g, shape, kh)
    k, p, l = lat.cvfield(kh), lat.cvfield(ph), lat.cvfield()
    lat.laph_apply(l, k)
    assert rel_err(l.download(), ref) < TOL
    # sub-ranges: the slices outside stay as they were (a sentinel)
    sent = np.full_like(kh, 7.25)
    for t0, nt in ((1, 1), (T - 1, 1), (1, T - 1), (0, 1)):
        l.upload(sent)
        lat.laph_apply(l, k, t0, nt)
        out = l.download()
        inside = np.zeros(T, dtype=bool)
        inside[t0:t0 + nt] = True
        assert np.array_equal(out[~inside], sent[~inside])
        assert rel_err(out[inside], ref[inside]) < TOL
    # the reducing and the filter form, one launch ("laph_fused" 1) and two (0)
    coef = rng.standard_normal((T, 3))
    want_dot = np.array([np.vdot(lr.cplx(kh[t]), lr.cplx(ref[t])) for t in range(T)])
    nk = np.array([np.linalg.norm(kh[t]) * np.linalg.norm(ref[t]) for t in range(T)])
    want_f = coef[:, 0, None, None, None] * ref + coef[:, 1, None, None, None] * kh + coef[:, 2, None, None, None] * ph
    want_f2 = coef[:, 0, None, None, None] * ref + coef[:, 1, None, None, None] * kh
    got = {}
    try:
        for fused in (1, 0):
            lat.set_option("laph_fused", fused)
            l.zero()
            d = lat.laph_apply(l, k, dot=True)
            assert rel_err(l.download(), ref) < TOL
            assert np.all(np.abs(d - want_dot) <= 3 * (lat.V // T) * EPS * nk), (fused, np.abs(d - want_dot).max())
            lat.laph_apply(l, k, coef=coef, prev=p)
            f3 = l.download()
            assert rel_err(f3, want_f) < TOL
            lat.laph_apply(l, k, coef=coef)
            f2 = l.download()
            assert rel_err(f2, want_f2) < TOL
            # a sub-range of the filter form takes the coefficients of its own slices
            l.upload(sent)
            lat.laph_apply(l, k, T - 1, 1, coef=coef[T - 1:], prev=p)
            out = l.download()
            assert np.array_equal(out[:T - 1], sent[:T - 1]) and rel_err(out[T - 1], want_f[T - 1]) < TOL
            got[fused] = (d, f3, f2)
    finally:
        lat.set_option("laph_fused", 1)
    assert rel_err(got[1][1], got[0][1]) < TOL and rel_err(got[1][2], got[0][2]) < TOL
    assert np.all(np.abs(got[1][0] - got[0][0]) <= 3 * (lat.V // T) * EPS * nk)
    for f in (k, p, l):
        f.free()


def test_changed_links_are_seen_by_the_next_call(lats):
    from tmlqcd_amd import Lattice
    shape = (4, 2, 6, 2)
    lat = Lattice(*shape)
    try:
        g = random_gauge(21, lat.V)
        lat.set_gauge(g)
        rng = np.random.default_rng(3)
        kh = _field(rng, lat)
        k, l = lat.cvfield(kh), lat.cvfield()
        lat.laph_apply(l, k)
        before = l.download()
        assert rel_err(before, lr.apply_field(g, shape, kh)) < TOL
        mom = 0.3 * rng.standard_normal((lat.V, 4, 8))
        lat.momenta_upload(mom)
        lat.update_gauge(0.1)
        g2 = lat.gauge_download()
        assert np.abs(g2 - g).max() > 1e-3
        lat.laph_apply(l, k)
        after = l.download()
        assert rel_err(after, before) > 1e-4
        assert rel_err(after, lr.apply_field(g2, shape, kh)) < TOL
    finally:
        lat.close()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pieces_against_numpy_with_a_frozen_slice(lats, shape):
    lat, _ = lats(shape)
    T, S3 = lat.T, lat.V // lat.T
    N = 3 * S3
    rng = np.random.default_rng(17)
    nv = 70 if S3 <= 256 else 7          # 70: more than the 65 vectors of one launch
    vh = [_field(rng, lat) for _ in range(nv)]
    wh = _field(rng, lat)
    vs, w = [lat.cvfield(h) for h in vh], lat.cvfield(wh)
    Vc = np.stack([lr.cplx(h).reshape(T, N) for h in vh], axis=1)          # [T][nv][N]
    wc = lr.cplx(wh).reshape(T, N)
    active = np.ones(T, dtype=np.int32)
    frozen = T - 1
    active[frozen] = 0
    live = active.astype(bool)
    # dots
    out = np.full((T, nv), 3.5 + 2.5j)
    lat.laph_dots(vs, w, active=active, out=out)
    want = np.einsum("tin,tn->ti", np.conj(Vc), wc)
    bound = N * EPS * np.linalg.norm(Vc, axis=2) * np.linalg.norm(wc, axis=1)[:, None]
    assert np.all(np.abs(out - want)[live] <= bound[live]), np.abs(out - want)[live].max()
    assert np.all(out[frozen] == 3.5 + 2.5j)
    again = np.full((T, nv), 3.5 + 2.5j)
    lat.laph_dots(vs, w, active=active, out=again)
    assert np.array_equal(out.view(np.float64), again.view(np.float64))
    full = lat.laph_dots(vs, w)
    assert np.array_equal(full[live].view(np.float64), out[live].view(np.float64))
    # a sub-range gives the bits of the full range
    part = lat.laph_dots(vs, w, 1, 1)
    assert np.array_equal(part[0].view(np.float64), full[1].view(np.float64))
    # projection
    h = rng.standard_normal((T, nv)) + 1j * rng.standard_normal((T, nv))
    n2 = np.full(T, -1.0)
    lat.laph_project(vs, w, h, active=active, out=n2)
    got = lr.cplx(w.download()).reshape(T, N)
    wantw = wc - np.einsum("ti,tin->tn", h, Vc)
    scale = np.abs(wc).max() + (np.abs(h)[:, :, None] * np.abs(Vc)).max() * nv
    assert np.abs(got - wantw)[live].max() <= 4 * (nv + 1) * EPS * scale
    assert np.array_equal(got[frozen], wc[frozen]) and n2[frozen] == -1.0
    wn = np.sum(np.abs(got) ** 2, axis=1)
    assert np.all(np.abs(n2 - wn)[live] <= N * EPS * wn[live])
    w2 = lat.cvfield(wh)
    n2b = np.full(T, -1.0)
    lat.laph_project(vs, w2, h, active=active, out=n2b)
    assert np.array_equal(n2, n2b) and np.array_equal(w2.download(), w.download())
    # the norms alone, then the scaling to unit norm per slice
    n0 = lat.laph_project([], w, np.zeros((T, 0)), active=active, out=np.full(T, -1.0))
    assert np.array_equal(n0[live], n2[live]) and n0[frozen] == -1.0
    u = lat.cvfield()
    u.upload(np.full_like(wh, 1.5))
    nn = lat.laph_normalise(u, w, active=active, sqnorm=np.full(T, -1.0))
    assert np.array_equal(nn, n2)
    uh = lr.cplx(u.download()).reshape(T, N)
    assert np.abs(uh[live] - got[live] / np.sqrt(wn[live])[:, None]).max() <= 4 * EPS * np.abs(uh[live]).max()
    assert np.all(np.abs(np.sum(np.abs(uh[live]) ** 2, axis=1) - 1.0) <= N * EPS)
    assert np.all(u.download()[frozen] == 1.5)
    # rotation: n vectors, k columns, one matrix per slice; in place, vectors k .. n-1 and the frozen slice stay
    for n, k in ((nv, nv - 1), (nv, 5), (3, 1)):
        for i in range(nv):
            vs[i].upload(vh[i])
        Y = rng.standard_normal((T, n, k))
        lat.laph_rotate(vs[:n], Y, active=active)
        got = np.stack([lr.cplx(f.download()).reshape(T, N) for f in vs], axis=1)
        wantv = np.einsum("tik,tin->tkn", Y, Vc[:, :n])
        bnd = 4 * n * EPS * np.einsum("tik,tin->tkn", np.abs(Y), np.abs(Vc[:, :n]))
        assert np.all(np.abs(got[:, :k] - wantv)[live] <= bnd[live] + 1e-300)
        assert np.array_equal(got[:, k:], Vc[:, k:]) and np.array_equal(got[frozen], Vc[frozen])
        first = [f.download() for f in vs[:k]]
        for i in range(nv):
            vs[i].upload(vh[i])
        lat.laph_rotate(vs[:n], Y, active=active)
        assert all(np.array_equal(a, f.download()) for a, f in zip(first, vs[:k]))
    for f in vs + [w, w2, u]:
        f.free()


def test_rotation_at_the_largest_basis(lats):
    """n = 128 inputs (64 KiB of LDS per block), k = 126 columns: eight column groups, the last one partial"""
    lat, _ = lats((4, 2, 6, 2))
    T, N = lat.T, 3 * (lat.V // lat.T)
    rng = np.random.default_rng(23)
    n, k = 128, 126
    vh = [_field(rng, lat) for _ in range(n)]
    vs = [lat.cvfield(h) for h in vh]
    Vc = np.stack([lr.cplx(h).reshape(T, N) for h in vh], axis=1)
    Y = rng.standard_normal((T, n, k))
    lat.laph_rotate(vs, Y)
    got = np.stack([lr.cplx(f.download()).reshape(T, N) for f in vs], axis=1)
    bnd = 4 * n * EPS * np.einsum("tik,tin->tkn", np.abs(Y), np.abs(Vc))
    assert np.all(np.abs(got[:, :k] - np.einsum("tik,tin->tkn", Y, Vc)) <= bnd)
    assert np.array_equal(got[:, k:], Vc[:, k:])
    for f in vs:
        f.free()


def _refused(capfd, call, text):
    from tmlqcd_amd.hip import TmHipError
    capfd.readouterr()
    with pytest.raises(TmHipError):
        call()
    err = capfd.readouterr().err
    assert text in err, err


def test_refusals_write_nothing(lats, capfd):
    from tmlqcd_amd import Lattice
    lat, _ = lats((4, 2, 6, 2))
    rng = np.random.default_rng(2)
    kh = _field(rng, lat)
    sent = np.full_like(kh, -3.0)
    k, l = lat.cvfield(kh), lat.cvfield(sent)
    other = Lattice(4, 2, 6, 2)
    bare = Lattice(4, 2, 6, 2)
    try:
        other.set_gauge(random_gauge(4, other.V))
        foreign = other.cvfield(kh)
        _refused(capfd, lambda: lat.laph_apply(k, k), "out == in")
        _refused(capfd, lambda: lat.laph_apply(l, k, 2, 3), "outside [0, T = 4)")
        _refused(capfd, lambda: lat.laph_apply(l, k, -1, 2), "outside [0, T = 4)")
        _refused(capfd, lambda: lat.laph_apply(l, k, 0, 0), "outside [0, T = 4)")
        _refused(capfd, lambda: lat.laph_apply(l, foreign), "a field of another context")
        _refused(capfd, lambda: lat.laph_apply(foreign, k), "a field of another context")
        _refused(capfd, lambda: lat.laph_dots([foreign], k), "a field of another context")
        _refused(capfd, lambda: lat.laph_eigensystem(4, start=None, t0=3, nt=2), "outside [0, T = 4)")
        lat.set_option("laph_basis", 5)
        try:
            _refused(capfd, lambda: lat.laph_eigensystem(4), "nev + 2 <= laph_basis = 5")
        finally:
            lat.set_option("laph_basis", 0)
        _refused(capfd, lambda: lat.laph_eigensystem(127), "nev + 2 <= laph_basis = 128")
        assert np.array_equal(l.download(), sent) and np.array_equal(k.download(), kh)
        # no resident links: the refusal of the Polyakov loop
        bk, bl = bare.cvfield(kh), bare.cvfield(sent)
        _refused(capfd, lambda: bare.laph_apply(bl, bk), "the links are not resident (tmhip_set_gauge first)")
        _refused(capfd, lambda: bare.polyakov_loop(0), "the links are not resident (tmhip_set_gauge first)")
        _refused(capfd, lambda: bare.laph_eigensystem(2), "the links are not resident (tmhip_set_gauge first)")
        assert np.array_equal(bl.download(), sent)
        # the loopback rehearsal of a T-split rank
        other.set_loopback(1)
        _refused(capfd, lambda: other.laph_apply(foreign, foreign), "T-split ranks (and their loopback rehearsal) are not built")
        _refused(capfd, lambda: other.laph_eigensystem(2), "T-split ranks (and their loopback rehearsal) are not built")
        _refused(capfd, lambda: other.cvfield(), "T-split ranks (and their loopback rehearsal) are not built")
        other.set_loopback(0)
        assert np.array_equal(foreign.download(), kh)
    finally:
        other.close()
        bare.close()
