"""The 104-byte packed link read: the two kept rows of every link in their compact form (tmlqcd_amd/csrc/gauge_pack_codec.h: low
words as they are, high words as 26-bit fields with a five-bit exponent, one escape per link), option gauge_pack_compact.

As in tests/test_gpu_gauge_pack.py and tests/test_gpu_gauge_pack112.py, whose shapes, fixtures and batteries these tests use, every
comparison is np.array_equal against gauge_pack 0 in the same process plus equal iteration counts, or equality of counts -- no
tolerance anywhere.  What a field must report -- 104, 112 or 0 bytes per link, and the rotation counts -- comes from the host model
tests/gauge_pack104_host.py, which tests/test_gauge_pack104_codec.py holds against the header."""
import numpy as np
import pytest

from tests import gauge_pack104_host as g104
from tests import test_gpu_gauge_pack as base
from tests import test_gpu_gauge_pack112 as t112
from tests.util import random_spinor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=base.SHAPES, ids=lambda s: "x".join(map(str, s)))
def setup(request):
    shape = request.param
    g = base._gauge(shape)
    lat = base._lattice(shape, g)
    N = shape[0] * shape[1] * shape[2] * shape[3] // 2
    k, p = random_spinor(31, N), random_spinor(32, N)
    yield shape, g, lat, N, k, p
    lat.close()


def _both_batteries(lat, N, k, p, packed=True):
    base._assert_same_with_and_without(lat, N, k, p, packed=packed)
    base._assert_same_with_and_without(lat, N, k, p, packed=packed, battery=base._battery_dot_and_shifted)


def test_random_su3_field_is_read_in_104_bytes_and_gives_the_same_bits(setup):
    shape, g, lat, N, k, p = setup
    assert lat.gauge_pack_format() == 104
    assert g104.predict(g[:2 * N])[0] == 104
    _both_batteries(lat, N, k, p)


def test_compact_off_reads_112_bytes_with_the_same_rotations_and_bits(setup):
    shape, g, lat, N, k, p = setup
    assert lat.gauge_pack_format() == 104
    st = lat.gauge_pack_stats()
    lat.set_option("gauge_pack_compact", 0)
    try:
        assert lat.gauge_pack_format() == 112
        assert lat.gauge_pack_stats() == st
        _both_batteries(lat, N, k, p)
    finally:
        lat.set_option("gauge_pack_compact", -1)
    assert lat.gauge_pack_format() == 104 and lat.gauge_pack_stats() == st


@pytest.mark.parametrize("rot", [0, 1, 2])
def test_forced_rotation(setup, rot):
    shape, g, lat, N, k, p = setup
    lat.set_option("gauge_pack_rot", rot)
    try:
        fmt, st = g104.predict(g[:2 * N], first=rot)
        print("rot", rot, "model", fmt, st, "device", lat.gauge_pack_format(), lat.gauge_pack_stats())
        assert fmt == 104
        assert lat.gauge_pack_format() == 104
        assert lat.gauge_pack_stats() == st
        base._assert_same_with_and_without(lat, N, k, p, cg=(rot == 2))
    finally:
        lat.set_option("gauge_pack_rot", -1)


def _rebuild_exact_small_integers(a, b):
    """conj(a x b) in the operation order of tmhip_su3_row_rebuild with plain numpy products and sums: for rows of 0.0, -0.0 and
    +-1.0 every product and sum is exact, so this is the device's fma sequence bit for bit, the signs of the zeros included.
    a, b: [n][3][2]."""
    c = np.empty_like(a)
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        re = a[:, i, 0] * b[:, j, 0]
        re = (-a[:, i, 1]) * b[:, j, 1] + re
        re = (-a[:, j, 0]) * b[:, i, 0] + re
        re = a[:, j, 1] * b[:, i, 1] + re
        im = a[:, i, 0] * b[:, j, 1]
        im = a[:, i, 1] * b[:, j, 0] + im
        im = (-a[:, j, 0]) * b[:, i, 1] + im
        im = (-a[:, j, 1]) * b[:, i, 0] + im
        c[:, k, 0], c[:, k, 1] = re, -im
    return c


def test_unit_field_with_negative_zeros(setup):
    """Links of exact 0.0 and 1.0: exponent code 0 and the top of the window.  The third row is what the rebuild of the first two
    gives, so that rotation 0 holds every link: its imaginary parts are -0.0, because the rebuild ends in a negation.  On some links
    -0.0 is planted in the kept rows as well, which the compact form has to hand back with its sign."""
    shape, g, lat, N, k, p = setup
    u = np.zeros((g.shape[0] * 4, 3, 3, 2))
    for r in range(3):
        u[:, r, r, 0] = 1.0
    n = np.arange(len(u))
    u[n % 5 == 0, 0, 1, 0] = -0.0
    u[n % 7 == 0, 1, 2, 1] = -0.0
    u[n % 3 == 0, 0, 0, 1] = -0.0
    u[n % 11 == 0, 1, 0, 0] = -0.0
    u[:, 2] = _rebuild_exact_small_integers(u[:, 0], u[:, 1])
    assert set(np.unique(np.abs(u))) == {0.0, 1.0}
    assert int(np.signbit(u[:, :2]).sum()) > len(u) // 2 and int(np.signbit(u[:, 2]).sum()) > 2 * len(u)
    lat.set_gauge(u.reshape(g.shape))
    try:
        st = lat.gauge_pack_stats()
        print("unit field: format", lat.gauge_pack_format(), "stats", st)
        assert lat.gauge_pack_format() == 104
        assert st == (1, 16 * N, 0, 0, 0)
        base._assert_same_with_and_without(lat, N, k, p, cg=False)
    finally:
        lat.set_gauge(g)


def test_drifted_links(setup):
    """Twelve update_gauge steps as in the 112-byte test: format and rotation counts as the host model predicts for the downloaded
    links, and the bits of the full read."""
    shape, g, lat, N, k, p = setup
    rng = np.random.default_rng(11)
    try:
        for step in range(12):
            if step % 3 == 0:
                lat.momenta_upload(0.3 * rng.standard_normal((2 * N, 4, 8)))
            lat.update_gauge(0.05)
        fmt, st = g104.predict(lat.gauge_download()[:2 * N])
        print("drifted: model", fmt, st, "device", lat.gauge_pack_format(), lat.gauge_pack_stats(), "build %.3f ms" % lat.gauge_pack_build_ms())
        assert lat.gauge_pack_format() == fmt
        assert lat.gauge_pack_stats() == st
        assert st[0] == 1
        _both_batteries(lat, N, k, p)
    finally:
        lat.set_gauge(g)


def _field_with_small_link(g, zero_partner):
    """g with one link whose element [0][0] is 1e-12 + i * (rounding noise), the noise as it comes or set to 0.0.  (The construction
    leaves rounding noise in the imaginary part of element [0][1] as well; zero_partner clears every such real of the link, so
    that the planted 1e-12 is the one small real left.)"""
    u = t112._link_with_small_element(np.random.default_rng(17), 0, 0, 1e-12, False)
    partner = float(u[0, 0, 1])
    assert partner != 0.0 and abs(partner) < 2.0 ** -30          # a second small real in the kept row
    assert 2.0 ** -495 < abs(float(u[0, 0, 0])) < 2.0 ** -30
    if zero_partner:
        noise = np.abs(u) < 2.0 ** -30
        noise[0, 0, 0] = False
        u[noise] = 0.0
        assert u[0, 0, 1] == 0.0 and int((np.abs(u[u != 0.0]) < 2.0 ** -30).sum()) == 1
    g2 = g.copy()
    g2[5, 1] = u
    return g2


def test_one_small_real_takes_the_escape_and_two_fall_back_to_112(setup):
    shape, g, lat, N, k, p = setup
    try:
        g_one = _field_with_small_link(g, True)
        fmt, st_one = g104.predict(g_one[:2 * N])
        assert fmt == 104                                       # exactly one small real in the link's kept rows: the escape
        lat.set_gauge(g_one)
        print("one small real: device", lat.gauge_pack_format(), lat.gauge_pack_stats(), "model", fmt, st_one)
        assert lat.gauge_pack_format() == 104
        assert lat.gauge_pack_stats() == st_one
        base._assert_same_with_and_without(lat, N, k, p, cg=False)

        g_two = _field_with_small_link(g, False)
        fmt, st_two = g104.predict(g_two[:2 * N])
        assert fmt == 112 and st_two == st_one                  # rotations are chosen by the tail alone
        lat.set_gauge(g_two)
        print("two small reals: device", lat.gauge_pack_format(), lat.gauge_pack_stats(), "model", fmt, st_two)
        assert lat.gauge_pack_format() == 112
        assert lat.gauge_pack_stats() == st_one
        base._assert_same_with_and_without(lat, N, k, p, cg=False)
    finally:
        lat.set_gauge(g)


def test_a_link_scaled_by_two_is_read_in_full(setup):
    shape, g, lat, N, k, p = setup
    g2 = g.copy()
    g2[11, 1] *= 2.0
    assert g104.predict(g2[:2 * N])[0] == 0
    lat.set_gauge(g2)
    try:
        st = lat.gauge_pack_stats()
        print("scaled link: format", lat.gauge_pack_format(), "stats", st)
        assert lat.gauge_pack_format() == 0
        assert st[0] == 0 and st[4] == 2                         # the link's forward and backward slot
        base._assert_same_with_and_without(lat, N, k, p, cg=False, packed=False)
    finally:
        lat.set_gauge(g)


def test_set_gauge_and_update_gauge_invalidate_the_format(setup):
    shape, g, lat, N, k, p = setup
    assert lat.gauge_pack_format() == 104
    try:
        lat.set_gauge(_field_with_small_link(g, False))
        assert lat.gauge_pack_format() == 112                    # set_gauge: the twin and its format are built anew
        lat.momenta_upload(0.3 * np.random.default_rng(5).standard_normal((2 * N, 4, 8)))
        lat.update_gauge(0.05)
        fmt, st = g104.predict(lat.gauge_download()[:2 * N])
        print("after update_gauge: model", fmt, st, "device", lat.gauge_pack_format(), lat.gauge_pack_stats())
        assert fmt == 104                                        # the updated link is generic again: no small real left
        assert lat.gauge_pack_format() == 104 and lat.gauge_pack_stats() == st
        base._assert_same_with_and_without(lat, N, k, p, cg=False)
    finally:
        lat.set_gauge(g)
    assert lat.gauge_pack_format() == 104
