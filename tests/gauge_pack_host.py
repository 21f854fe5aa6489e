"""Host model of the packed link codec (tmlqcd_amd/csrc/gauge_pack_codec.h), for the tests of the 112-byte link read.

rebuild_row does the device's fma sequence in exact rational arithmetic with one rounding to double per step (float(Fraction) is
correctly rounded), so it returns the device's rebuilt row bit for bit; offset / fits are the integer rule of the tail.
tests/test_gauge_pack_codec.py holds both against the C++ header compiled as host code."""
import struct
from fractions import Fraction as F

BITS = 21
DMAX, DMIN = 2 ** (BITS - 1) - 1, -2 ** (BITS - 1)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def real(u):
    return struct.unpack("<d", struct.pack("<Q", u & 0xFFFFFFFFFFFFFFFF))[0]


def add_ulps(x, k):
    """The double whose 64-bit pattern is bits(x) + k."""
    return real(bits(x) + k)


def _fma(a, b, c):
    return float(F(a) * F(b) + F(c))


def rebuild_row(a, b):
    """conj(a x b) as tmhip_su3_row_rebuild computes it.  a, b: three (re, im) pairs each; returns six floats re0, im0, re1, ..."""
    out = []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        re = float(F(a[i][0]) * F(b[j][0]))
        re = _fma(-a[i][1], b[j][1], re)
        re = _fma(-a[j][0], b[i][0], re)
        re = _fma(a[j][1], b[i][1], re)
        im = float(F(a[i][0]) * F(b[j][1]))
        im = _fma(a[i][1], b[j][0], im)
        im = _fma(-a[j][0], b[i][1], im)
        im = _fma(-a[j][1], b[i][0], im)
        out += [re, -im]
    return out


def offset(stored, rebuilt):
    """The tail's offset of one real, or None where it has none (out of range, or the signs differ)."""
    s, w = bits(stored), bits(rebuilt)
    if (s ^ w) >> 63:
        return None
    d = s - w
    return d if DMIN <= d <= DMAX else None


def rotation_fits(u, r):
    """u: a link as [3][3][2] floats.  True where rotation r (rows r, r + 1 kept, row r + 2 rebuilt) encodes it."""
    a, b, c = u[r % 3], u[(r + 1) % 3], u[(r + 2) % 3]
    w = rebuild_row([(float(x[0]), float(x[1])) for x in a], [(float(x[0]), float(x[1])) for x in b])
    stored = [float(c[e][p]) for e in range(3) for p in range(2)]
    return all(offset(s, x) is not None for s, x in zip(stored, w))
