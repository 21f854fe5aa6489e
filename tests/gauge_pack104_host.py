"""Host model of the 104-byte packed link read: which kept rows fit the compact form of tmlqcd_amd/csrc/gauge_pack_codec.h, which
rotation the build kernel stores a link on, and from both the format and the counts a whole field must report.

fits_compact is the integer rule of the header (tests/test_gauge_pack104_codec.py holds it against the header compiled as host
code).  The rotation of a link is the first one the tail holds, exactly as for the 112-byte read (tests/gauge_pack_host.py:
rotation_fits, exact rational arithmetic, about a millisecond per link).  field_rotations asks that model only where a
vectorised estimate cannot decide: the rebuild in plain double arithmetic differs from the device's fma sequence by at most
8 roundings of terms below 1, under 2e-15 absolutely, so a stored real whose distance from that estimate plus 2e-15 is below
2^19 of its own ulps (counted with the smaller ulp of its binade's lower neighbour) and below its own magnitude (same sign) fits the
21-bit offset for certain, and one whose distance minus 2e-15 is above 2^21 of its ulps does not."""
import numpy as np

from tests import gauge_pack_host as gph

E_LOW, E_HIGH, E_ESC_MIN = 993, 1023, 528        # biased exponents: [2^-30, 2) plain, [2^-495, 2^-30) through the one escape


def fits_compact(reals):
    """reals: array [..., 12] of doubles (two kept rows).  True where every real is +-0.0 or in [2^-30, 2) except at most one in
    [2^-495, 2^-30)."""
    u = np.ascontiguousarray(reals, dtype=np.float64).view(np.uint64)
    e = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    m = u & np.uint64((1 << 52) - 1)
    zero = (e == 0) & (m == 0)
    plain = (e >= E_LOW) & (e <= E_HIGH)
    small = (e >= E_ESC_MIN) & (e < E_LOW)
    return (zero | plain | small).all(axis=-1) & (small.sum(axis=-1) <= 1)


def kept_rows(links, rot):
    """links [n][3][3][2], rot [n] -> [n][12]: rows rot and rot + 1 (mod 3) in the codec's order"""
    n = len(links)
    idx = np.arange(n)
    return np.concatenate([links[idx, rot % 3].reshape(n, 6), links[idx, (rot + 1) % 3].reshape(n, 6)], axis=1)


def _estimate(links, r):
    """per link: +1 rotation r certainly fits the tail, -1 certainly not, 0 undecided"""
    U = links[..., 0] + 1j * links[..., 1]
    a, b, c = U[:, r % 3], U[:, (r + 1) % 3], links[:, (r + 2) % 3].reshape(len(links), 6)
    w = np.conj(np.cross(a, b))
    w = np.stack([w.real, w.imag], axis=-1).reshape(len(links), 6)
    dist = np.abs(c - w)
    ulp_small = np.spacing(np.abs(c)) * 0.5
    ulp_large = np.spacing(np.abs(c))
    yes = ((dist + 2e-15) < 2.0 ** 19 * ulp_small) & ((dist + 2e-15) < np.abs(c))
    no = (dist - 2e-15) > 2.0 ** 21 * ulp_large
    return np.where(yes.all(axis=1), 1, np.where(no.any(axis=1), -1, 0))


def field_rotations(links, first=0):
    """links [n][3][3][2] -> [n] rotation 0..2 of each link as gauge_pack_kernel chooses it (first, first + 1, first + 2 in turn), 3: none"""
    links = np.ascontiguousarray(links, dtype=np.float64)
    out = np.full(len(links), 3)
    for step in (2, 1, 0):                                    # later steps first, so that earlier ones overwrite
        r = (first + step) % 3
        est = _estimate(links, r)
        for n in np.nonzero(est == 0)[0]:
            est[n] = 1 if gph.rotation_fits(links[n], r) else -1
        out[est == 1] = r
    return out


def predict(g, first=0, compact=True):
    """g: [V][4][3][3][2], the links as downloaded -> (bytes per link 0 | 104 | 112, the five numbers of gauge_pack_stats): every
    link sits in the stencil's copy twice, as the forward hop of its site and the backward hop of its neighbour."""
    links = np.ascontiguousarray(g, dtype=np.float64).reshape(-1, 3, 3, 2)
    rot = field_rotations(links, first)
    counts = [2 * int((rot == r).sum()) for r in range(4)]
    if counts[3]:
        return 0, (0, *counts)
    ok = fits_compact(kept_rows(links, rot)).all()
    return (104 if (compact and ok) else 112), (1, *counts)
