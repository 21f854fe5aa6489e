"""TEST INFRASTRUCTURE ONLY: the online measurements of the reference that are not the gradient flow, restated in NumPy.

  slice_sums            the site loops of correlators_measurement (meas/correlators.c:159-170, dir 0) and pion_norm_measurement
                        (meas/pion_norm.c:98-107, dir 3) with _gamma0, _gamma5, _spinor_prod_re, _spinor_prod_im of su3spinor.h
  onlinemeas_text       the file correlators_measurement writes from them (correlators.c:183-229)
  pionnorm_text         the file pion_norm_measurement writes (pion_norm.c:115-138)
  polyakov_loop         polyakov_loop_dir / polyakov_loop (meas/polyakov_loop.c:325-558, :51-157), any direction
  oriented_plaquettes   measure_oriented_plaquettes (meas/oriented_plaquettes.c:39-86) and the line of oriented_plaquettes_measurement
Spinors come as the two e/o halves [V/2][4][3][2] float64 (site = the reference's e/o sub-index: lexicographic index / 2, parity
from the coordinate sum), links as the lexicographic [V][4][3][3][2] field, for any even T, LX, LY, LZ.  Every function returns its
value together with `sum_abs`, the sum over sites or lines of the absolute contribution, which is the scale of its rounding error.
tests/test_meas_restate.py pins all of it to the reference through tests/golden/ref_meas_scalars_*.json."""
import numpy as np

from tests.gauge_restate import _plaq_field, to_complex

PLANES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def eo_to_lexic(even, odd, dims):
    """convert_eo_to_lexic: complex [T][LX][LY][LZ][4][3]"""
    T, LX, LY, LZ = dims
    V = T * LX * LY * LZ
    t, x, y, z = np.unravel_index(np.arange(V), dims)
    par = (t + x + y + z) & 1
    both = np.stack([np.asarray(even)[:V // 2], np.asarray(odd)[:V // 2]])
    lex = both[par, np.arange(V) >> 1]
    return (lex[..., 0] + 1j * lex[..., 1]).reshape(T, LX, LY, LZ, 4, 3)


def split_eo(lex, dims):
    """A lexicographic [V][4][3][2] field -> its (even, odd) halves"""
    V = int(np.prod(dims))
    t, x, y, z = np.unravel_index(np.arange(V), dims)
    par = (t + x + y + z) & 1
    lex = np.asarray(lex).reshape(V, 4, 3, 2)
    return np.ascontiguousarray(lex[par == 0]), np.ascontiguousarray(lex[par == 1])


def site_bilinears(psi):
    """per site: _spinor_prod_re(psi, psi); _spinor_prod_re(psi, gamma0 psi); _spinor_prod_im(psi, gamma5 gamma0 psi)"""
    phi = psi[..., [2, 3, 0, 1], :]                                              # _gamma0
    pp = (psi.real * psi.real + psi.imag * psi.imag).sum(axis=(-1, -2))
    pa = (psi.real * phi.real + psi.imag * phi.imag).sum(axis=(-1, -2))         # _spinor_prod_re(r, s)
    phi = phi * np.array([1.0, 1.0, -1.0, -1.0])[:, None]                        # _gamma5
    p4 = (-psi.real * phi.imag + psi.imag * phi.real).sum(axis=(-1, -2))        # _spinor_prod_im(r, s)
    return pp, pa, p4


def slice_sums(even, odd, dims, dir):
    """{"pp", "pa", "p4"}: the raw sums per slice (dir 0: T time-slices, dir 3: LZ z-slices), and "sum_abs_*" next to each"""
    assert dir in (0, 3)
    vals = site_bilinears(eo_to_lexic(even, odd, dims))
    axes = (1, 2, 3) if dir == 0 else (0, 1, 2)
    out = {}
    for name, v in zip(("pp", "pa", "p4"), vals):
        out[name] = v.sum(axis=axes)
        out["sum_abs_" + name] = np.abs(v).sum(axis=axes)
    return out


def _corr_block(tag, C, t0, n):
    s = "%s  1  0  %e  %e\n" % (tag, C[t0], 0.)
    for t in range(1, n // 2):
        s += "%s  1  %d  %e  " % (tag, t, C[(t0 + t) % n])
        s += "%e\n" % C[(t0 + n - t) % n]
    s += "%s  1  %d  %e  %e\n" % (tag, max(1, n // 2), C[(t0 + n // 2) % n], 0.)     # the C loop leaves t = max(1, n / 2)
    return s


def onlinemeas_text(pp, pa, p4, t0, kappa, dims):
    """correlators.c:183-229 from the raw sums of one rank"""
    T, LX, LY, LZ = dims
    Cpp = [+float(v) / LX / LY / LZ / 2. / kappa / kappa for v in pp]
    Cpa = [-float(v) / LX / LY / LZ / 2. / kappa / kappa for v in pa]
    Cp4 = [+float(v) / LX / LY / LZ / 2. / kappa / kappa for v in p4]
    return _corr_block("1", Cpp, t0, T) + _corr_block("2", Cpa, t0, T) + _corr_block("6", Cp4, t0, T)


def pionnorm_text(pp, z0, dims):
    """pion_norm.c:115-138 from the raw z-slice sums"""
    T, LX, LY, LZ = dims
    Cpp = [+float(v) / LX / LY / T * 2. for v in pp]
    return _corr_block("1", Cpp, z0, LZ)


def polyakov_loop(g, dims, dir):
    """(pl, sum_abs): the trace of the ordered product of the links along `dir` from coordinate 0, summed over the lines and divided
    by 3 lines; sum_abs = the sum of |tr| over the lines"""
    U = np.moveaxis(to_complex(g, dims)[..., dir, :, :], dir, 0)      # [L_dir][the other three extents][3][3]
    P = U[0]
    for k in range(1, U.shape[0]):
        P = P @ U[k]
    tr = np.trace(P, axis1=-2, axis2=-1)
    lines = tr.size
    return complex(tr.sum() / (3. * lines)), float(np.abs(tr).sum())


def oriented_plaquettes(g, dims):
    """(plaq[6], sum_abs[6]): Re tr P / 3 averaged over the sites for the planes (0,1) .. (2,3); sum_abs = sum over sites of |Re tr P|"""
    U = to_complex(g, dims)
    V = int(np.prod(dims))
    fields = [_plaq_field(U, a, b) for a, b in PLANES]
    return [float(f.sum() / 3.0 / V) for f in fields], [float(np.abs(f).sum()) for f in fields]


def oriented_line(traj, plaq):
    return "%.8d %14.12f %14.12f %14.12f %14.12f %14.12f %14.12f\n" % ((traj,) + tuple(plaq))


def polyakov_line(nstore, dir, pl):
    return "%4d\t%2d\t%25.16e\t%25.16e\n" % (nstore, dir, pl.real, pl.imag)
