"""TEST INFRASTRUCTURE ONLY: the molecular-dynamics link and momentum updates in plain NumPy.

update_gauge (update_gauge.c:51-110) multiplies every link by exp(step P).  The reference, the CPU oracle and the device kernel
all evaluate that exponential with the same truncated Cayley-Hamilton polynomial (expo.c:56-97), so agreeing with one another
says nothing about the polynomial itself.  `update_gauge_ld` is the true answer instead: a Taylor series with scaling and
squaring in long double, and NO restoresu3 -- exp of an anti-hermitian traceless matrix is in SU(3) already.

Layouts: links float64 [V][4][3][3][2] (su3.h:40-43), momenta and derivative float64 [V][4][8] (su3adj.h).
"""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).eps < 2e-19, "md_restate needs an extended-precision long double (eps %g)" % np.finfo(LD).eps

_ONE, _THREE = LD(1), LD(3)
_INV_SQRT3, _TWO_INV_SQRT3 = _ONE / np.sqrt(_THREE), LD(2) / np.sqrt(_THREE)


def su3_of(p):
    """_make_su3 (su3adj.h:45-54): the anti-hermitian traceless v = i sum_a p_a lambda_a of su3adj vectors p [..., 8];
    complex long double [..., 3, 3]."""
    p = np.asarray(p, dtype=LD)
    d1, d2, d3, d4, d5, d6, d7, d8 = (p[..., a] for a in range(8))
    v = np.zeros(p.shape[:-1] + (3, 3), dtype=CLD)
    v[..., 0, 0] = 1j * (_INV_SQRT3 * d8 + d3)
    v[..., 0, 1] = d2 + 1j * d1
    v[..., 0, 2] = d5 + 1j * d4
    v[..., 1, 0] = -d2 + 1j * d1
    v[..., 1, 1] = 1j * (_INV_SQRT3 * d8 - d3)
    v[..., 1, 2] = d7 + 1j * d6
    v[..., 2, 0] = -d5 + 1j * d4
    v[..., 2, 1] = -d7 + 1j * d6
    v[..., 2, 2] = -1j * (_TWO_INV_SQRT3 * d8)
    return v


def adj_norm(p):
    """|p|: the Euclidean norm of su3adj vectors [..., 8] (the Frobenius norm of su3_of(p) is sqrt(2) |p|)"""
    return np.sqrt(np.sum(np.asarray(p, dtype=np.float64) ** 2, axis=-1))


def _mm(a, b):
    return np.einsum("...ij,...jk->...ik", a, b)


def expm_ld(v, terms=24):
    """exp(v) of complex [..., 3, 3] in long double: v / 2^s with max-entry norm <= 1/4 (row sums <= 3/4), `terms` Taylor terms
    by Horner (0.75^24 / 24! < 2e-27), s squarings."""
    v = np.asarray(v, dtype=CLD)
    big = float(np.abs(v).max()) if v.size else 0.0
    s = 0
    while big > 0.25 * 2.0 ** s:
        s += 1
    x = v / LD(2) ** s
    eye = np.zeros_like(x)
    for i in range(3):
        eye[..., i, i] = 1
    r = eye.copy()
    for k in range(terms, 0, -1):
        r = eye + _mm(x, r) / LD(k)
    for _ in range(s):
        r = _mm(r, r)
    return r


def cld(g):
    """float64 [..., 2] (re, im) -> complex long double [...]"""
    g = np.asarray(g)
    return g[..., 0].astype(LD) + 1j * g[..., 1].astype(LD)


def update_gauge_ld(g, mom, step):
    """exp(step P_mu(x)) U_mu(x) for every link, complex long double [V][4][3][3] (g, mom untouched)"""
    V = mom.shape[0]
    return _mm(expm_ld(su3_of(LD(step) * np.asarray(mom, dtype=LD))), cld(g[:V]))


def update_momenta(mom, deriv, step):
    """update_momenta.c:67-72: P - step * dS, float64 (one multiply and one subtract per entry, no other rounding)"""
    return mom - step * deriv


def row2_deviation(g):
    """max |row2 - conj(row0 x row1)| (max over the real and imaginary parts) over links float64 [..., 3, 3, 2]: what the guard of
    the 12-real link read measures"""
    u = g[..., 0] + 1j * g[..., 1]
    d = u[..., 2, :] - np.conj(np.cross(u[..., 0, :], u[..., 1, :]))
    return float(max(np.abs(d.real).max(), np.abs(d.imag).max()))
