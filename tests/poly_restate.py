"""TEST INFRASTRUCTURE ONLY: the polynomial monomial NDPOLY restated in NumPy over the CPU oracle.

Ptilde_nd.c:141-189 (Clenshaw's recursion around a Qsq callable) and the branch g_epsbar != 0 || phmc_exact_poly == 0 of
monomial/ndpoly_monomial.c: derivative :79-117, heatbath :179-209 + 255-256 (without the random numbers), acceptance :282-368.
Fields are complex [N][4][3] (oracle/nd_restate.py); the derivative is su3adj [VPR][4][8], accumulated by Oracle.deriv_Sb one
call per reference call, in the reference's order.  n = MDPolyDegree, roots = the 2n - 2 complex MDPolyRoots.
"""
import numpy as np

from oracle.nd_restate import H_eo_tm_ndpsi, Qtm_dagger_ndpsi, Qtm_ndpsi, Qtm_pm_ndpsi, _nsq
from tests.rat_restate import EO, OE, Q_tau1_sub_const_ndpsi, Rat
from tests.util import TOL


def roots_of(s):
    """the complex MDPolyRoots of a scalars fixture (tests/golden/ref_poly_scalars_*.json)"""
    return [complex(a, b) for a, b in s["MDPolyRoots"]]


def gpu_bound(s, key, j=None):
    """the bound of the GPU tests for quantity `key` of a scalars fixture (entry j of a list): 8 x the deviation this restatement has from
    the reference (`restate_vs_ref`, stored by tools/make_golden_poly.py, re-measured by tests/test_poly_restate.py), at least TOL"""
    d = s["restate_vs_ref"][key]
    return max(8.0 * (d if j is None else d[j]), TOL)


def comb4(R, S, U, V, c1, c2, c3, c4):
    """linalg/assign_mul_add_mul_add_mul_add_mul_r.c:64: c1 R + c2 S + c3 U + c4 V, added left to right"""
    return ((c1 * R + c2 * S) + c3 * U) + c4 * V


def Ptilde_ndpsi(Qsq, coefs, Ss, Sc, evmin, evmax):
    """Ptilde_nd.c:141-189 -> (R_s, R_c); Qsq(x_s, x_c) -> (y_s, y_c)"""
    n = len(coefs)
    fact1 = 4 / (evmax - evmin)
    fact2 = -2 * (evmax + evmin) / (evmax - evmin)
    ds, dc = np.zeros_like(Ss), np.zeros_like(Sc)
    dds, ddc = np.zeros_like(Ss), np.zeros_like(Sc)
    for j in range(n - 1, 0, -1):
        svs, svc = ds, dc
        Rs, Rc = Qsq(ds, dc)
        ds = comb4(ds, Rs, dds, Ss, fact2, fact1, -1.0, coefs[j])
        dc = comb4(dc, Rc, ddc, Sc, fact2, fact1, -1.0, coefs[j])
        dds, ddc = svs, svc
    auxs, auxc = Qsq(ds, dc)
    t2, t3, t4 = coefs[0] / 2, fact1 / 2, fact2 / 2
    return comb4(auxs, ds, dds, Ss, t3, t4, -1.0, t2), comb4(auxc, dc, ddc, Sc, t3, t4, -1.0, t2)


class Poly(Rat):
    """orc: an Oracle with the gauge field set; g_mubar, g_epsbar = mb, eb; invmaxev = phmc_invmaxev = the monomial's EVMaxInv."""

    def __init__(self, orc, mb, eb, invmaxev):
        Rat.__init__(self, orc, mb, eb)
        self.c = invmaxev

    def Qsq(self, xs, xc):
        return Qtm_pm_ndpsi(self.H, xs, xc, self.mb, self.eb, self.c)

    def _qt1(self, ks, kc, z, Cpol):
        return Q_tau1_sub_const_ndpsi(self.H, ks, kc, z, Cpol, self.c, self.mb, self.eb)

    def Ptilde(self, coefs, Ss, Sc, evmin, evmax):
        return Ptilde_ndpsi(self.Qsq, coefs, Ss, Sc, evmin, evmax)

    def derivative(self, pf_up, pf_dn, roots, Cpol, df):
        """:79-117, forcefactor = -Cpol invmaxev (:69)"""
        n = len(roots) // 2 + 1
        ff = -Cpol * self.c
        chi = [(pf_up, pf_dn)]
        for k in range(1, n - 1):
            chi.append(self._qt1(chi[k - 1][0], chi[k - 1][1], roots[k - 1], Cpol))
        hi = chi[n - 2]
        for j in range(n - 1, 0, -1):
            hi = self._qt1(hi[0], hi[1], roots[2 * n - 3 - j], Cpol)
            w0, w1 = H_eo_tm_ndpsi(self.H, chi[j - 1][0], chi[j - 1][1], EO, self.mb, self.eb)
            self._deriv(EO, w0, hi[0], df, ff)
            self._deriv(EO, w1, hi[1], df, ff)
            w0, w1 = H_eo_tm_ndpsi(self.H, hi[0], hi[1], EO, self.mb, self.eb)
            self._deriv(OE, chi[j - 1][0], w0, df, ff)
            self._deriv(OE, chi[j - 1][1], w1, df, ff)
        return df

    def _B(self, up, dn, rts, Cpol):
        for z in rts:
            up, dn = self._qt1(up, dn, z, Cpol)
        return up, dn

    def heatbath(self, eta_up, eta_dn, roots, Cpol, ptilde_coefs, evmin, evmax):
        """:179-209, 255-256 -> (energy0, pf_up, pf_dn)"""
        n = len(roots) // 2 + 1
        e0 = _nsq(eta_up, eta_dn)
        up, dn = Qtm_ndpsi(self.H, eta_up, eta_dn, self.mb, self.eb, self.c)
        up, dn = self._B(up, dn, [roots[n - 2 + j] for j in range(1, n)], Cpol)
        pu, pd = self.Ptilde(ptilde_coefs, up, dn, evmin, evmax)
        return e0, pu, pd

    def acc(self, pf_up, pf_dn, roots, Cpol, md_coefs, ptilde_coefs, evmin, evmax, precision_hfinal):
        """:282-368 -> (energy1, corrections, Ener[0 .. 7])"""
        n = len(roots) // 2 + 1
        Ener = [0.0] * 8
        factor = [1.0] * 8
        for j in range(1, 8):
            factor[j] = j * factor[j - 1]
        chi = [None] * 8
        chi[0] = self._B(pf_up, pf_dn, [roots[j - 1] for j in range(1, n)], Cpol)
        Ener[0] = _nsq(*chi[0])
        ij, steps = 0, 0
        for j in range(1, 8):
            steps = j
            if j % 2:
                a = self.Ptilde(ptilde_coefs, chi[j - 1][0], chi[j - 1][1], evmin, evmax)
                b = self.Ptilde(md_coefs, a[0], a[1], evmin, evmax)
                chi[j - 1] = b
                chi[j] = Qtm_dagger_ndpsi(self.H, b[0], b[1], self.mb, self.eb, self.c)
            else:
                a = Qtm_ndpsi(self.H, chi[j - 1][0], chi[j - 1][1], self.mb, self.eb, self.c)
                b = self.Ptilde(md_coefs, a[0], a[1], evmin, evmax)
                chi[j - 1] = b
                chi[j] = self.Ptilde(ptilde_coefs, b[0], b[1], evmin, evmax)
            Ener[j] = Ener[j - 1] + Ener[0]
            sgn = -1.0
            ij = 1
            while ij < j:
                Ener[j] += sgn * (factor[j] / (factor[ij] * factor[j - ij])) * Ener[ij]
                sgn = -sgn
                ij += 1
            Ener[j] += sgn * _nsq(*chi[j])
            if abs(Ener[j] - Ener[j - 1]) < precision_hfinal:
                break
        return Ener[ij], steps, Ener
