"""TEST INFRASTRUCTURE ONLY: the loop bodies of the rational monomials restated in NumPy over the CPU oracle.

monomial/ndrat_monomial.c (type NDRAT): force :114-160, heatbath :235-254, acceptance :299-309;
monomial/rat_monomial.c (type RAT, g_mu = 0): force :95-132, heatbath :191-199, acceptance :244-250;
and Q_tau1_sub_const_ndpsi (operator/tm_operators_nd.c:311-380).  Every function takes the shifted solutions as input -- no
solve in here.  Fields are complex [N][4][3] (oracle/nd_restate.py); the derivative is su3adj [VPR][4][8], accumulated by
Oracle.deriv_Sb one call per reference call, in the reference's order (j descending).
"""
import numpy as np

from oracle.nd_restate import H_eo_tm_ndpsi, cplx, hop_over, m_ee_inv, m_oo_sub_g5, real

EO, OE = 0, 1


def Q_tau1_sub_const_ndpsi(H, ks, kc, z, Cpol, invev, mb, eb):
    """tm_operators_nd.c:311-380 -> (l_s, l_c)"""
    d3, d2 = m_ee_inv(H(EO, kc), H(EO, ks), mb, eb)                     # :323-328
    d0, d1 = m_oo_sub_g5(kc, ks, H(OE, d3), H(OE, d2), -mb, -eb)        # :330-336
    return Cpol * invev * d0 - Cpol * z * ks, Cpol * invev * d1 - Cpol * z * kc


class Rat:
    """orc: an Oracle with the gauge field set.  ndrat: g_mubar, g_epsbar = mb, eb.  rat works at g_mu = 0 and puts orc.mu back."""

    def __init__(self, orc, mb=0.0, eb=0.0):
        self.orc, self.mb, self.eb = orc, mb, eb
        self.N = orc.Vh
        self.H = hop_over(orc.Hopping_Matrix, orc.Vh)

    def _buf(self, x):
        b = self.orc.new_field()
        b[:self.N] = real(x)
        return b

    def _deriv(self, ieo, l, k, df, fac):
        self.orc.deriv_Sb(ieo, self._buf(l), self._buf(k), df, fac)

    def _op(self, name, x, *args):
        l = np.zeros((self.N, 4, 3, 2))
        if name == "H_eo_tm_inv_psi":
            self.orc.H_eo_tm_inv_psi(l, real(x), *args)
        else:
            self.orc.op(name, l, real(x))
        return cplx(l)

    # ---- ndrat
    def ndrat_force(self, chi, mu, rmu, invmaxev, df):
        for j in range(len(mu) - 1, -1, -1):
            cu, cd = chi[j]
            w0, w1 = Q_tau1_sub_const_ndpsi(self.H, cu, cd, -1j * mu[j], 1., invmaxev, self.mb, self.eb)
            w2, w3 = H_eo_tm_ndpsi(self.H, cu, cd, EO, self.mb, self.eb)
            f = rmu[j] * invmaxev
            self._deriv(EO, w2, w0, df, f)
            self._deriv(EO, w3, w1, df, f)
            w4, w5 = H_eo_tm_ndpsi(self.H, w0, w1, EO, self.mb, self.eb)
            self._deriv(OE, cu, w4, df, f)
            self._deriv(OE, cd, w5, df, f)
        return df

    def ndrat_heatbath(self, eta_up, eta_dn, chi, nu, rnu, invmaxev):
        """-> (energy0, pf_up, pf_dn)"""
        e0 = float(np.vdot(eta_up, eta_up).real + np.vdot(eta_dn, eta_dn).real)
        pu, pd = eta_up.copy(), eta_dn.copy()
        for j in range(len(nu) - 1, -1, -1):
            tu, td = Q_tau1_sub_const_ndpsi(self.H, chi[j][0], chi[j][1], 1j * nu[j], 1., invmaxev, self.mb, self.eb)
            pu = pu + 1j * rnu[j] * tu
            pd = pd + 1j * rnu[j] * td
        return e0, pu, pd

    @staticmethod
    def ndrat_acc(pf_up, pf_dn, chi, rmu):
        wu, wd = pf_up.copy(), pf_dn.copy()
        for j in range(len(rmu) - 1, -1, -1):
            wu = wu + rmu[j] * chi[j][0]
            wd = wd + rmu[j] * chi[j][1]
        return float(np.vdot(pf_up, wu).real + np.vdot(pf_dn, wd).real)

    # ---- rat (g_mu = 0)
    def _at_mu0(self):
        rat = self

        class _Ctx:
            def __enter__(self):
                self.mu = rat.orc.mu
                rat.orc.set_mu(0.0)

            def __exit__(self, *a):
                rat.orc.set_mu(self.mu)
        return _Ctx()

    def rat_force(self, chi, rmu, df):
        with self._at_mu0():
            for j in range(len(rmu) - 1, -1, -1):
                w0 = self._op("Qtm_plus_psi", chi[j])
                w2 = self._op("H_eo_tm_inv_psi", chi[j], EO, -1.)
                self._deriv(OE, w0, w2, df, rmu[j])
                w3 = self._op("H_eo_tm_inv_psi", w0, EO, +1.)
                self._deriv(EO, w3, chi[j], df, rmu[j])
        return df

    def rat_heatbath(self, eta, chi, nu, rnu):
        """-> (energy0, pf)"""
        e0 = float(np.vdot(eta, eta).real)
        pf = eta.copy()
        with self._at_mu0():
            for j in range(len(nu) - 1, -1, -1):
                t = self._op("Qtm_plus_psi", chi[j])
                t = t + (-1j * nu[j]) * chi[j]
                pf = pf + 1j * rnu[j] * t
        return e0, pf

    @staticmethod
    def rat_acc(pf, chi, rmu):
        w = pf.copy()
        for j in range(len(rmu) - 1, -1, -1):
            w = w + rmu[j] * chi[j]
        return float(np.vdot(pf, w).real)
