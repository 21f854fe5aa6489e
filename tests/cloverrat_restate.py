"""TEST INFRASTRUCTURE ONLY: the tr-log energies and the CLOVERRAT bodies restated over the CPU oracle and NumPy.

operator/clover_det.c:115-279 (sw_trace, sw_trace_nd) through numpy.linalg.slogdet / det on the 6x6 blocks of the oracle's sw
(tests/ndsw_restate.Clover), and the CLOVERRAT branches of monomial/rat_monomial.c:56-262 through the oracle's Qsw_plus_psi,
Hopping_Matrix + clover_inv (= H_eo_sw_inv_psi), deriv_Sb, sw_spinor_eo, sw_deriv and sw_all, as tests/ndsw_restate.NdCloverRat
does it for the doublet.  No solve in here: the bodies take the shifted solutions as arguments.

Spinor fields are the oracle's real buffers [VPR/2][4][3][2] (the first VOLUME/2 sites are the field) or complex [N][4][3]
(oracle/nd_restate.cplx / real), as each function says.
"""
import numpy as np

from tests.ndsw_restate import EE, EO, OE, OO, Clover, clover_of, cplx, real  # noqa: F401  (re-exported for the tests)


# ---- operator/clover_det.c ------------------------------------------------------------------------------------------------
def sw_trace_terms(cl, ieo, mu):
    """clover_det.c:147-161: log |det(1 + T_i(x) + i mu)|^2 per site of parity ieo and chirality -> [N][2]"""
    a = cl.m[ieo] + 1j * mu * np.eye(6)
    return 2.0 * np.linalg.slogdet(a)[1]


def sw_trace_nd_terms(cl, ieo, mu, eps):
    """clover_det.c:234-252: log( Re det_0 Re det_1 ), det_i = det((1 + T_i(x))^2 + mu^2 - eps^2), per site of parity ieo -> [N]"""
    a = cl.m[ieo]
    d = np.linalg.det(a @ a + (mu * mu - eps * eps) * np.eye(6))
    return np.log(d[:, 0].real * d[:, 1].real)


def sw_trace(cl, ieo, mu):
    """-> (sum over the sites, sum of the absolute values of the per-site terms: the scale a comparison is made on)"""
    t = sw_trace_terms(cl, ieo, mu).sum(axis=1)
    return float(t.sum()), float(np.abs(t).sum())


def sw_trace_nd(cl, ieo, mu, eps):
    t = sw_trace_nd_terms(cl, ieo, mu, eps)
    return float(t.sum()), float(np.abs(t).sum())


# ---- monomial/rat_monomial.c, type CLOVERRAT --------------------------------------------------------------------------------
class CloverRat:
    """The CLOVERRAT bodies over an Oracle created with mu = 0 whose gauge field is set: sw_term and sw_invert(EE, 0.) run in
    here (rat_monomial.c:76-78).  Fields: complex [N][4][3]."""

    def __init__(self, orc, kappa, c_sw):
        self.orc, self.kappa, self.c_sw = orc, kappa, c_sw
        self.N = orc.Vh
        self.sw = orc.sw_term(kappa, c_sw)
        self.sw_inv, self.fails = orc.sw_invert(self.sw, EE, 0.0)
        orc.set_clover(self.sw, self.sw_inv)

    def _buf(self, x):
        b = self.orc.new_field()
        b[:self.N] = real(x)
        return b

    def Qp(self, x):
        """mnl->Qp = Qsw_plus_psi at g_mu = g_mu3 = 0"""
        out = self.orc.new_field()
        self.orc.op("Qsw_plus_psi", out, self._buf(x))
        return cplx(out[:self.N])

    def Qsq(self, x):
        """mnl->Qsq = Qsw_pm_psi"""
        out = self.orc.new_field()
        self.orc.op("Qsw_pm_psi", out, self._buf(x))
        return cplx(out[:self.N])

    def H_eo_sw_inv_psi(self, x, ieo, tau3sign, mu):
        """clovertm_operators.c:268-272"""
        out = self.orc.new_field()
        self.orc.Hopping_Matrix(ieo, out, self._buf(x))
        self.orc.clover_inv(out, tau3sign, mu)
        return cplx(out[:self.N])

    def force(self, chi, rmu, trlog, df):
        """:66-73, :95-139 -> df [VPR][4][8] accumulated; returns (swm, swp) as they stand before sw_all"""
        orc = self.orc
        swm, swp = np.zeros((orc.V, 4, 3, 3, 2)), np.zeros((orc.V, 4, 3, 3, 2))
        for j in range(len(rmu) - 1, -1, -1):
            w0 = self.Qp(chi[j])                                        # :96
            w2 = self.H_eo_sw_inv_psi(chi[j], EO, -1, 0.0)              # :100
            orc.deriv_Sb(OE, self._buf(w0), self._buf(w2), df, rmu[j])  # :102
            w3 = self.H_eo_sw_inv_psi(w0, EO, +1, 0.0)                  # :106
            orc.deriv_Sb(EO, self._buf(w3), self._buf(chi[j]), df, rmu[j])   # :109
            orc.sw_spinor_eo(EE, swm, swp, self._buf(w2), self._buf(w3), rmu[j])       # :113
            orc.sw_spinor_eo(OO, swm, swp, self._buf(w0), self._buf(chi[j]), rmu[j])   # :116
        if trlog:
            orc.sw_deriv(EE, swm, swp, 0.0)                             # :135
        pre = (swm.copy(), swp.copy())
        orc.sw_all(df, swm, swp, self.kappa, self.c_sw)                 # :138
        return pre

    def heatbath(self, eta, chi, nu, rnu):
        """:177, :194-199 -> (energy0, pf)"""
        e0 = float(np.vdot(eta, eta).real)
        pf = eta.copy()
        for j in range(len(nu) - 1, -1, -1):
            t = self.Qp(chi[j]) - 1j * nu[j] * chi[j]
            pf = pf + 1j * rnu[j] * t
        return e0, pf

    @staticmethod
    def acc(pf, chi, rmu):
        """:244-250"""
        w = pf.copy()
        for j in range(len(rmu) - 1, -1, -1):
            w = w + rmu[j] * chi[j]
        return float(np.vdot(pf, w).real)


# ---- the cases of tests/test_gpu_trlog.py -----------------------------------------------------------------------------------
TRACE_SHAPES = [(2, 2, 2, 2), (4, 4, 4, 4), (6, 4, 2, 8)]               # site-local kernels: extents of 2, one block, a ragged one
TRACE_MU = (0.0, 0.23)
# the T-split drop-in case (tests/mp_trlog_worker.py): ((T, LX, LY, LZ) of the whole lattice, gauge seed, kappa, c_sw, mu, (mubar, epsbar))
SPLIT_CASE = ((8, 4, 4, 4), 61, 0.13, 1.57, 0.23, (0.1375, 0.1175))
