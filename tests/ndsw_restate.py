"""TEST INFRASTRUCTURE ONLY: the clover doublet restated in complex128 NumPy, statement by statement.

operator/clover_invert.c:440-495 (sw_invert_nd), operator/clovertm_operators.c:352-425 (clover_inv_nd), :733-850
(clover_gamma5_nd), :960-1074 (assign_mul_one_sw_pm_imu_eps), the Qsw_*_ndpsi family of operator/tm_operators_nd.c,
operator/clover_deriv.c:156-243 (sw_deriv_nd) and the NDCLOVERRAT bodies of monomial/ndrat_monomial.c.  Every operator is a
composition over a hop callable H(ieo, x) (oracle/nd_restate.hop_over) and a `Clover` holding the 6x6 blocks of any sw
array, so it runs on every lattice shape over oracle.oraclebind.Oracle (Hopping_Matrix, sw_term, deriv_Sb, sw_spinor_eo,
sw_all).  The solvers are oracle/nd_restate.py's with the operator passed in.

A field is complex [N][4][3] (oracle/nd_restate.py).  The functions keep the reference's argument ORDER (which differs from
function to function: k_s before k_c here, l_c before l_s there), so that each call site below reads like its original.
"""
import numpy as np

from oracle.nd_restate import cplx, hop_over, real  # noqa: F401  (re-exported for the tests)

EE, OO, EO, OE = 0, 1, 0, 1


def six_invert(a):
    """clover_invert.c:88-160 on complex [..., 6, 6]: Householder triangularisation without pivoting, inversion of the triangle,
    the reflections from the right in reverse order.  Returns (inverse, number of near-singular pivots)."""
    a = np.array(a, dtype=np.complex128)
    tiny = 1.0e-20
    sh = a.shape[:-2]
    d = np.zeros(sh + (6,), dtype=np.complex128)
    p = np.zeros(sh + (6,))
    fails = 0
    for k in range(5):
        s = np.sum(np.abs(a[..., k + 1:, k]) ** 2, axis=-1)
        s = np.sqrt(1.0 + s / np.abs(a[..., k, k]) ** 2)
        sigma = s * a[..., k, k]
        a[..., k, k] += sigma
        p[..., k] = (sigma * np.conj(a[..., k, k])).real
        q = np.abs(sigma) ** 2
        fails += int(np.sum(q < tiny))
        d[..., k] = -np.conj(sigma) / q
        for j in range(k + 1, 6):
            z = np.sum(np.conj(a[..., k:, k]) * a[..., k:, j], axis=-1) / p[..., k]
            a[..., k:, j] -= z[..., None] * a[..., k:, k]
    sigma = a[..., 5, 5]
    q = np.abs(sigma) ** 2
    fails += int(np.sum(q < tiny))
    d[..., 5] = np.conj(sigma) / q
    for k in range(5, -1, -1):
        for i in range(k - 1, -1, -1):
            z = np.sum(a[..., i, i + 1:k] * a[..., i + 1:k, k], axis=-1) + a[..., i, k] * d[..., k]
            a[..., i, k] = -z * d[..., i]
    a[..., 5, 5] = d[..., 5]
    for k in range(4, -1, -1):
        u = a[..., k:, k].copy()
        a[..., k, k] = d[..., k]
        a[..., k + 1:, k] = 0
        z = np.einsum("...ij,...j->...i", a[..., :, k:], u) / p[..., k, None]
        a[..., :, k:] -= z[..., :, None] * np.conj(u)[..., None, :]
    return a, fails


class Clover:
    """The 6x6 blocks of one sw array [V][3][2][3][3][2] (operator/clover_term.c) per parity, and of sw_invert_nd's result."""

    def __init__(self, sw, eo2lexic, Vh, odd_offset):
        """eo2lexic: g_eo2lexic; odd_offset: (VOLUME + RAND) / 2, where the odd sites start in it."""
        self.Vh = Vh
        self.lex = [np.asarray(eo2lexic[:Vh]), np.asarray(eo2lexic[odd_offset:odd_offset + Vh])]
        swc = sw[..., 0] + 1j * sw[..., 1]                    # [V][3][2][3][3]
        self.m = [self._six(swc[ix]) for ix in self.lex]      # [parity] -> [N][2 chiralities][6][6]
        self.inv = None                                       # [N][2][6][6] after sw_invert_nd (even sites)
        self.fails = 0

    @staticmethod
    def _six(s):
        """populate_6x6_matrix as sw_invert_nd / sw_deriv_nd do it: (sw[0], sw[1]; sw[1]^dagger, sw[2]) per chirality"""
        n = s.shape[0]
        m = np.zeros((n, 2, 6, 6), dtype=np.complex128)
        for i in range(2):
            m[:, i, :3, :3] = s[:, 0, i]
            m[:, i, :3, 3:] = s[:, 1, i]
            m[:, i, 3:, :3] = np.conj(np.swapaxes(s[:, 1, i], -1, -2))
            m[:, i, 3:, 3:] = s[:, 2, i]
        return m

    def sw_invert_nd(self, mshift, inverse=six_invert):
        """clover_invert.c:440-495 -> sw_inv in the host layout [V/2][4][2][3][3][2]"""
        a = self.m[0]
        b = a @ a + mshift * np.eye(6)
        r = inverse(b)
        self.inv, self.fails = (r if isinstance(r, tuple) else (r, 0))
        return self.sw_inv_host()

    def sw_inv_host(self):
        w = self.inv
        out = np.zeros((self.Vh, 4, 2, 3, 3), dtype=np.complex128)
        for i in range(2):
            out[:, 0, i] = w[:, i, :3, :3]
            out[:, 1, i] = w[:, i, :3, 3:]
            out[:, 2, i] = w[:, i, 3:, 3:]
            out[:, 3, i] = w[:, i, 3:, :3]
        return real(out)

    def cond(self, mshift):
        """largest 2-norm condition number of (1+T)^2 + mshift over the even sites and both chiralities"""
        a = self.m[0]
        return float(np.linalg.cond(a @ a + mshift * np.eye(6)).max())

    def logdet(self, mshift):
        """sum over the even sites of log det((1+T)^2 + mshift)"""
        a = self.m[0]
        sign, ld = np.linalg.slogdet(a @ a + mshift * np.eye(6))
        return float(ld.sum())


def _chir(x):
    """complex [N][4][3] -> [N][2 chiralities][6] (spins 2b, 2b+1)"""
    return x.reshape(x.shape[0], 2, 6)


def _spin(y):
    return y.reshape(y.shape[0], 4, 3)


_SGN = np.array([1.0, -1.0])[None, :, None]   # +i mu on spins 0, 1 and -i mu on spins 2, 3 for the "_s" flavour


def assign_mul_one_sw_pm_imu_eps(cl, ieo, l_s, l_c, mu, eps):
    """clovertm_operators.c:960-1074 -> (k_s, k_c)"""
    m = cl.m[ieo]
    s, c = _chir(l_s), _chir(l_c)
    ks = np.einsum("nbij,nbj->nbi", m, s) + 1j * mu * _SGN * s + eps * c
    kc = np.einsum("nbij,nbj->nbi", m, c) - 1j * mu * _SGN * c + eps * s
    return _spin(ks), _spin(kc)


def clover_inv_nd(cl, ieo, l_c, l_s):
    """clovertm_operators.c:352-425 -> (l_c, l_s); sw_invert_nd fills the even sites only"""
    assert ieo == EE and cl.inv is not None
    f = lambda x: _spin(np.einsum("nbij,nbj->nbi", cl.inv, _chir(x)))
    return f(l_c), f(l_s)


def clover_gamma5_nd(cl, ieo, k_c, k_s, j_c, j_s, mubar, epsbar):
    """clovertm_operators.c:733-850 -> (l_c, l_s)"""
    ps, pc = assign_mul_one_sw_pm_imu_eps(cl, ieo, k_s, k_c, mubar, epsbar)
    up = np.array([1, 1, 0, 0], dtype=bool)[None, :, None]
    return np.where(up, pc - j_c, j_c - pc), np.where(up, ps - j_s, j_s - ps)


# ---- operators (g_mubar = mb, g_epsbar = eb, phmc_invmaxev = c); all return (l_strange, l_charm) --------------------------
def _q(cl, H, ks, kc, mb, eb, c):
    d0, d1 = H(EO, kc), H(EO, ks)
    d2, d3 = assign_mul_one_sw_pm_imu_eps(cl, EE, d0, d1, mb, eb)
    d2, d3 = clover_inv_nd(cl, EE, d2, d3)
    d0, d1 = H(OE, d2), H(OE, d3)
    d2, d3 = clover_gamma5_nd(cl, OO, kc, ks, d0, d1, mb, -eb)
    return c * d3, c * d2                                               # l_charm = c D2, l_strange = c D3


def Qsw_ndpsi(cl, H, ks, kc, mb, eb, c):
    """tm_operators_nd.c:91-111"""
    return _q(cl, H, ks, kc, mb, eb, c)


def Qsw_dagger_ndpsi(cl, H, ks, kc, mb, eb, c):
    """tm_operators_nd.c:154-174"""
    return _q(cl, H, ks, kc, -mb, eb, c)


def Qsw_pm_ndpsi(cl, H, ks, kc, mb, eb, c):
    """tm_operators_nd.c:240-285"""
    d0, d1 = H(EO, kc), H(EO, ks)
    d2, d3 = assign_mul_one_sw_pm_imu_eps(cl, EE, d0, d1, -mb, eb)
    d2, d3 = clover_inv_nd(cl, EE, d2, d3)
    d0, d1 = H(OE, d2), H(OE, d3)
    d2, d3 = clover_gamma5_nd(cl, OO, kc, ks, d0, d1, -mb, -eb)
    d0, d1 = H(EO, d3), H(EO, d2)
    d7, d6 = assign_mul_one_sw_pm_imu_eps(cl, EE, d1, d0, mb, eb)
    d6, d7 = clover_inv_nd(cl, EE, d6, d7)
    d0, d1 = H(OE, d6), H(OE, d7)
    lc, ls = clover_gamma5_nd(cl, OO, d2, d3, d1, d0, mb, -eb)
    return c * c * ls, c * c * lc


def Qsw_tau1_sub_const_ndpsi(cl, H, ks, kc, z, Cpol, invev, mb, eb):
    """tm_operators_nd.c:378-444"""
    d0, d1 = H(EO, kc), H(EO, ks)
    d3, d2 = assign_mul_one_sw_pm_imu_eps(cl, EE, d0, d1, -mb, eb)     # :393-394: (k_s, k_c) = (D3, D2)
    d2, d3 = clover_inv_nd(cl, EE, d2, d3)
    ls, lc = H(OE, d3), H(OE, d2)
    d0, d1 = clover_gamma5_nd(cl, OO, kc, ks, ls, lc, -mb, -eb)         # l_c = D0, l_s = D1; j_c = l_strange, j_s = l_charm
    return Cpol * invev * d0 - Cpol * z * ks, Cpol * invev * d1 - Cpol * z * kc


def H_eo_sw_ndpsi(cl, H, ks, kc, mb, eb):
    """tm_operators_nd.c:521-535"""
    d0, d1 = H(EO, ks), H(EO, kc)
    lc, ls = assign_mul_one_sw_pm_imu_eps(cl, EE, d0, d1, mb, eb)       # (k_s, k_c) = (l_charm, l_strange)
    ls, lc = clover_inv_nd(cl, EE, ls, lc)
    return ls, lc


def Msw_ee_inv_ndpsi(cl, ks, kc, mb, eb):
    """tm_operators_nd.c:539-549"""
    ls, lc = assign_mul_one_sw_pm_imu_eps(cl, EE, ks, kc, -mb, eb)
    ls, lc = clover_inv_nd(cl, EE, ls, lc)
    return ls, lc


def sw_deriv_nd(cl, ieo, swm, swp):
    """clover_deriv.c:156-243: accumulates into swm / swp [V][4][3][3][2] (lexicographic sites)"""
    a = cl.m[ieo] @ cl.inv                                              # [N][2][6][6]
    for acc, b in ((swp, a[:, 1] + a[:, 0]), (swm, a[:, 1] - a[:, 0])):
        blk = np.stack([b[:, :3, :3], b[:, :3, 3:], b[:, 3:, 3:], b[:, 3:, :3]], axis=1)
        acc[cl.lex[ieo]] += real(blk)


class NdCloverRat:
    """The NDCLOVERRAT bodies of monomial/ndrat_monomial.c over an Oracle with the gauge field set; no solve in here."""

    def __init__(self, orc, cl, mb, eb):
        self.orc, self.cl, self.mb, self.eb = orc, cl, mb, eb
        self.N = orc.Vh
        self.H = hop_over(orc.Hopping_Matrix, orc.Vh)

    def _buf(self, x):
        b = self.orc.new_field()
        b[:self.N] = real(x)
        return b

    def force(self, chi, mu, rmu, invmaxev, kappa, c_sw, trlog, df):
        """:80-86, :114-184 -> df [VPR][4][8] accumulated; returns (swm, swp) as they stand before sw_all"""
        orc, cl, H, mb, eb = self.orc, self.cl, self.H, self.mb, self.eb
        swm, swp = np.zeros((orc.V, 4, 3, 3, 2)), np.zeros((orc.V, 4, 3, 3, 2))
        for j in range(len(mu) - 1, -1, -1):
            cu, cd = chi[j]
            w0, w1 = Qsw_tau1_sub_const_ndpsi(cl, H, cu, cd, -1j * mu[j], 1., invmaxev, mb, eb)
            w2, w3 = H_eo_sw_ndpsi(cl, H, cu, cd, mb, eb)
            f = rmu[j] * invmaxev
            orc.deriv_Sb(EO, self._buf(w2), self._buf(w0), df, f)
            orc.deriv_Sb(EO, self._buf(w3), self._buf(w1), df, f)
            w4, w5 = H_eo_sw_ndpsi(cl, H, w0, w1, mb, eb)
            orc.deriv_Sb(OE, self._buf(cu), self._buf(w4), df, f)
            orc.deriv_Sb(OE, self._buf(cd), self._buf(w5), df, f)
            orc.sw_spinor_eo(EE, swm, swp, self._buf(w5), self._buf(w2), f)
            orc.sw_spinor_eo(OO, swm, swp, self._buf(cu), self._buf(w1), f)
            orc.sw_spinor_eo(EE, swm, swp, self._buf(w4), self._buf(w3), f)
            orc.sw_spinor_eo(OO, swm, swp, self._buf(cd), self._buf(w0), f)
        if trlog:
            sw_deriv_nd(cl, EE, swm, swp)
        pre = (swm.copy(), swp.copy())
        orc.sw_all(df, swm, swp, kappa, c_sw)
        return pre

    def heatbath(self, eta_up, eta_dn, chi, nu, rnu, invmaxev):
        """:212-217, :235-254 -> (energy0, pf_up, pf_dn)"""
        e0 = float(np.vdot(eta_up, eta_up).real + np.vdot(eta_dn, eta_dn).real)
        pu, pd = eta_up.copy(), eta_dn.copy()
        for j in range(len(nu) - 1, -1, -1):
            tu, td = Qsw_tau1_sub_const_ndpsi(self.cl, self.H, chi[j][0], chi[j][1], 1j * nu[j], 1., invmaxev, self.mb, self.eb)
            pu = pu + 1j * rnu[j] * tu
            pd = pd + 1j * rnu[j] * td
        return e0, pu, pd

    @staticmethod
    def acc(pf_up, pf_dn, chi, rmu):
        """:299-309"""
        wu, wd = pf_up.copy(), pf_dn.copy()
        for j in range(len(rmu) - 1, -1, -1):
            wu = wu + rmu[j] * chi[j][0]
            wd = wd + rmu[j] * chi[j][1]
        return float(np.vdot(pf_up, wu).real + np.vdot(pf_dn, wd).real)


def clover_of(orc, kappa, c_sw):
    """Clover blocks from the oracle's sw_term on its current gauge field"""
    return Clover(orc.sw_term(kappa, c_sw), orc.eo2lexic(), orc.Vh, orc.VPR // 2)


# ---- the cases of the GPU tests (tests/test_gpu_ndsw_*.py, test_gpu_ndcloverrat.py); tests/test_ndsw_restate.py asserts that every
# 6x6 block (1+T)^2 + mubar^2 - epsbar^2 they meet is well conditioned in the restatement alone
KAPPA, C_SW = 0.13, 1.57
THETA = (1.0, 0.3, -0.2, 0.5)
FIXTURE = (0.1375, 0.1175, 0.6931)                                     # (mubar, epsbar, invmaxev) of tests/golden/ref_nd_* / ref_ndsw_*
POINTS = {"fixture": FIXTURE, "epsbar0": (0.1375, 0.0, 0.6931), "mubar0": (0.0, 0.1175, 0.6931), "eps_gt_mu": (0.05, 0.12, 0.6931)}
SMALL = [(2, 2, 2, 2), (4, 2, 6, 2), (6, 10, 2, 4), (24, 4, 4, 4), (4, 4, 4, 16)]     # the lists of tests/test_gpu_nd_shapes.py
XCD = [((10, 10, 6, 14), 0), ((18, 12, 12, 14), 256)]
SHAPES = [(sh, 0) for sh in SMALL] + XCD
COND_MAX = 1.0e3
FORCE_SHAPES = [(4, 4, 4, 4), (6, 4, 2, 8)]                            # tests/test_gpu_ndcloverrat.py: forces and sw_deriv_nd (fixture point) ...
DRIVER_SHAPE = (4, 4, 6, 4)                                            # ... and the drivers
REFUSAL_SHIFT = 0.005                                                  # tests/test_gpu_ndsw_shapes.py::test_refusals on (4, 2, 6, 2)


def shape_seed(shape):
    return 3000 + sum(shape) * 7 + shape[0]
