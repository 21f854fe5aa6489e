"""TEST INFRASTRUCTURE ONLY (see oracle/README.md).

The non-degenerate twisted-mass doublet restated in complex128 NumPy: the site-local blocks and the Qtm_ndpsi family of
operator/tm_operators_nd.c, and the solvers solver/cg_her_nd.c:57-160 and solver/cg_mms_tm_nd.c:64-215, statement by
statement.  Every operator is a plain composition over a hop callable H(ieo, x) -> Hopping_Matrix(ieo, x) of one flavour;
`hop_over` makes one from the CPU oracle (oracle/oraclebind.Oracle.Hopping_Matrix).

A field is complex [N][4][3] (site, spin, colour); `cplx` / `real` convert from / to the float64 [N][4][3][2] layout of
the reference (su3.h:60-63).  A doublet is a pair (strange = up, charm = dn).  No GPU or torch dependency.
"""
import numpy as np


def cplx(a):
    """float64 [N][4][3][2] -> complex128 [N][4][3]"""
    return a[..., 0] + 1j * a[..., 1]


def real(z):
    """complex128 [N][4][3] -> contiguous float64 [N][4][3][2]"""
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def hop_over(hopping_matrix, N):
    """H(ieo, x) over any hopping_matrix(ieo, l, k) that writes float64 [N][4][3][2] arrays (Oracle.Hopping_Matrix)."""
    def H(ieo, x):
        out = np.zeros((N, 4, 3, 2))
        hopping_matrix(ieo, out, real(x))
        return cplx(out)
    return H


_UP = np.array([1, 1, 0, 0], dtype=bool)[None, :, None]   # spins 0, 1


# ---- site-local blocks ---------------------------------------------------------------------------------------------
def m_ee_inv(ks, kc, mu, eps):
    """M_ee_inv_ndpsi, tm_operators_nd.c:639-696 -> (l_s, l_c)"""
    zs = np.where(_UP, 1 - 1j * mu, 1 + 1j * mu)
    nrm = 1. / (1. + mu * mu - eps * eps)
    return nrm * (zs * ks + eps * kc), nrm * (np.conj(zs) * kc + eps * ks)


def m_oo_sub_g5(ks, kc, js, jc, mu, eps):
    """M_oo_sub_g5_ndpsi, tm_operators_nd.c:698-757 -> (l_s, l_c)"""
    zs = np.where(_UP, 1 - 1j * mu, 1 + 1j * mu)
    p1, p2 = zs * ks + eps * kc, np.conj(zs) * kc + eps * ks
    return np.where(_UP, p1 - js, js - p1), np.where(_UP, p2 - jc, jc - p2)


# ---- operators (g_mubar = mb, g_epsbar = eb, phmc_invmaxev = c) ------------------------------------------------------
def Qtm_ndpsi(H, ks, kc, mb, eb, c):
    """tm_operators_nd.c:68-89 -> (l_s, l_c)"""
    d3, d2 = m_ee_inv(H(0, ks), H(0, kc), mb, eb)
    ls, lc = m_oo_sub_g5(ks, kc, H(1, d3), H(1, d2), -mb, -eb)
    return c * ls, c * lc


def Qtm_dagger_ndpsi(H, ks, kc, mb, eb, c):
    """tm_operators_nd.c:130-152"""
    d2, d3 = m_ee_inv(H(0, kc), H(0, ks), mb, eb)
    ls, lc = m_oo_sub_g5(ks, kc, H(1, d3), H(1, d2), mb, -eb)
    return c * ls, c * lc


def Qtm_pm_ndpsi(H, ks, kc, mb, eb, c):
    """tm_operators_nd.c:195-238"""
    d2, d3 = m_ee_inv(H(0, kc), H(0, ks), mb, eb)
    d2, d3 = m_oo_sub_g5(kc, ks, H(1, d2), H(1, d3), -mb, -eb)
    d5, d4 = m_ee_inv(H(0, d2), H(0, d3), -mb, eb)
    ls, lc = m_oo_sub_g5(d3, d2, H(1, d4), H(1, d5), -mb, -eb)
    return c * c * ls, c * c * lc


def H_eo_tm_ndpsi(H, ks, kc, ieo, mb, eb):
    """tm_operators_nd.c:508-519: the result lands as (l_charm, l_strange)"""
    lc, ls = m_ee_inv(H(ieo, ks), H(ieo, kc), -mb, eb)
    return ls, lc


# ---- solvers -------------------------------------------------------------------------------------------------------
def _nsq(a, b):
    """square_norm(a) + square_norm(b)"""
    return float(np.vdot(a, a).real + np.vdot(b, b).real)


def _dot(a, b, c, d):
    """scalar_prod_r(a, b) + scalar_prod_r(c, d)"""
    return float(np.vdot(a, b).real + np.vdot(c, d).real)


def cg_her_nd(f, P_up, P_dn, Q_up, Q_dn, max_iter, eps_sq, rel_prec):
    """cg_her_nd.c:57-160 with f(x_up, x_dn) -> (y_up, y_dn).  P is the start vector (not modified).
    Returns (return value, x_up, x_dn)."""
    squarenorm = _nsq(Q_up, Q_dn)
    xu, xd = P_up.copy(), P_dn.copy()
    normsp = _nsq(P_up, P_dn)
    if normsp == 0:                                                     # :83-91
        ru, rd = Q_up.copy(), Q_dn.copy()
        pu, pd = Q_up.copy(), Q_dn.copy()
        normsq = _nsq(Q_up, Q_dn)
    else:                                                               # :93-104
        au, ad = f(xu, xd)
        ru, rd = Q_up - au, Q_dn - ad
        pu, pd = ru.copy(), rd.copy()
        normsq = _nsq(pu, pd)
    for iteration in range(max_iter):                                   # :107
        au, ad = f(pu, pd)
        pro = _dot(pu, au, pd, ad)
        alpha = normsq / pro
        xu += alpha * pu
        xd += alpha * pd
        ru += -alpha * au
        rd += -alpha * ad
        err = _nsq(ru, rd)
        if (err <= eps_sq and rel_prec == 0) or (err <= eps_sq * squarenorm and rel_prec == 1):   # :132
            return iteration + 1, xu, xd
        beta = err / normsq                                             # :147-151
        pu = beta * pu + ru
        pd = beta * pd + rd
        normsq = err
    return -1, xu, xd


def cg_mms_tm_nd(f, Q_up, Q_dn, shifts, max_iter, eps_sq, rel_prec):
    """cg_mms_tm_nd.c:64-215: solves (f + shifts[s]^2) x_s = Q.  Returns (return value, [(x_up, x_dn) per shift],
    drops as [iteration, shifts remaining] pairs (the reference's debug line :164), shifts still active at the end)."""
    n = len(shifts)
    sigma = [shifts[0] * shifts[0]] + [shifts[im] * shifts[im] - shifts[0] * shifts[0] for im in range(1, n)]   # :90,95
    P = [[np.zeros_like(Q_up), np.zeros_like(Q_dn)] for _ in range(n)]
    ps = [[Q_up.copy(), Q_dn.copy()] for _ in range(n)]                 # ps[0] unused
    zitam1, zita, alphas, betas = [1.0] * n, [1.0] * n, [1.0] * n, [0.0] * n
    squarenorm = _nsq(Q_up, Q_dn)                                       # :109
    ru, rd = Q_up.copy(), Q_dn.copy()
    pu, pd = Q_up.copy(), Q_dn.copy()
    normsq = squarenorm
    shifts_left = n
    drops = []
    iteration = 0
    for iteration in range(max_iter):                                   # :118
        au, ad = f(pu, pd)                                              # :121-124
        au = au + sigma[0] * pu
        ad = ad + sigma[0] * pd
        pro = _dot(pu, au, pd, ad)
        alpham1 = alphas[0]
        alphas[0] = normsq / pro
        im = 1
        while im < shifts_left:                                         # :133-168
            gamma = zita[im] * alpham1 / (alphas[0] * betas[0] * (1. - zita[im] / zitam1[im]) + alpham1 * (1. + sigma[im] * alphas[0]))
            zitam1[im] = zita[im]
            zita[im] = gamma
            alphas[im] = alphas[0] * zita[im] / zitam1[im]
            P[im][0] += alphas[im] * ps[im][0]
            P[im][1] += alphas[im] * ps[im][1]
            if iteration > 0 and iteration % 20 == 0 and im == shifts_left - 1:
                sn = _nsq(ps[im][0], ps[im][1])
                if alphas[shifts_left - 1] * alphas[shifts_left - 1] * sn <= eps_sq:
                    shifts_left -= 1
                    drops.append([iteration, shifts_left])
            im += 1
        P[0][0] += alphas[0] * pu                                       # :171-176
        P[0][1] += alphas[0] * pd
        ru += -alphas[0] * au
        rd += -alphas[0] * ad
        err = _nsq(ru, rd)                                              # :180
        if (err <= eps_sq and rel_prec == 0) or (err <= eps_sq * squarenorm and rel_prec > 0) or iteration == max_iter - 1:
            break                                                       # :186-190
        betas[0] = err / normsq                                         # :194-197
        pu = betas[0] * pu + ru
        pd = betas[0] * pd + rd
        normsq = err
        for im in range(1, shifts_left):                                # :201-205
            betas[im] = betas[0] * zita[im] * alphas[im] / (zitam1[im] * alphas[0])
            ps[im][0] = betas[im] * ps[im][0] + zita[im] * ru
            ps[im][1] = betas[im] * ps[im][1] + zita[im] * rd
    ret = -1 if iteration == max_iter - 1 else iteration + 1           # :208-209
    return ret, [tuple(x) for x in P], drops, shifts_left
