"""TEST INFRASTRUCTURE ONLY: the Wilson gradient flow of the reference restated in NumPy.

step_gradient_flow and the loop of gradient_flow_measurement (meas/gradient_flow.c:52-222), project_traceless_antiherm and
cayley_hamilton_exponent (matrix_utils.c:45-137) and measure_clover_field_strength_observables
(meas/measure_clover_field_strength_observables.c:55-225), in the idiom of tests/gauge_restate.py: a lexicographic
[V][4][3][3][2] float64 field for any T, LX, LY, LZ (extent 2 included: shifts are np.roll), staples and clover leaves written as
the paths of links they walk."""
import numpy as np

from tests.gauge_restate import MM, MN, PLAQUETTE_PATHS, PM, PN, _dag, expm_su3, measure_plaquette, path_product, to_complex

ZFAC = (1.0, 8.0 / 9.0, -17.0 / 36.0, 3.0 / 4.0, -1.0)
ZEPSFAC = (0.25, 1.0, 1.0)
# the four plaquettes of the clover leaf (mu = k, nu = l) as closed paths from x, measure_clover_field_strength_observables.c:135-162
LEAF_PATHS = ((PM, PN, MM, MN), (PN, MM, MN, PM), (MM, MN, PM, PN), (MN, PM, PN, MM))
PLANES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# the terms of new_epsilon4() (tensors.h:65-92) that survive "i1 < i2 and i3 < i4", in its order: (sign, plane, plane)
EPS_TERMS = ((+1, (0, 1), (2, 3)), (-1, (0, 2), (1, 3)), (+1, (0, 3), (1, 2)), (+1, (1, 2), (0, 3)), (-1, (1, 3), (0, 2)), (+1, (2, 3), (0, 1)))
E_NORM = lambda V: -4 / (4 * 16.0 * V)                    # noqa: E731   (g_nproc = 1)
Q_NORM = -1 / (4 * 32.0 * np.pi * np.pi)


def from_complex(U):
    """complex [T][LX][LY][LZ][4][3][3] -> [V][4][3][3][2] float64"""
    out = np.empty(U.shape + (2,))
    out[..., 0], out[..., 1] = U.real, U.imag
    return out.reshape(-1, 4, 3, 3, 2)


def project_traceless_antiherm(m):
    """matrix_utils.c:117-137: note the factor 0.5 and that the diagonal keeps its imaginary part only"""
    out = np.empty_like(m)
    tr = (1.00 / 3.00) * (m[..., 0, 0].imag + m[..., 1, 1].imag + m[..., 2, 2].imag)
    for i in range(3):
        out[..., i, i] = (m[..., i, i].imag - tr) * 1j
    for i, j in ((0, 1), (0, 2), (1, 2)):
        out[..., i, j] = (m[..., i, j] - np.conj(m[..., j, i])) * 0.50
        out[..., j, i] = -np.conj(out[..., i, j])
    return out


def cayley_hamilton_exponent(A):
    """matrix_utils.c:45-115, formula by formula, for a stack of traceless anti-hermitian matrices"""
    a = lambda i, j: A[..., i, j]                          # noqa: E731
    c0 = (1j * (a(0, 0) * (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) + a(0, 1) * (a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2)) +
                a(0, 2) * (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)))).real
    c1 = -0.5 * (a(0, 0) * a(0, 0) + a(0, 1) * a(1, 0) + a(0, 2) * a(2, 0) + a(1, 0) * a(0, 1) + a(1, 1) * a(1, 1) + a(1, 2) * a(2, 1) +
                 a(2, 0) * a(0, 2) + a(2, 1) * a(1, 2) + a(2, 2) * a(2, 2)).real
    zero = (c0 == 0) & (c1 == 0)                           # the cold-start branch: exp(0) = 1
    c1s = np.where(zero, 1.0, c1)
    neg = c0 < 0
    c0 = np.abs(c0)
    fac_1_3 = 1 / 3.0
    c0max = 2.0 * np.power(fac_1_3 * c1s, 1.5)
    theta_3 = fac_1_3 * np.arccos(np.minimum(c0 / c0max, 1.0))
    u = np.sqrt(fac_1_3 * c1s) * np.cos(theta_3)
    w = np.sqrt(c1s) * np.sin(theta_3)
    ma = np.exp(2j * u)
    mb = np.exp(-1j * u)
    cw = np.cos(w)
    u2, w2 = u * u, w * w
    with np.errstate(divide="ignore", invalid="ignore"):
        xi0 = np.where(w > 0.05, np.sin(w) / w, 1 - 0.16666666666666667 * w2 * (1 - 0.05 * w2 * (1 - 0.023809523809523808 * w2)))
    divisor = 1.0 / (9.0 * u2 - w2)
    f0 = divisor * (ma * (u * u - w * w) + mb * (8 * u * u * cw + 2j * u * (3 * u * u + w * w) * xi0))
    f1 = divisor * (-2j * u * ma + mb * (2j * u * cw + (3 * u * u - w * w) * xi0))
    f2 = divisor * (mb * (cw + 3j * u * xi0) - ma)
    f0, f1, f2 = [np.where(neg, np.conj(f), f) for f in (f0, f1, f2)]
    eye = np.eye(3, dtype=complex)
    tmp = f2[..., None, None] * A + f1[..., None, None] * eye          # exponent_from_coefficients, :36-43
    out = tmp @ A + f0[..., None, None] * eye
    return np.where(zero[..., None, None], eye, out)


def staples(U, mu):
    """get_staples.c:34-69 for every site: per k != mu the staple above, then the one below"""
    st = np.zeros_like(U[..., mu, :, :])
    for k in range(4):
        if k == mu:
            continue
        for p in PLAQUETTE_PATHS:
            st = st + path_product(U, mu, k, p)
    return st


def step_gradient_flow_c(U, eps):
    """gradient_flow.c:52-130 on a complex [T][LX][LY][LZ][4][3][3] field"""
    Z = None
    for f in range(3):
        new = np.empty_like(U)
        znew = np.empty_like(U)
        for mu in range(4):
            z_tmp = project_traceless_antiherm(staples(U, mu) @ _dag(U[..., mu, :, :]))
            if f == 0:
                z = eps * z_tmp
            else:
                z = (eps * ZFAC[2 * f - 1]) * z_tmp
                z = z + ZFAC[2 * f] * Z[..., mu, :, :]
            znew[..., mu, :, :] = z
            w = cayley_hamilton_exponent(project_traceless_antiherm(ZEPSFAC[f] * z))
            new[..., mu, :, :] = w @ U[..., mu, :, :]
        U, Z = new, znew
    return U


def step_gradient_flow(g, dims, eps, nsteps=1):
    """nsteps steps on a [V][4][3][3][2] field; returns the flowed field in the same layout"""
    U = to_complex(g, dims)
    for _ in range(nsteps):
        U = step_gradient_flow_c(U, eps)
    return from_complex(U)


def _tr(a, b):
    """_trace_su3_times_su3 (su3.h:667-676) assigned to a double: Re tr(a b)"""
    return np.einsum("...ij,...ji->...", a, b).real


def field_strength_sites(g, dims):
    """Per-site sums before normalisation: (sum over planes of tr(G_kl G_kl), sum of the Levi-Civita terms), each [T][LX][LY][LZ]"""
    U = to_complex(g, dims)
    G = {}
    e = 0.0
    for k, l in PLANES:
        leaf = 0.0
        for p in LEAF_PATHS:
            leaf = leaf + path_product(U, k, l, p)
        G[(k, l)] = project_traceless_antiherm(leaf)
        e = e + _tr(G[(k, l)], G[(k, l)])
    q = 0.0
    for sign, p1, p2 in EPS_TERMS:
        q = q + sign * _tr(G[p1], G[p2])
    return e, q


def field_strength(g, dims):
    """(E, Q) of measure_clover_field_strength_observables"""
    e, q = field_strength_sites(g, dims)
    V = int(np.prod(dims))
    return E_NORM(V) * float(e.sum()), Q_NORM * float(q.sum())


def sum_abs_q(g, dims):
    """sum over sites of |the site's contribution to Q|: the scale of Q's rounding error"""
    _, q = field_strength_sites(g, dims)
    return float(np.abs(Q_NORM * q).sum())


def observables(g, dims):
    """(P, E, Q) as the measurement loop takes them: P = measure_plaquette / (6 VOLUME)"""
    V = int(np.prod(dims))
    e, q = field_strength(g, dims)
    return measure_plaquette(g, dims) / (6.0 * V), e, q


def gradient_flow(g, dims, eps, tmax):
    """The loop of gradient_flow_measurement (gradient_flow.c:172-222): [n][8] rows t P Eplaq Esym tsqEplaq tsqEsym Wsym Qsym"""
    t, P, E, Q = [0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3
    P[2], E[2], Q[2] = observables(g, dims)
    rows = []
    while t[1] < tmax:
        t[0], E[0], Q[0], P[0] = t[2], E[2], Q[2], P[2]
        for step in (1, 2):
            t[step] = t[step - 1] + eps
            g = step_gradient_flow(g, dims, eps)
            P[step], E[step], Q[step] = observables(g, dims)
        W = t[1] * t[1] * (2 * E[1] + t[1] * ((E[2] - E[0]) / (2 * eps)))
        tsqE = t[1] * t[1] * E[1]
        rows.append([t[1], P[1], 36 * (1 - P[1]), E[1], t[1] * t[1] * 36 * (1 - P[1]), tsqE, W, Q[1]])
    return np.array(rows).reshape(-1, 8)


GRADFLOW_HEADER = "traj t P Eplaq Esym tsqEplaq tsqEsym Wsym Qsym\n"


def gradflow_text(traj, rows):
    """The file gradient_flow_measurement writes (gradient_flow.c:159, :210-219), trailing space included"""
    out = GRADFLOW_HEADER
    for r in rows:
        out += "%06d %f %2.12f %2.12f %2.12f %2.12f %2.12f %2.12f %.12f \n" % ((traj,) + tuple(r))
    return out


def random_antiherm(seed, n, scale=1.0):
    """n random traceless anti-hermitian 3x3 matrices"""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, 3, 3)) + 1j * rng.standard_normal((n, 3, 3))
    return project_traceless_antiherm(scale * m)


__all__ = ["cayley_hamilton_exponent", "expm_su3", "field_strength", "gradient_flow", "observables", "project_traceless_antiherm",
           "step_gradient_flow", "sum_abs_q"]
