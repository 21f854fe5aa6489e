"""TEST INFRASTRUCTURE ONLY: the gauge monomial of the reference restated in NumPy.

gauge_derivative / gauge_EMderivative (monomial/gauge_monomial.c:48-162) with get_staples.c and get_rectangle_staples.c,
measure_plaquette / measure_gauge_action (measure_gauge_action.c:46-189) and measure_rectangles (measure_rectangles.c:51-140), over a
lexicographic [V][4][3][3][2] float64 field for any T, LX, LY, LZ (extent 2 included, where x + mu == x - mu: shifts are np.roll).
A staple is written as the path of links it walks from x to x + mu; `t_slab=(t0, t1)` restricts the outputs to the time-slices
[t0, t1) of the full lattice (what one rank of a T split owns)."""
import numpy as np

# step codes of a path: +nu, -nu, +mu, -mu
PN, MN, PM, MM = 0, 1, 2, 3
PLAQUETTE_PATHS = ((PN, PM, MN), (MN, PM, PN))                                         # get_staples.c: above, below
RECTANGLE_PATHS = ((PN, PN, PM, MN, MN), (MN, MN, PM, PN, PN), (PN, PM, PM, MN, MM),   # get_rectangle_staples.c, in its order
                   (MN, PM, PM, PN, MM), (MM, MN, PM, PM, PN), (MM, PN, PM, PM, MN))


def to_complex(g, dims):
    """[V][4][3][3][2] float64 -> complex [T][LX][LY][LZ][4][3][3]"""
    T, LX, LY, LZ = dims
    g = np.asarray(g)[:T * LX * LY * LZ]
    return (g[..., 0] + 1j * g[..., 1]).reshape(T, LX, LY, LZ, 4, 3, 3)


def _at(f, shift):
    """f(x + shift) as a field of x"""
    for ax, s in enumerate(shift):
        if s:
            f = np.roll(f, -s, axis=ax)
    return f


def _dag(m):
    return np.conj(np.swapaxes(m, -1, -2))


def path_product(U, mu, nu, path):
    """Ordered product of links along `path` starting at every site x"""
    pos = [0, 0, 0, 0]
    out = None
    for c in path:
        d = mu if c & 2 else nu
        if c & 1:
            pos[d] -= 1
            l = _dag(_at(U[..., d, :, :], pos))
        else:
            l = _at(U[..., d, :, :], pos)
            pos[d] += 1
        out = l if out is None else out @ l
    return out


def trace_lambda(w):
    """su3adj.h:164-172 without the factor: [..., 3, 3] complex -> [..., 8]"""
    im, re = w.imag, w.real
    return np.stack([-im[..., 1, 0] - im[..., 0, 1], re[..., 1, 0] - re[..., 0, 1], -im[..., 0, 0] + im[..., 1, 1],
                     -im[..., 2, 0] - im[..., 0, 2], re[..., 2, 0] - re[..., 0, 2], -im[..., 2, 1] - im[..., 1, 2],
                     re[..., 2, 1] - re[..., 1, 2], (-im[..., 0, 0] - im[..., 1, 1] + 2.0 * im[..., 2, 2]) * 0.577350269189625], axis=-1)


def _slab(a, dims, t_slab):
    if t_slab is None:
        return a
    return a[t_slab[0]:t_slab[1]]


def gauge_derivative(g, dims, beta, c0=1.0, c1=0.0, use_rectangles=False, glambda=0.0, t_slab=None):
    """The contribution gauge_derivative (glambda = 0) / gauge_EMderivative adds to hf->derivative: [V or slab sites][4][8]"""
    U = to_complex(g, dims)
    factor = -c0 * beta / 3.0 if use_rectangles else -beta / 3.0
    out = np.zeros(U.shape[:4] + (4, 8))
    for mu in range(4):
        z = U[..., mu, :, :]
        st = np.zeros_like(z)
        for k in range(4):
            if k == mu:
                continue
            w = (1.0 + glambda) if (k == 0 or mu == 0) else (1.0 - glambda)
            for p in PLAQUETTE_PATHS:
                st = st + w * path_product(U, mu, k, p)
        out[..., mu, :] += factor * trace_lambda(z @ _dag(st))
        if use_rectangles:
            st = np.zeros_like(z)
            for nu in range(4):
                if nu == mu:
                    continue
                for p in RECTANGLE_PATHS:
                    st = st + path_product(U, mu, nu, p)
            out[..., mu, :] += (factor * c1 / c0) * trace_lambda(z @ _dag(st))
    return _slab(out, dims, t_slab).reshape(-1, 4, 8)


def _plaq_field(U, mu1, mu2):
    """Re tr( U_mu1(x) U_mu2(x+mu1) [U_mu2(x) U_mu1(x+mu2)]^dagger ) per site"""
    e1, e2 = [0] * 4, [0] * 4
    e1[mu1], e2[mu2] = 1, 1
    p1 = U[..., mu1, :, :] @ _at(U[..., mu2, :, :], e1)
    p2 = U[..., mu2, :, :] @ _at(U[..., mu1, :, :], e2)
    return np.einsum("...ij,...ij->...", p1, np.conj(p2)).real


def measure_gauge_action(g, dims, glambda=0.0, t_slab=None):
    U = to_complex(g, dims)
    s = 0.0
    for mu1 in range(3):
        for mu2 in range(mu1 + 1, 4):
            w = (1.0 + glambda) if mu1 == 0 else (1.0 - glambda)
            s += w * _slab(_plaq_field(U, mu1, mu2), dims, t_slab).sum()
    return s / 3.0


def measure_plaquette(g, dims, t_slab=None):
    return measure_gauge_action(g, dims, 0.0, t_slab)


def measure_rectangles(g, dims, t_slab=None):
    U = to_complex(g, dims)
    s = 0.0
    for mu in range(4):
        for nu in range(4):
            if nu == mu:
                continue
            p1 = path_product(U, nu, mu, (PN, PM, PM))      # U_mu(x) U_nu(x+mu) U_nu(x+mu+nu)   (here "nu" of the path is mu)
            p2 = path_product(U, mu, nu, (PN, PN, PM))      # U_nu(x) U_nu(x+nu) U_mu(x+2nu)
            s += _slab(np.einsum("...ij,...ij->...", p1, np.conj(p2)).real, dims, t_slab).sum()
    return s / 3.0


def gauge_energy(g, dims, beta, c0=1.0, c1=0.0, use_rectangles=False, glambda=0.0):
    """gauge_heatbath / gauge_acc: beta (c0 S_plaq + c1 S_rect)"""
    e = beta * c0 * measure_gauge_action(g, dims, glambda)
    if use_rectangles:
        e += beta * c1 * measure_rectangles(g, dims)
    return e


def seed_derivative(V, seed=4711):
    """The non-zero derivative field the fixtures start from"""
    return np.random.default_rng(seed).standard_normal((V, 4, 8))


def checksums(df):
    """Order-sensitive sums of a derivative field (for fixtures too large to store): plain, squared, weighted by a seeded vector"""
    w = np.random.default_rng(99).standard_normal(df.shape)
    return {"sum": float(df.sum()), "sum_sq": float((df * df).sum()), "weighted": float((df * w).sum())}


# ---- the update of the reference restated, for the CPU leapfrog of the tests (update_gauge.c:51-110, expo.c) ----
def make_su3(p):
    """su3adj [..., 8] -> anti-hermitian traceless [..., 3, 3] (_make_su3, su3adj.h:45-54)"""
    d1, d2, d3, d4, d5, d6, d7, d8 = [p[..., k] for k in range(8)]
    r3 = 0.5773502691896258
    v = np.zeros(p.shape[:-1] + (3, 3), dtype=complex)
    v[..., 0, 0] = 1j * (r3 * d8 + d3); v[..., 0, 1] = d2 + 1j * d1; v[..., 0, 2] = d5 + 1j * d4
    v[..., 1, 0] = -d2 + 1j * d1; v[..., 1, 1] = 1j * (r3 * d8 - d3); v[..., 1, 2] = d7 + 1j * d6
    v[..., 2, 0] = -d5 + 1j * d4; v[..., 2, 1] = -d7 + 1j * d6; v[..., 2, 2] = -1j * 2.0 * r3 * d8
    return v


def expm_su3(v, order=24):
    out = np.broadcast_to(np.eye(3, dtype=complex), v.shape).copy()
    term = out.copy()
    for k in range(1, order + 1):
        term = term @ v / k
        out = out + term
    return out


def update_gauge(g, mom, step):
    """U <- exp(step P) U for every link; g [V][4][3][3][2], mom [V][4][8]; returns the new field"""
    U = g[..., 0] + 1j * g[..., 1]
    U = expm_su3(make_su3(step * mom)) @ U
    out = np.empty_like(g)
    out[..., 0], out[..., 1] = U.real, U.imag
    return out
