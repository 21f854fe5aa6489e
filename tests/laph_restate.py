"""TEST INFRASTRUCTURE ONLY: the gauge-covariant 3D Laplacian of the reference's jacobi.c restated in NumPy.

    l(x) = 6 k(x) - sum_{mu=1..3} [ U_mu(x) k(x+mu) + U_mu(x-mu)^dagger k(x-mu) ]

on one time-slice: the raw links of the lexicographic gauge field ([VOLUME][4][3][3][2], site = t SPACEVOLUME + ix), no boundary
phases, no kappa; neighbours wrap inside the slice (ix = (x LY + y) LZ + z, geometry_eo.c:851-860), and with an extent of 2 the two
neighbours are one site and both terms count.  The subtractions are made in the reference's order.  A colour vector is complex128
[SPACEVOLUME][3]; a colour-vector field float64 [T][SPACEVOLUME][3][2] on the host.  tests/test_laph_restate.py pins this file to the
reference's object code (tests/golden/ref_laph_*.npz).  No GPU or torch dependency.
"""
import numpy as np


def cplx(a):
    """float64 [...][2] -> complex128 [...]"""
    return np.ascontiguousarray(a[..., 0] + 1j * a[..., 1])


def reals(z):
    """complex128 [...] -> float64 [...][2]"""
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def neighbours(LX, LY, LZ):
    """(up, dn): int [3][SPACEVOLUME], g_iup3d / g_idn3d for mu = 1, 2, 3"""
    x, y, z = np.meshgrid(np.arange(LX), np.arange(LY), np.arange(LZ), indexing="ij")
    idx = lambda a, b, c: ((a % LX) * LY + (b % LY)) * LZ + (c % LZ)
    up = np.stack([idx(x + 1, y, z), idx(x, y + 1, z), idx(x, y, z + 1)]).reshape(3, -1)
    dn = np.stack([idx(x - 1, y, z), idx(x, y - 1, z), idx(x, y, z - 1)]).reshape(3, -1)
    return up, dn


def slice_links(gauge, dims, t):
    """the spatial links of time-slice t: complex128 [3][SPACEVOLUME][3][3]"""
    T, LX, LY, LZ = dims
    S3 = LX * LY * LZ
    return cplx(gauge[t * S3:(t + 1) * S3, 1:4]).transpose(1, 0, 2, 3)


def jacobi(gauge, dims, k, t):
    """Jacobi(l, k, t) of jacobi.c:43-72; k: complex128 [SPACEVOLUME][3] -> l of the same shape"""
    T, LX, LY, LZ = dims
    up, dn = neighbours(LX, LY, LZ)
    U = slice_links(gauge, dims, t)
    l = 6.0 * k
    for mu in range(3):
        l = l - np.einsum("xab,xb->xa", U[mu], k[up[mu]])
        l = l - np.einsum("xba,xb->xa", np.conj(U[mu][dn[mu]]), k[dn[mu]])
    return l


def apply_field(gauge, dims, field, t0=0, nt=None):
    """the operator on the slices [t0, t0 + nt) of a host colour-vector field (float64 [T][SPACEVOLUME][3][2]); the others come back zero"""
    nt = dims[0] - t0 if nt is None else nt
    out = np.zeros_like(field)
    for t in range(t0, t0 + nt):
        out[t] = reals(jacobi(gauge, dims, cplx(field[t]), t))
    return out


def dense(gauge, dims, t):
    """the matrix of time-slice t, complex128 [3 SPACEVOLUME][3 SPACEVOLUME], row = 3 ix + colour"""
    T, LX, LY, LZ = dims
    S3 = LX * LY * LZ
    up, dn = neighbours(LX, LY, LZ)
    U = slice_links(gauge, dims, t)
    A = np.zeros((S3, 3, S3, 3), dtype=np.complex128)
    ix = np.arange(S3)
    for a in range(3):
        A[ix, a, ix, a] += 6.0
    for mu in range(3):
        for a in range(3):
            for b in range(3):
                np.add.at(A, (ix, a, up[mu], b), -U[mu][:, a, b])
                np.add.at(A, (ix, a, dn[mu], b), -np.conj(U[mu][dn[mu]][:, b, a]))
    return A.reshape(3 * S3, 3 * S3)


def gauge_transform(gauge, dims, omega):
    """U_mu(x) -> Omega(x) U_mu(x) Omega(x+mu)^dagger on the spatial links of every slice; omega: float64 [VOLUME][3][3][2]"""
    T, LX, LY, LZ = dims
    S3 = LX * LY * LZ
    up, _ = neighbours(LX, LY, LZ)
    W = cplx(omega)
    out = gauge.copy()
    for t in range(T):
        Wt = W[t * S3:(t + 1) * S3]
        for mu in range(3):
            U = cplx(gauge[t * S3:(t + 1) * S3, mu + 1])
            out[t * S3:(t + 1) * S3, mu + 1] = reals(np.einsum("xab,xbc,xdc->xad", Wt, U, np.conj(Wt[up[mu]])))
    return out


def scale_slice_toward_unity(gauge, dims, t, s):
    """the spatial links of slice t replaced by (1 - s) 1 + s U: a smoother slice, whose lowest eigenvalues separate faster"""
    S3 = dims[1] * dims[2] * dims[3]
    out = gauge.copy()
    one = np.zeros((3, 3, 2))
    one[np.arange(3), np.arange(3), 0] = 1.0
    out[t * S3:(t + 1) * S3, 1:4] = (1.0 - s) * one + s * gauge[t * S3:(t + 1) * S3, 1:4]
    return out
