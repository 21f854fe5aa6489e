"""NumPy restatement of the chronological solver guess (solver/chrono_guess.c, solver/lu_solve.c of the reference) on complex128
fields [N][4][3].  tests/test_csg_restate.py pins it to the reference's own outputs (tests/golden/ref_csg_4x4.npz); the GPU tests at
shapes without a fixture rest on it."""
import numpy as np

SPINOR_SEED, NRHS = 20261019, 6


def rhs_fields(Vh, nrhs=NRHS, seed=SPINOR_SEED):
    """The right-hand sides of the fixtures (tools/make_golden_csg.py) as float64 [Vh][4][3][2]: b_k = phi0 + 0.1 k d + 0.1 r_k with
    independent random r_k, so that the solutions span as many dimensions as a list holds vectors."""
    rng = np.random.default_rng(seed)
    phi0, d = rng.standard_normal((Vh, 4, 3, 2)), rng.standard_normal((Vh, 4, 3, 2))
    r = [rng.standard_normal((Vh, 4, 3, 2)) for _ in range(nrhs)]
    return [phi0 + 0.1 * k * d + 0.1 * r[k] for k in range(nrhs)]


def dot(s, r):
    """sum conj(s) r"""
    return complex(np.vdot(s, r))


def orthogonalise(vs):
    """the vectors older than the newest lose their component along it (in place); vs oldest first"""
    new = vs[-1]
    for i in range(len(vs) - 2, -1, -1):
        vs[i] -= dot(new, vs[i]) * new


def projections(A, vs, phi):
    """(G, bn): G[i][j] = <v_i, A v_j> from the upper triangle, mirrored below it; bn[j] = <v_j, phi>"""
    n = len(vs)
    G = np.zeros((n, n), dtype=np.complex128)
    bn = np.zeros(n, dtype=np.complex128)
    for j in range(n):
        w = A(vs[j])
        for i in range(j + 1):
            G[i, j] = dot(vs[i], w)
            if i != j:
                G[j, i] = np.conj(G[i, j])
        bn[j] = dot(vs[j], phi)
    return G, bn


def lu_solve(G, b):
    """y with G y = b: row-wise LU, unit lower factor; row 0 stays, every later row i first changes place with the row below it
    that has the largest |entry|^2 in column i as it stands (strictly larger wins), right-hand side included"""
    M = np.array(G, dtype=np.complex128)
    rhs = np.array(b, dtype=np.complex128)
    n = len(rhs)
    for i in range(1, n):
        size = np.abs(M[i:, i]) ** 2
        best = i + int(np.argmax(size))        # argmax returns the first of equal maxima, as the strict comparison does
        if best != i:
            M[[i, best]] = M[[best, i]]
            rhs[[i, best]] = rhs[[best, i]]
        for j in range(n):
            upto = min(i, j)
            M[i, j] -= M[i, :upto] @ M[:upto, j]
            if j < i:
                M[i, j] /= M[j, j]
    y = np.zeros(n, dtype=np.complex128)
    for i in range(n):
        y[i] = rhs[i] - M[i, :i] @ y[:i]
    x = np.zeros(n, dtype=np.complex128)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - M[i, i + 1:] @ x[i + 1:]) / M[i, i]
    return x


def combine(vs, y):
    """sum_i y_i v_i, newest vector first"""
    out = y[-1] * vs[-1]
    for i in range(len(vs) - 2, -1, -1):
        out = out + y[i] * vs[i]
    return out


def chrono_guess(A, vs, phi):
    """-> (trial, G, bn, y); vs (oldest first) is orthogonalised in place; an empty list gives a zero trial vector"""
    if not vs:
        return np.zeros_like(phi), np.zeros((0, 0), dtype=np.complex128), np.zeros(0, dtype=np.complex128), np.zeros(0, dtype=np.complex128)
    orthogonalise(vs)
    G, bn = projections(A, vs, phi)
    y = lu_solve(G, bn)
    return combine(vs, y), G, bn, y


def add_solution(index_array, n, N):
    """the bookkeeping of chrono_add_solution: -> (slot the normalised solution goes to, new n); index_array is updated in place"""
    if N <= 0:
        return None, n
    if n < N:
        index_array[n] = n
        n += 1
        return index_array[n - 1], n
    for i in range(1, N):
        index_array[i - 1] = index_array[i]
    index_array[N - 1] = (index_array[N - 2] + 1) % N if N > 1 else 0
    return index_array[N - 1], n


def normalised(x):
    return x / np.sqrt(np.vdot(x, x).real)
