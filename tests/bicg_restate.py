"""NumPy restatement of BiCGstab (solver/bicgstab_complex.c:49-116 of the reference) on complex128 fields, over any operator A(x).
tests/test_bicg_restate.py pins it to the reference's own outputs (tests/golden/ref_bicg_*, tools/make_golden_bicg.py) with the
operators of the CPU oracle; `operator` below builds those, `case_setup` the oracle and the fields of a fixture case."""
import numpy as np

from oracle.nd_restate import cplx, real

SPINOR_SEED = 20261019
# iteration counts are pinned for KIND_M only: on the indefinite KIND_Q operators the count moves with the last bits of the reductions
KIND_M = ("Mtm_plus_psi", "Mtm_minus_psi", "Mtm_plus_sym_psi", "Mtm_minus_sym_psi", "Msw_plus_psi", "D_psi")
KIND_Q = ("Qtm_plus_psi", "Qtm_minus_psi", "Qsw_plus_psi", "Qsw_minus_psi")
CLOVER = ("Qsw_plus_psi", "Qsw_minus_psi", "Msw_plus_psi")


def fields(V, seed=SPINOR_SEED):
    """The sources and the starting guess of the fixtures as float64 [n][4][3][2]: q_eo, q_full, p0_eo"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V // 2, 4, 3, 2)), rng.standard_normal((V, 4, 3, 2)), 0.1 * rng.standard_normal((V // 2, 4, 3, 2))


def bicgstab_complex(A, P, Q, max_iter, eps_sq, rel_prec, noise=None):
    """Returns (the reference's return value, the solution, |r|^2 at the top of every iteration run).  noise: a function that
    perturbs a scalar product (the sensitivity runs of the fixtures' generator)."""
    dot = (lambda a, b: complex(np.vdot(a, b))) if noise is None else (lambda a, b: noise(complex(np.vdot(a, b))))
    P = P.copy()
    r = A(P)
    p = Q - r
    r = p.copy()
    hatr = p.copy()
    rho0 = dot(hatr, r)
    squarenorm = dot(Q, Q).real
    hist = []
    for i in range(max_iter):
        err = dot(r, r).real
        hist.append(err)
        if (((err <= eps_sq) and rel_prec == 0) or ((err <= eps_sq * squarenorm) and rel_prec == 1)) and i > 0:
            return i, P, hist
        v = A(p)
        alpha = rho0 / dot(hatr, v)
        s = r - alpha * v
        t = A(s)
        omega = dot(t, s) / dot(t, t).real
        P += alpha * p + omega * s
        r = s - omega * t
        rho1 = dot(hatr, r)
        if abs(rho1.real) < 1e-25 and abs(rho1.imag) < 1e-25:
            return -1, P, hist
        beta = (alpha * rho1) / (omega * rho0)
        p = r + beta * (p - omega * v)
        rho0 = rho1
    return -1, P, hist


def operator(orc, name):
    """A(x) on complex fields over the CPU oracle (oracle/oraclebind.py): the e/o operators on [V/2][4][3], D_psi on [V][4][3]"""
    n = orc.V if name == "D_psi" else orc.Vh

    def A(x):
        l = np.zeros((n, 4, 3, 2))
        if name == "D_psi":
            orc.D_psi(l, real(x))
        else:
            orc.op(name, l, real(x))
        return cplx(l)
    return A


def oracle_for(dims, gauge, kappa, c_sw, case):
    from oracle.oraclebind import Oracle
    orc = Oracle(*dims, kappa=kappa, mu=case["g_mu"])
    orc.set_gauge(np.ascontiguousarray(gauge))
    if case["op"] in CLOVER:
        sw = orc.sw_term(kappa, c_sw)
        swi, fails = orc.sw_invert(sw, 0, case["g_mu"])
        assert fails == 0
        orc.set_clover(sw, swi)
    return orc


def case_fields(case, V):
    """(Q, P0) of a fixture case as float64 arrays"""
    q_eo, q_full, p0 = fields(V)
    full = case["op"] == "D_psi"
    Q = q_full if full else q_eo
    P0 = p0 if case["guess"] else np.zeros_like(Q)
    return Q, P0


def bound_of(case, Q):
    return case["eps_sq"] * (float(np.sum(Q ** 2)) if case["rel_prec"] == 1 else 1.0)
