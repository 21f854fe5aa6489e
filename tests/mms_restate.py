"""TEST INFRASTRUCTURE ONLY: solver/cg_mms_tm.c:65-197 restated statement by statement in complex128 NumPy, over any operator
callable A(x) -> M_psi x on complex [N][4][3] fields (use nd_restate.cplx / real to convert from / to the reference layout).
No GPU or torch dependency.  Returns what the reference leaves behind: the return value, *cgmms_reached_prec, the solutions,
the drop schedule [[iteration, shifts remaining], ...] (the g_debug_level > 2 lines of :150-152) and the shifts left."""
import numpy as np


def _sq(x):
    return float(np.sum(x.real * x.real + x.imag * x.imag))


def _dot(a, b):
    return float(np.sum(a.real * b.real + a.imag * b.imag))


def cg_mms_tm(A, Q, shifts, max_iter, eps_sq, rel_prec):
    no_shifts = len(shifts)
    P = [np.zeros_like(Q) for _ in shifts]                                   # :85,94
    alphas, betas = np.ones(no_shifts), np.zeros(no_shifts)
    zita, zitam1 = np.ones(no_shifts), np.ones(no_shifts)
    sigma = np.zeros(no_shifts)
    sigma[0] = shifts[0] * shifts[0]                                         # :88
    for im in range(1, no_shifts):
        sigma[im] = shifts[im] * shifts[im] - sigma[0]                      # :91
    ps = [None] + [Q.copy() for _ in range(1, no_shifts)]                    # :96
    squarenorm = _sq(Q)
    r, p = Q.copy(), Q.copy()                                                # :107-108
    normsq = squarenorm
    drops, err, reached = [], 0.0, None
    iteration = 0
    for iteration in range(max_iter):
        Ap = A(p) + sigma[0] * p                                             # :115-117
        pro = _dot(p, Ap)                                                    # :118
        alpham1 = alphas[0]
        alphas[0] = normsq / pro
        im = 1
        while im < no_shifts:                                                # :126-155
            gamma = zita[im] * alpham1 / (alphas[0] * betas[0] * (1. - zita[im] / zitam1[im]) + alpham1 * (1. + sigma[im] * alphas[0]))
            zitam1[im] = zita[im]
            zita[im] = gamma
            alphas[im] = alphas[0] * zita[im] / zitam1[im]
            P[im] = P[im] + alphas[im] * ps[im]
            if iteration > 0 and iteration % 20 == 0 and im == no_shifts - 1:
                sn = _sq(ps[im])
                if alphas[no_shifts - 1] * alphas[no_shifts - 1] * sn <= eps_sq:
                    no_shifts -= 1
                    drops.append([iteration, no_shifts])
            im += 1
        P[0] = P[0] + alphas[0] * p                                          # :158
        r = r + (-alphas[0]) * Ap                                            # :160
        err = _sq(r)
        if (err <= eps_sq and rel_prec == 0) or (err <= eps_sq * squarenorm and rel_prec > 0) or iteration == max_iter - 1:
            reached = err
            break
        betas[0] = err / normsq                                              # :180
        p = betas[0] * p + r
        normsq = err
        for im in range(1, no_shifts):                                       # :186-189
            betas[im] = betas[0] * zita[im] * alphas[im] / (zitam1[im] * alphas[0])
            ps[im] = betas[im] * ps[im] + zita[im] * r
    ret = -1 if iteration == max_iter - 1 else iteration + 1                # :193-194
    return ret, reached, P, drops, no_shifts
