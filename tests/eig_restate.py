"""TEST INFRASTRUCTURE ONLY: the eigensolver of tmlqcd_amd/csrc/eig.hip restated in NumPy over any callable operator.

Thick-restart Lanczos (Wu and Simon) with full reorthogonalisation (classical Gram-Schmidt, twice) for the nev lowest or
highest eigenpairs of a Hermitian positive operator A(x) -> y on flat complex128 vectors, with the optional Chebyshev
filter of the lowest end: the same basis size, restart rule, interval rule, convergence test (true residual with A) and
operator-application cap as the device driver, so that the two can be compared run for run from one start vector.  The
small symmetric eigenproblem is numpy.linalg.eigh.  tests/test_eig_restate.py pins this file to numpy.linalg.eigvalsh of
the dense matrix.  No GPU or torch dependency.
"""
import numpy as np


class _Run:
    def __init__(self, A, max_apps):
        self.A, self.apps, self.max_apps = A, 0, max_apps

    def apply(self, x):
        self.apps += 1
        return self.A(x)

    def filtered(self, x, deg, lo, hi):
        """B x, B = A (deg 0) or T_deg((hi + lo - 2 A) / (hi - lo))"""
        if deg <= 0:
            return self.apply(x)
        a, c = -2.0 / (hi - lo), (hi + lo) / (hi - lo)
        tprev, tcur = x, a * self.apply(x) + c * x
        for _ in range(2, deg + 1):
            tprev, tcur = tcur, 2.0 * (a * self.apply(tcur) + c * tcur) - tprev
        return tcur

    def residuals(self, V, cnt):
        theta, res = np.zeros(cnt), np.zeros(cnt)
        for i in range(cnt):
            y = self.apply(V[i])
            t = np.vdot(V[i], y)
            theta[i] = t.real
            res[i] = np.linalg.norm(y - t * V[i])
        return theta, res


def _lanczos(run, V, m, nev, largest, deg, lo, hi, prec, one_cycle):
    """One run from the unit start vector V[0].  Returns (got, theta, res, converged, ritz, ritz_res, keep)."""
    T = np.zeros((m, m))
    k, anorm = 0, 0.0
    cost = deg if deg > 0 else 1
    fresh, theta, res, conv = False, None, None, 0       # fresh: theta / res are the computed residuals of V[:got] as they stand
    while True:
        length, broke, capped, beta = k, False, False, 0.0
        for j in range(k, m):
            if run.apps + cost + nev > run.max_apps:
                capped = True
                break
            w = run.filtered(V[j], deg, lo, hi)
            B = V[:j + 1]
            h = np.conj(B @ np.conj(w))          # <v_i, w> without a conjugated copy of the basis
            w = w - h @ B
            h2 = np.conj(B @ np.conj(w))
            w = w - h2 @ B
            h = h + h2
            n2 = np.vdot(w, w).real
            T[j, j] = h[j].real
            beta = np.sqrt(n2)
            anorm = max(anorm, np.sqrt(n2 + np.sum(np.abs(h) ** 2)))
            length = j + 1
            if not beta > 1e-14 * anorm:
                broke, beta = True, 0.0
                break
            V[j + 1] = w / beta
            if j + 1 < m:
                T[j, j + 1] = T[j + 1, j] = beta
        if length == k and capped:
            got = min(nev, max(k, 1))
            if one_cycle:
                return got, None, None, 0, np.zeros(0), np.zeros(0), 0
            if not fresh:                                  # else the restart before has just computed them: the cap includes them
                theta, res = run.residuals(V, got)
                conv = int(np.sum(res <= prec))
            return got, theta, res, conv, None, None, 0
        th, S = np.linalg.eigh(T[:length, :length])
        rres = np.abs(beta * S[length - 1])
        keep = min(nev + (m - nev) // 2, m - 2, length - 1)
        keep = max(keep, 1)
        keep_rule = keep
        last = broke or capped or one_cycle
        if last and keep < min(nev, length):
            keep = min(nev, length)
        cols = [length - 1 - q if largest else q for q in range(keep)]
        est_ok = all(rres[c] <= prec for c in cols[:min(nev, keep)])
        V[:keep] = S[:, cols].T @ V[:length]
        got = min(nev, keep)
        if one_cycle:
            return got, None, None, 0, th, rres, keep_rule
        if last or deg > 0 or est_ok:
            theta, res = run.residuals(V, got)
            conv = int(np.sum(res <= prec))
            fresh = True
            if conv == nev or last:
                return got, theta, res, conv, None, None, 0
        else:
            fresh = False
        V[keep] = V[length]
        T[:] = 0.0
        for q, c in enumerate(cols):
            T[q, q] = th[c]
            T[q, keep] = T[keep, q] = beta * S[length - 1, c]
        k = keep


def eigenvalues(A, start, nev, which=0, prec=1e-8, max_apps=5000, m=24, cheb=0, interval=(0.0, 0.0)):
    """-> dict(evals, resid, converged, apps, vectors): the contract of tmhip_eigenvalues.  start: the start vector (any norm)."""
    assert nev >= 1 and nev + 2 <= m and max_apps >= nev + 1
    run = _Run(A, max_apps)
    V = np.zeros((m + 1, start.size), dtype=np.complex128)
    V[0] = start / np.linalg.norm(start)
    deg = cheb if which == 0 else 0
    lo, hi = interval
    if deg > 0 and not hi > lo:
        got, _, _, _, ritz, rres, keep = _lanczos(run, V, m, nev, False, 0, 0.0, 0.0, prec, True)
        if len(ritz) >= nev + 2:
            hi = 1.1 * (ritz[-1] + rres[-1])
            lo = ritz[min(keep, len(ritz)) - 1]
        if not hi > lo or len(ritz) < nev + 2:           # a cycle the cap cut short, or none at all: run unfiltered
            lo = hi = 0.0
        else:
            V[0] = V[:nev].sum(axis=0) / np.sqrt(nev)
    filtered = deg > 0 and hi > lo
    got, theta, res, conv, _, _, _ = _lanczos(run, V, m, nev, True if filtered else which == 1, deg if filtered else 0, lo, hi, prec, False)
    order = np.argsort(theta if which == 0 else -theta, kind="stable")
    evals, resid = np.full(nev, theta[order[-1]]), np.full(nev, np.inf)
    evals[:got], resid[:got] = theta[order], res[order]
    return {"evals": evals, "resid": resid, "converged": conv, "apps": run.apps, "vectors": V[:got][order].copy()}
