"""TEST INFRASTRUCTURE ONLY: the correction monomials restated in NumPy over the CPU oracle.

apply_Z_psi / apply_Z_ndpsi (monomial/ratcor_monomial.c:183-218, monomial/ndratcor_monomial.c:202-245) and the series loops of the
heatbath (:98-110, :110-123) and of the acceptance step (:151-168, :166-187), statement by statement, around the restated multi-shift
solvers (tests/mms_restate.py, oracle/nd_restate.py).  A field is a tuple of complex [N][4][3] arrays: one for the single-flavour
types, (up, dn) for the doublet.  The loops stop after six applications of Z, the length of the reference's coefficient tables.
"""
import numpy as np

from oracle import nd_restate as nd
from oracle.nd_restate import cplx, hop_over
from tests import mms_restate
from tests.util import TOL

TYPES = ("ratcor", "ndratcor", "cloverratcor", "ndcloverratcor")
HB_COEFS = [1. / 4., -3. / 32., 7. / 128., -77. / 2048., 231. / 8192., -1463. / 65536.]
ACC_COEFS = [-1. / 2., 3. / 8., -5. / 16., 35. / 128., -63. / 256., 231. / 1024.]


def gpu_bound(t, key, j=None):
    """the bound of the GPU tests for quantity `key` of type entry t of a scalars fixture (entry j of a list): 8 x the deviation this
    restatement has from the reference (`restate_vs_ref`, stored by tools/make_golden_ratcor.py, re-measured by
    tests/test_ratcor_restate.py), at least TOL"""
    d = t["restate_vs_ref"][key]
    return max(8.0 * (d if j is None else d[j]), TOL)


def _sq(f):
    return float(sum(np.sum(x.real * x.real + x.imag * x.imag) for x in f))


def _dot(a, b):
    return float(sum(np.sum(x.real * y.real + x.imag * y.imag) for x, y in zip(a, b)))


class RatCor:
    """orc: an Oracle made with mu = 0 and the scalars' kappa whose gauge field is set; name: one of TYPES; s: the scalars fixture
    (kappa, c_sw, mubar, epsbar, invmaxev)."""

    def __init__(self, orc, name, s):
        self.nd, self.sw = name.startswith("nd"), "clover" in name
        self.N = N = orc.Vh
        mb, eb, c = s["mubar"], s["epsbar"], s["invmaxev"]
        if self.nd:
            H = hop_over(orc.Hopping_Matrix, N)
            if self.sw:
                from tests import ndsw_restate as sw
                cl = sw.clover_of(orc, s["kappa"], s["c_sw"])
                cl.sw_invert_nd(mb * mb - eb * eb)
                self.Qsq = lambda f: sw.Qsw_pm_ndpsi(cl, H, f[0], f[1], mb, eb, c)
            else:
                self.Qsq = lambda f: nd.Qtm_pm_ndpsi(H, f[0], f[1], mb, eb, c)
        elif self.sw:
            from tests.cloverrat_restate import CloverRat
            m = CloverRat(orc, s["kappa"], s["c_sw"])
            assert m.fails == 0
            self.Qsq = lambda f: (m.Qsq(f[0]),)
        else:
            def q(f):
                buf, out = orc.new_field(), orc.new_field()
                buf[:N] = nd.real(f[0])
                orc.op("Qtm_pm_psi", out, buf)
                return (cplx(out[:N]),)
            self.Qsq = q

    def solve(self, src, c):
        """-> (return value of the solver, [chi_j as field tuples])"""
        if self.nd:
            it, P, _, _ = nd.cg_mms_tm_nd(lambda u, d: self.Qsq((u, d)), src[0], src[1], c["mu"], c["max_iter"], c["accprec"], c["rel_prec"])
            return it, [tuple(p) for p in P]
        it, _, P, _, _ = mms_restate.cg_mms_tm(lambda x: self.Qsq((x,))[0], src[0], c["mu"], c["max_iter"], c["accprec"], c["rel_prec"])
        return it, [(p,) for p in P]

    def apply_Z(self, l, c):
        """-> (k = Z l, delta, the first solve's return value)"""
        rmu, A = c["rmu"], c["A"]
        it0, chi = self.solve(l, c)
        k = tuple(x.copy() for x in l)
        for j in range(len(rmu) - 1, -1, -1):
            k = tuple(x + rmu[j] * y for x, y in zip(k, chi[j]))
        _, chi = self.solve(k, c)
        for j in range(len(rmu) - 1, -1, -1):
            k = tuple(x + rmu[j] * y for x, y in zip(k, chi[j]))
        t = tuple((A * A) * x for x in k)
        k = tuple(x - y for x, y in zip(self.Qsq(t), l))
        return k, _sq(k), it0

    def heatbath(self, eta, c):
        """-> (energy0, pf, applications of Z (-6: delta >= accprec after the sixth), deltas, summed first-solve return values)"""
        e0 = _sq(eta)
        pf, up0 = tuple(x.copy() for x in eta), eta
        deltas, iters = [], 0
        for i in range(1, 7):
            up1, delta, it0 = self.apply_Z(up0, c)
            deltas.append(delta)
            iters += it0
            pf = tuple(x + HB_COEFS[i - 1] * y for x, y in zip(pf, up1))
            if delta < c["accprec"]:
                return e0, pf, i, deltas, iters
            up0 = up1
        return e0, pf, -6, deltas, iters

    def acc(self, pf, c):
        """-> (energy1, applications of Z, deltas, summed first-solve return values, w_fields[4 (, 5)])"""
        up0, delta, iters = self.apply_Z(pf, c)
        deltas = [delta]
        w = tuple(x + ACC_COEFS[0] * y for x, y in zip(pf, up0))
        n = 1
        for i in range(2, 7):
            if delta < c["accprec"]:
                break
            up0, delta, it0 = self.apply_Z(up0, c)
            deltas.append(delta)
            iters += it0
            n = i
            w = tuple(x + ACC_COEFS[i - 1] * y for x, y in zip(w, up0))
        return _dot(pf, w), (n if delta < c["accprec"] else -6), deltas, iters, w


def deviations(rc, nd_, t, eta, arrs, name):
    """What tools/make_golden_ratcor.py stores as `restate_vs_ref` and tests/test_ratcor_restate.py measures again: fields relative to
    their largest element, scalars relative to their value.  t: the type's entry of the scalars file; arrs: the npz (None: scalars only)."""
    def frel(got, keys):
        return max(float(np.abs(nd.real(g) - arrs[k]).max() / np.abs(arrs[k]).max()) for g, k in zip(got, keys))

    def srel(a, b):
        return abs(a - b) / abs(b)
    sfx = ("_up", "_dn") if nd_ else ("_up",)
    dev, counts = {}, {}
    k, delta, it0 = rc.apply_Z(eta, t["arb"])
    dev["arb_delta"], counts["arb_iters"] = srel(delta, t["arb"]["delta"]), it0
    if arrs is not None:
        dev["arb_Z"] = frel(k, [name + "_arb_Z" + x for x in sfx])
    k, delta, it0 = rc.apply_Z(eta, t["fit"])
    dev["fit_delta"], counts["fit_iters"] = srel(delta, t["fit"]["delta"]), it0
    if arrs is not None:
        dev["fit_Z"] = frel(k, [name + "_fit_Z" + x for x in sfx])
    e0, pf, napp, deltas, iters = rc.heatbath(eta, t["fit"])
    hb = t["fit"]["heatbath"]
    counts["heatbath_napp"], counts["heatbath_iters"] = napp, iters
    dev["energy0"] = srel(e0, hb["energy0"])
    dev["heatbath_deltas"] = [srel(a, b) for a, b in zip(deltas, hb["deltas"])]
    dev["pf_norm"] = srel(_sq(pf), sum(hb["pf_norms"]))
    if arrs is not None:
        dev["pf"] = frel(pf, [name + "_pf" + x for x in sfx])
        pf = tuple(cplx(arrs[name + "_pf" + x]) for x in sfx)             # the acceptance step starts from the reference's field
    e1, napp, deltas, iters, w = rc.acc(pf, t["fit"])
    ac = t["fit"]["acc"]
    counts["acc_napp"], counts["acc_iters"] = napp, iters
    dev["energy1"] = srel(e1, ac["energy1"])
    dev["acc_deltas"] = [srel(a, b) for a, b in zip(deltas, ac["deltas"])]
    if arrs is not None:
        dev["w"] = frel(w, [name + "_w4", name + "_w5"][:len(sfx)])
    return dev, counts
