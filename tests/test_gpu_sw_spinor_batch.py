"""GPU: sw_spinor_eo_batch (clover.hip) -- n outer-product pairs of operator/clover_deriv.c:252-318 summed into swm / swp in one
launch -- against the CPU oracle's sw_spinor_eo applied n times and against n launches of the device's own single-pair kernel,
on 4^4 and a ragged shape with a padded field stride (tests/ndsw_restate.FORCE_SHAPES) plus 2^4; the refusals."""
import types

import numpy as np
import pytest

from tests import ndsw_restate as sw
from tests.util import TOL, random_spinor, rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 2, 2)] + sw.FORCE_SHAPES
IDS = ["2x2x2x2", "4x4x4x4", "6x4x2x8"]
RAT_MAX_PAIRS = 64


def pair(shape):
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    return Oracle(*shape, kappa=sw.KAPPA, mu=0.0), Lattice(*shape, kappa=sw.KAPPA, mu=0.0)


def parity_sites(orc):
    """lexicographic site numbers of the even and of the odd sites"""
    lex = np.asarray(orc.eo2lexic())
    return [lex[:orc.Vh], lex[orc.VPR // 2:orc.VPR // 2 + orc.Vh]]


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_batch_against_the_oracle_and_against_single_calls(shape, n):
    orc, lat = pair(shape)
    N = orc.Vh
    m = min(n, 4) + 1
    host = [random_spinor(700 + q, N) for q in range(m)]
    dev = [lat.field(h) for h in host]
    obuf = []
    for h in host:
        b = orc.new_field(); b[:N] = h; obuf.append(b)
    ki = [j % m for j in range(n)]                    # pool[q] is kk of pair q and ll of pair q-1: one field in two pairs from n = 2 on
    li = [(j + 1) % m for j in range(n)]
    fac = [(-1.0) ** (j + 1) * (0.3 + 0.11 * (j % 5)) for j in range(n)]         # the first factor is negative
    sites = parity_sites(orc)
    for ieo in (0, 1):
        swm, swp = np.zeros((orc.V, 4, 3, 3, 2)), np.zeros((orc.V, 4, 3, 3, 2))
        lat.swpm_zero()
        orc.sw_spinor_eo(1 - ieo, swm, swp, obuf[0], obuf[1], 0.37)              # something is there already, on the other parity ...
        lat.sw_spinor_eo(1 - ieo, dev[0], dev[1], 0.37)
        orc.sw_spinor_eo(ieo, swm, swp, obuf[1], obuf[0], -0.21)                 # ... and on this one
        lat.sw_spinor_eo(ieo, dev[1], dev[0], -0.21)
        bm, bp = lat.get_swpm()
        for j in range(n):
            orc.sw_spinor_eo(ieo, swm, swp, obuf[ki[j]], obuf[li[j]], fac[j])
        lat.sw_spinor_eo_batch(ieo, [dev[q] for q in ki], [dev[q] for q in li], fac)
        gm, gp = lat.get_swpm()
        e1 = max(rel_err(gm, swm), rel_err(gp, swp))
        # the other parity's half is untouched bit for bit
        assert np.array_equal(gm[sites[1 - ieo]], bm[sites[1 - ieo]]) and np.array_equal(gp[sites[1 - ieo]], bp[sites[1 - ieo]])
        # n launches of the single-pair kernel
        lat.swpm_zero()
        lat.sw_spinor_eo(1 - ieo, dev[0], dev[1], 0.37)
        lat.sw_spinor_eo(ieo, dev[1], dev[0], -0.21)
        for j in range(n):
            lat.sw_spinor_eo(ieo, dev[ki[j]], dev[li[j]], fac[j])
        sm, sp = lat.get_swpm()
        e2 = max(rel_err(gm, sm), rel_err(gp, sp))
        print("sw_spinor_eo_batch %s ieo = %d n = %d: against the oracle %.2e, against n single launches %.2e" % (shape, ieo, n, e1, e2))
        assert e1 < TOL
        assert e2 < TOL
        # it accumulates: from zero, a second call doubles the result
        lat.swpm_zero()
        lat.sw_spinor_eo_batch(ieo, [dev[q] for q in ki], [dev[q] for q in li], fac)
        om, op = lat.get_swpm()
        lat.sw_spinor_eo_batch(ieo, [dev[q] for q in ki], [dev[q] for q in li], fac)
        tm, tp = lat.get_swpm()
        assert np.array_equal(tm, 2 * om) and np.array_equal(tp, 2 * op)
        assert om.any() and not om[sites[1 - ieo]].any() and not op[sites[1 - ieo]].any()
    for h, d in zip(host, dev):
        assert np.array_equal(d.download(), h)
    lat.close()


def test_refusals_leave_the_accumulators_alone():
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    orc, lat = pair((4, 4, 4, 4))
    N = lat.Vh
    a, b = lat.field(random_spinor(1, N)), lat.field(random_spinor(2, N))
    lat.swpm_zero()
    lat.sw_spinor_eo(0, a, b, 0.3)
    before = lat.get_swpm()
    other = Lattice(4, 4, 4, 6)                                         # another stride
    big = RAT_MAX_PAIRS + 1
    cases = {
        "n = 0": ([], [], []),
        "n > RAT_MAX_PAIRS": ([a] * big, [b] * big, [1.0] * big),
        "null kk": ([a, types.SimpleNamespace(h=None)], [b, b], [1.0, 1.0]),
        "null ll": ([a], [types.SimpleNamespace(h=None)], [1.0]),
        "fp32": ([a], [lat.field32()], [1.0]),
        "full field": ([lat.full_field()], [b], [1.0]),
        "stride": ([a, a], [b, other.field()], [1.0, 1.0]),
    }
    for what, (ks, ls, fs) in cases.items():
        with pytest.raises(TmHipError):
            lat.sw_spinor_eo_batch(0, ks, ls, fs)
        gm, gp = lat.get_swpm()
        assert np.array_equal(gm, before[0]) and np.array_equal(gp, before[1]), what
    lat.sw_spinor_eo_batch(0, [a] * RAT_MAX_PAIRS, [b] * RAT_MAX_PAIRS, [0.0] * RAT_MAX_PAIRS)   # the largest legal n, factors 0: adds nothing
    gm, gp = lat.get_swpm()
    assert np.array_equal(gm, before[0]) and np.array_equal(gp, before[1])
    other.close()
    lat.close()
