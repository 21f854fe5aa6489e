"""GPU: tmhip_cg_mms_tm against the NumPy restatement (tests/mms_restate.py over the CPU oracle's operators) on non-hypercubic
lattices with twisted boundaries, in every form the solver takes: the fused e/o stencils (incl. a padded XCD grid), the unfused
e/o form (shapes cg_her does not fuse), and the full-lattice Q_pm_psi."""
import numpy as np
import pytest

from oracle.nd_restate import cplx
from oracle.oraclebind import Oracle
from tests import mms_restate
from tests.test_mms_abi import operator
from tests.util import random_gauge, random_spinor
from tmlqcd_amd import Lattice

pytestmark = pytest.mark.gpu
THETA = (1.0, 0.3, -0.2, 0.5)
KAPPA, MU, C_SW = 0.13, 0.05, 1.1
SHIFTS = [0.05, 0.2, 0.9, 3.0, 8.0]
# (T, LX, LY, LZ), form expected for the e/o operators (0 fused, 1 unfused), padded XCD grid
SHAPES = [((22, 8, 8, 6), 0, True), ((8, 4, 6, 4), 0, False), ((4, 6, 4, 8), 0, False), ((6, 10, 2, 4), 1, False), ((10, 4, 4, 6), 1, False)]


@pytest.mark.parametrize("dims,form,padded", SHAPES)
@pytest.mark.parametrize("opname", ["Qtm_pm_psi", "Qsw_pm_psi", "Q_pm_psi"])
def test_shape_against_restatement(dims, form, padded, opname):
    T, LX, LY, LZ = dims
    V = T * LX * LY * LZ
    Vh = V // 2
    if padded:   # the 64-thread launches of this shape take more than 64 blocks and a grid padded to a multiple of eight (one chunk per XCD)
        assert Vh % 64 == 0 and Vh // 64 >= 64 and (Vh // 64) % 8 != 0
    mu = 0.0 if opname == "Q_pm_psi" else MU
    g = random_gauge(7, V)
    orc = Oracle(T, LX, LY, LZ, kappa=KAPPA, mu=mu, theta=THETA)
    orc.set_gauge(g)
    lat = Lattice(T, LX, LY, LZ, kappa=KAPPA, mu=mu, theta=THETA)
    lat.set_gauge(g)
    if opname == "Qsw_pm_psi":
        sw = orc.sw_term(KAPPA, C_SW)
        swi, fails = orc.sw_invert(sw, 0, mu)
        assert fails == 0
        orc.set_clover(sw, swi)
        lat.sw_term(g, KAPPA, C_SW)
        lat.sw_invert(0, mu)
    full = opname == "Q_pm_psi"
    q = random_spinor(11, V if full else Vh)
    shifts = [mu if full else SHIFTS[0]] + SHIFTS[1:]
    it_ref, reached_ref, P_ref, drops, left = mms_restate.cg_mms_tm(operator(orc, opname, mu), cplx(q), shifts, 1000, 1e-22, 0)
    assert it_ref > 20   # the premise: at least one drop check happened
    it, reached, P = lat.cg_mms_tm(lat.full_field(q) if full else lat.field(q), shifts, 1000, 1e-22, 0, op=opname)
    assert lat.mms_form() == (2 if full else form)
    assert abs(it - it_ref) <= 1
    assert lat.mms_active_shifts() == left
    for k in range(len(shifts)):
        ref = np.stack([P_ref[k].real, P_ref[k].imag], axis=-1)
        assert np.sqrt(np.sum((P[k].download() - ref) ** 2) / np.sum(ref ** 2)) < 1e-9, k
    lat.close()
