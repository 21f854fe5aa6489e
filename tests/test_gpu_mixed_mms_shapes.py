"""GPU: tmhip_mixed_cg_mms_tm_nd on the shapes and launch forms where its kernels can go wrong, its refusals, and the monomial option.

* shapes: (2,2,2,2) where the +mu and -mu neighbours coincide, (4,2,6,2) with LZ/2 = 1, the ragged (6,10,2,4) and (10,10,6,14), whose
  4200 sites per parity take the padded XCD grid of the stencil and end in a partial wave (the set-up of tests/test_gpu_nd32_shapes.py:
  kappa 0.13, theta = (1, 0.3, -0.2, 0.5)); both forms of the operator ("nd_fused") and both forms of the vector pass ("mms32_fused").
  Yardstick: the restatement of tests/mixed_mms_restate.py on the CPU oracle's operator rounded to float32 (held against the
  reference's own runs by tests/test_mixed_mms_restate.py): the count rule on the iterations, update and removal counts equal or, where
  the counts moved within that rule, within one, and per shift the distance to oracle/nd_restate.py's cg_mms_tm_nd at most FACTOR
  times the restatement's.
* refusals, each with sentinel-filled outputs left untouched: the clover operator, a loopback context, 33 shifts, fp32 fields as P.
* "nd_mms_mixed": 1 moves tmhip_ndrat_derivative by no more than FACTOR times what the restatement's mixed solutions move the
  restated force; 0 is byte-identical to the option never set.
"""
import numpy as np
import pytest

from oracle import nd_restate as nd
from tests import mixed_mms_restate as mr
from tests.util import random_gauge, random_spinor

pytestmark = pytest.mark.gpu

KAPPA = 0.13
THETA = (1.0, 0.3, -0.2, 0.5)
FIXTURE = (0.1375, 0.1175, 0.6931)                 # (mubar, epsbar, invmaxev) of tests/golden/ref_nd_*
SHIFTS = [0.02, 0.15, 0.6, 2.5, 9.0]               # of tests/golden/ref_nd_scalars_8x8.json
SHAPES = [(2, 2, 2, 2), (4, 2, 6, 2), (6, 10, 2, 4), (10, 10, 6, 14)]
MAX_ITER, EPS_SQ, REL_PREC = 2000, 1e-14, 1         # tight enough for the reliable updates (rel_delta = 1e-10) and the removals
FACTOR = 4.0                                        # tests/test_gpu_mixed_mms.py


class _Setup:
    def __init__(self, shape):
        from oracle.oraclebind import Oracle
        from tmlqcd_amd import Lattice
        self.shape = shape
        self.orc = Oracle(*shape, kappa=KAPPA, mu=0.0, theta=THETA, threads=8)
        self.lat = Lattice(*shape, kappa=KAPPA, mu=0.0, theta=THETA)
        seed = 3000 + sum(shape) * 7 + shape[0]
        g = random_gauge(seed, self.orc.VPR)
        self.orc.set_gauge(g)
        self.lat.set_gauge(g)
        self.lat.set_nd(*FIXTURE)
        self.N = self.orc.Vh
        self.q = [random_spinor(seed + i, self.N) for i in (5, 6)]
        f64, f32 = mr.operators(self.orc, *FIXTURE)
        qu, qd = nd.cplx(self.q[0]), nd.cplx(self.q[1])
        # computed once, shared by every case of the shape
        self.ret, P, self.info = mr.mixed_cg_mms_tm_nd(f64, f32, qu, qd, SHIFTS, MAX_ITER, EPS_SQ, REL_PREC)
        _, self.X, _, _ = nd.cg_mms_tm_nd(f64, qu, qd, SHIFTS, MAX_ITER, 1e-22, 0)
        self.dist = [mr.distance(P[k], self.X[k]) for k in range(len(SHIFTS))]


@pytest.fixture(scope="module")
def setup():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = _Setup(shape)
        return made[shape]
    yield get
    for st in made.values():
        st.lat.close()


def test_last_shape_takes_the_padded_grid_and_a_partial_wave():
    Vh = 10 * 10 * 6 * 14 // 2
    nb = (Vh + 63) // 64
    assert nb >= 64 and nb % 8 != 0 and Vh % 64 != 0 and Vh % 256 != 0 and Vh > 256      # stencil grid padded; more than one block of the vector pass


@pytest.mark.parametrize("mms_fused", [1, 0])
@pytest.mark.parametrize("nd_fused", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_solver_matches_the_restatement(setup, shape, nd_fused, mms_fused):
    st = setup(shape)
    lat = st.lat
    assert st.ret > 0 and st.info["updates"], (st.ret, st.info)       # the yardstick run has reliable updates on every shape
    lat.set_option("nd_fused", nd_fused)
    lat.set_option("mms32_fused", mms_fused)
    qu, qd = lat.field(st.q[0]), lat.field(st.q[1])
    try:
        it, (nrel, nrem), P = lat.mixed_cg_mms_tm_nd(qu, qd, SHIFTS, MAX_ITER, EPS_SQ, REL_PREC)
        active = lat.nd_active_shifts()
        sol = [(nd.cplx(a.download()), nd.cplx(b.download())) for a, b in P]
    finally:
        lat.set_option("nd_fused", 1)
        lat.set_option("mms32_fused", 1)
        qu.free(); qd.free()
    for a, b in P:
        a.free(); b.free()
    ratios = [mr.distance(sol[k], st.X[k]) / st.dist[k] for k in range(len(SHIFTS))]
    print("%s nd_fused %d mms32_fused %d: %d iterations (restatement %d), %d updates (%d), %d removed (%d), distance ratios %s"
          % (shape, nd_fused, mms_fused, it, st.ret, nrel, len(st.info["updates"]), nrem, len(st.info["removals"]), ["%.2f" % r for r in ratios]))
    assert it > 0 and mr.count_rule(it, st.ret), (it, st.ret)
    slack = 0 if it == st.ret else 1
    assert abs(nrel - len(st.info["updates"])) <= slack, (nrel, st.info["updates"])
    assert abs(nrem - len(st.info["removals"])) <= slack, (nrem, st.info["removals"])
    assert active == len(SHIFTS) - nrem
    assert max(ratios) <= FACTOR, ratios


# ---------------------------------------------------------------- refusals
def _refusal_lattice():
    from tmlqcd_amd import Lattice
    lat = Lattice(4, 4, 4, 4, kappa=KAPPA, mu=0.0)
    lat.set_gauge(random_gauge(5, lat.V))
    lat.set_nd(*FIXTURE)
    return lat


def test_refusals_leave_the_outputs_untouched(capfd):
    from tmlqcd_amd.hip import TmHipError
    lat = _refusal_lattice()
    N = lat.Vh
    s64 = np.full((N, 4, 3, 2), 7.0)
    s32 = np.full((N, 4, 3, 2), 7.0, dtype=np.float32)
    qu, qd = lat.field(random_spinor(2, N)), lat.field(random_spinor(3, N))
    P = [(lat.field(s64), lat.field(s64)) for _ in range(2)]
    P32 = [(lat.field32(s32), lat.field32(s32)) for _ in range(2)]
    args = (100, 1e-14, 1)

    def refused(call, message):
        capfd.readouterr()
        with pytest.raises(TmHipError):
            call()
        assert message in capfd.readouterr().err, message
        for a, b in P:
            assert np.array_equal(a.download(), s64) and np.array_equal(b.download(), s64), message
        for a, b in P32:
            assert np.array_equal(a.download(), s32) and np.array_equal(b.download(), s32), message

    # the clover doublet has no fp32 twin: refused through the fp32 column of the operator table, as rg_mixed_cg_her_nd refuses it
    refused(lambda: lat.mixed_cg_mms_tm_nd(qu, qd, SHIFTS[:2], *args, P=P, op="Qsw_pm_ndpsi"), "mixed_cg_mms_tm_nd does not take Qsw_pm_ndpsi")
    refused(lambda: lat.mixed_cg_mms_tm_nd(qu, qd, [0.1 + 0.01 * k for k in range(33)], *args, P=(P * 17)[:33]), "nshifts = 33 is outside [1, 32]")
    refused(lambda: lat.mixed_cg_mms_tm_nd(qu, qd, SHIFTS[:2], *args, P=P32), "needs fp64 one-parity (EO) solution fields")
    lat.set_loopback(1)
    try:
        refused(lambda: lat.mixed_cg_mms_tm_nd(qu, qd, SHIFTS[:2], *args, P=P), "mixed_cg_mms_tm_nd: the fp32 doublet runs on unsplit lattices only")
    finally:
        lat.set_loopback(0)
    it, counts, _ = lat.mixed_cg_mms_tm_nd(qu, qd, SHIFTS[:2], 2000, 1e-10, 1, P=P)      # and the same context still solves
    assert it > 0
    lat.close()


# ---------------------------------------------------------------- the monomial option
MU3, RMU3 = [0.21, 0.6, 1.7], [0.05, 0.4, 1.3]      # tests/test_gpu_rat.py
SOLVE = (2000, 1e-14, 1)


def test_nd_mms_mixed_routes_the_ndrat_derivative():
    from oracle.oraclebind import Oracle
    from tests import rat_restate
    from tmlqcd_amd import Lattice
    dims = (4, 4, 4, 4)
    orc = Oracle(*dims, kappa=0.125, mu=0.0, theta=THETA, threads=8)
    g = random_gauge(91, orc.VPR)
    orc.set_gauge(g)
    N = orc.Vh
    hu, hd = random_spinor(21, N), random_spinor(22, N)

    def derivative(option):
        lat = Lattice(*dims, kappa=0.125, mu=0.0, theta=THETA)       # a context of its own: "never set" is really never set
        lat.set_gauge(g)
        lat.set_nd(*FIXTURE)
        if option is not None:
            lat.set_option("nd_mms_mixed", option)
        pu, pd = lat.field(hu), lat.field(hd)
        lat.derivative_zero()
        it = lat.ndrat_derivative(pu, pd, MU3, RMU3, FIXTURE[2], *SOLVE)
        out = lat.derivative().copy()
        lat.close()
        return it, out

    it_unset, d_unset = derivative(None)
    it0, d0 = derivative(0)
    it1, d1 = derivative(1)
    assert it0 == it_unset and d0.tobytes() == d_unset.tobytes()      # 0: nothing changes, bit for bit
    # the yardstick: the restated force on the restatement's mixed solutions against the restated force on the fp64 solutions
    f64, f32 = mr.operators(orc, *FIXTURE)
    qu, qd = nd.cplx(hu), nd.cplx(hd)
    ret, P, info = mr.mixed_cg_mms_tm_nd(f64, f32, qu, qd, MU3, *SOLVE)
    it64, X, _, _ = nd.cg_mms_tm_nd(f64, qu, qd, MU3, *SOLVE)
    assert ret > 0 and it64 == it0 and mr.count_rule(it1, ret), (ret, it1, it64, it0)
    rat = rat_restate.Rat(orc, FIXTURE[0], FIXTURE[1])
    fm = rat.ndrat_force(list(P), MU3, RMU3, FIXTURE[2], np.zeros((orc.VPR, 4, 8)))[:orc.V]
    fx = rat.ndrat_force(list(X), MU3, RMU3, FIXTURE[2], np.zeros((orc.VPR, 4, 8)))[:orc.V]
    bound = float(np.sqrt(((fm - fx) ** 2).sum()))
    got = float(np.sqrt(((d1 - d0) ** 2).sum()))
    print("ndrat_derivative: |F(mixed) - F(fp64)| = %.3e on the device, %.3e in the restatement (|F| = %.3e); iterations %d / %d"
          % (got, bound, float(np.sqrt((d0 ** 2).sum())), it1, it0))
    assert bound > 0 and 0 < got <= FACTOR * bound, (got, bound)
