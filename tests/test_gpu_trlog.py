"""GPU: the tr-log energies sw_trace / sw_trace_nd (operator/clover_det.c:115-279; clover.hip) on the device's clover term against
tests/cloverrat_restate.py (numpy.linalg.slogdet / det on the CPU oracle's sw), the clover determinant trajectory of
tests/test_gpu_md_trajectory.py with its tr-log taken on the device, and the drop-in symbols on host arrays, unsplit and on two
T-split ranks.

Bound: |got - want| <= TOL * sum over the sites of |per-site term| -- the project's fp64 tolerance on the natural scale of the sum."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cloverrat_restate as cr
from tests import ndsw_restate as sw
from tests.hostprog import run_child
from tests.test_gpu_md_trajectory import CloverDetTrajectory
from tests.util import TOL, random_gauge

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAPPA, C_SW = sw.KAPPA, sw.C_SW
IDS = ["2x2x2x2", "4x4x4x4", "6x4x2x8"]


def pair(shape):
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    orc = Oracle(*shape, kappa=KAPPA, mu=0.0, theta=sw.THETA)
    lat = Lattice(*shape, kappa=KAPPA, mu=0.0, theta=sw.THETA)
    g = random_gauge(sw.shape_seed(shape), orc.VPR)
    orc.set_gauge(g)
    lat.set_gauge(g)
    lat.sw_term(g, KAPPA, C_SW)
    return orc, lat, cr.clover_of(orc, KAPPA, C_SW), g


@pytest.mark.parametrize("shape", cr.TRACE_SHAPES, ids=IDS)
def test_traces_against_the_restatement(shape):
    orc, lat, cl, g = pair(shape)
    for ieo in (0, 1):
        for mu in cr.TRACE_MU:
            want, scale = cr.sw_trace(cl, ieo, mu)
            got = lat.sw_trace(ieo, mu)
            assert lat.sw_trace_failures() == 0
            print("sw_trace %s ieo = %d mu = %g: %.15e (cpu %.15e), distance / scale %.2e" % (shape, ieo, mu, got, want, abs(got - want) / scale))
            assert abs(got - want) <= TOL * scale
            assert lat.sw_trace(ieo, mu) == got                         # the same bits on every run
            nd0 = lat.sw_trace_nd(ieo, mu, 0.0)                         # eps = 0: the same number (clover_det.c:199-200)
            assert abs(nd0 - got) <= TOL * scale
        for name, (mub, epsb, _) in sw.POINTS.items():
            want, scale = cr.sw_trace_nd(cl, ieo, mub, epsb)
            got = lat.sw_trace_nd(ieo, mub, epsb)
            assert lat.sw_trace_failures() == 0
            print("sw_trace_nd %s ieo = %d %s: %.15e (cpu %.15e), distance / scale %.2e" % (shape, ieo, name, got, want, abs(got - want) / scale))
            assert abs(got - want) <= TOL * scale
            assert lat.sw_trace_nd(ieo, mub, epsb) == got
    lat.close()


def test_refused_until_the_clover_term_is_that_of_the_current_links():
    from tmlqcd_amd import Lattice
    from tmlqcd_amd.hip import TmHipError
    shape = (4, 4, 4, 4)
    orc, lat, cl, g = pair(shape)
    before = lat.sw_trace(0, 0.1)
    lat.momenta_upload(np.random.default_rng(3).standard_normal((lat.V, 4, 8)))
    lat.update_gauge(0.05)
    with pytest.raises(TmHipError):
        lat.sw_trace(0, 0.1)
    with pytest.raises(TmHipError):
        lat.sw_trace_nd(0, 0.1, 0.05)
    lat.sw_term(None, KAPPA, C_SW)
    moved = lat.sw_trace(0, 0.1)
    orc.set_gauge(np.ascontiguousarray(lat.gauge_download()))
    want, scale = cr.sw_trace(cr.clover_of(orc, KAPPA, C_SW), 0, 0.1)
    assert abs(moved - want) <= TOL * scale and abs(moved - before) > 1e3 * TOL * scale
    lat.close()
    fresh = Lattice(*shape, kappa=KAPPA)                                # no clover term at all
    with pytest.raises(TmHipError):
        fresh.sw_trace(0, 0.0)
    fresh.close()


class DeviceTrlogTrajectory(CloverDetTrajectory):
    """tests/test_gpu_md_trajectory.CloverDetTrajectory with the tr-log of its Hamiltonian taken on the device: no copy of the clover term"""

    def trlog(self):
        return -self.lat.sw_trace(0, self.mu)

    def host_trlog(self):
        return CloverDetTrajectory.trlog(self)


def test_clover_determinant_trajectory_with_the_trlog_on_the_device():
    tr = DeviceTrlogTrajectory()
    tr.clover()
    dev, host = tr.trlog(), tr.host_trlog()
    assert tr.lat.sw_trace_failures() == 0
    scale = _host_scale(tr.lat, tr.mu)
    print("tr-log at 8^4: device %.15e, numpy %.15e, distance / scale %.2e" % (dev, host, abs(dev - host) / scale))
    assert abs(dev - host) <= TOL * scale
    h0 = tr.energy()
    dh = {}
    for nsteps in (4, 8):
        tr.reset()
        tr.leapfrog(nsteps, 0.2 / nsteps)
        dh[nsteps] = tr.energy() - h0
    p = tr.lat.momenta_download()
    tr.lat.momenta_upload(-p)
    tr.leapfrog(8, 0.2 / 8)
    back = tr.lat.gauge_download()[:tr.lat.V]
    tr.close()
    print("clover, tr-log on the device: H0 = %.6f   dH(eps = 0.05) = %.3e   dH(eps = 0.025) = %.3e   ratio %.2f" % (h0, dh[4], dh[8], dh[4] / dh[8]))
    assert abs(dh[4]) < 5e-4 * abs(h0) and abs(dh[8]) < abs(dh[4])          # the assertions of test_clover_determinant_trajectory_conserves_its_hamiltonian
    assert 3.0 < dh[4] / dh[8] < 5.5
    assert np.abs(back - tr.g0).max() < 1e-10


def _host_scale(lat, mu):
    """sum over the even sites of |per-site term| of sw_trace(EE, mu), from the device's clover term in the host layout"""
    from oracle.oraclebind import Oracle
    orc = Oracle(lat.T, lat.LX, lat.LY, lat.LZ)
    cl = cr.Clover(lat.get_clover(True, False)[0], np.array(orc.eo2lexic()), orc.Vh, orc.VPR // 2)
    return float(np.abs(cr.sw_trace_terms(cl, 0, mu).sum(axis=1)).sum())


# ---------------------------------------------------------------- drop-in
def test_dropin_symbols():
    errs = run_child("trlog_dropin_child.py")
    print(errs)
    assert {"device_sw_trace_0_0", "device_sw_trace_1_0.23", "device_sw_trace_nd_0", "upload_sw_trace", "device_failures"} <= set(errs)
    for k, v in errs.items():
        if k == "upload_differs":
            assert v > 1e3 * TOL, (k, v)                                # the uploaded term is told apart from the device's
        elif k.endswith("_failures"):
            assert v == 0.0, (k, v)
        else:
            assert v <= TOL, (k, v)


def test_drop_in_traces_are_global_on_t_split_ranks(tmp_path):
    """Two T-split ranks over the host-staged transport (tests/mp_trlog_worker.py): both return the same bits, the sum over the whole
    lattice -- the unsplit value to the bound."""
    from oracle.oraclebind import Oracle
    from tmlqcd_amd import Lattice
    from tmlqcd_amd import synthetic as syn
    world = 2
    worker = os.path.join(ROOT, "tests", "mp_trlog_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TMLQCD_HIP_FLAG_TIMEOUT_S="60")
    job = "tl_%d_%d" % (os.getpid(), world)
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), job, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=400) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    parts = [np.load(os.path.join(str(tmp_path), "trlog_%d_of_%d.npz" % (r, world))) for r in range(world)]
    shape, seed, kappa, c_sw, mu, (mub, epsb) = cr.SPLIT_CASE
    g = syn.gauge_field(seed, *shape)
    orc = Oracle(*shape, kappa=kappa, mu=0.0)
    orc.set_gauge(g)
    cl = cr.clover_of(orc, kappa, c_sw)
    lat = Lattice(*shape, kappa=kappa)
    lat.set_gauge(g)
    lat.sw_term(g, kappa, c_sw)
    want = [cr.sw_trace(cl, 0, 0.0), cr.sw_trace(cl, 0, mu), cr.sw_trace(cl, 1, mu), cr.sw_trace_nd(cl, 0, mub, epsb), cr.sw_trace_nd(cl, 1, mub, epsb)]
    unsplit = [lat.sw_trace(0, 0.0), lat.sw_trace(0, mu), lat.sw_trace(1, mu), lat.sw_trace_nd(0, mub, epsb), lat.sw_trace_nd(1, mub, epsb)]
    lat.close()
    assert np.array_equal(parts[0]["sums"], parts[1]["sums"])           # the same bits on both ranks
    assert parts[0]["fails"][0] == 0 and parts[1]["fails"][0] == 0
    for got, (w, scale), u in zip(parts[0]["sums"], want, unsplit):
        print("split %.15e   unsplit %.15e   cpu %.15e   scale %.3e" % (got, u, w, scale))
        assert abs(got - w) <= TOL * scale and abs(got - u) <= TOL * scale
        assert abs(w) / 4 > 1e3 * TOL * scale                           # one rank's share, about half the sum, would not pass
