"""GPU: the six drop-in calls of the trajectory frame (include/tmlqcd_dropin.h) in a host program in miniature
(tests/traj_dropin_child.py: tests/host_stub + libtmlqcd_dropin.so in a process of its own), coherent and resident.

Two trajectories of update_tm.c -- gauge monomial and determinant monomial, the first rejected after the host has raised
g_update_gauge_copy and scribbled on its links, the second accepted -- with what the host sees around the six calls:

* both modes: tmlqcd_hip_moment_energy == the host's own loop on hf->momenta, ret_gauge_diff is exactly 0 after the reject (the snapshot
  wins), flags down after accept / reject, a following Hopping_Matrix uploads nothing;
* coherent: hf->gaugefield holds the device's links after accept / reject (one download each), ret_gauge_diff == the host's loop on them;
* resident: between tmlqcd_hip_gauge_snapshot and the acceptance step nothing crosses the bus but the momenta random_su3adj_field has
  drawn on the host (one upload per trajectory); accept and reject themselves move nothing and leave g_gauge_field alone until
  tmlqcd_hip_sync_gauge_to_host.
The transfer counts are the library's own (tmlqcd_hip_transfer_counts: gauge up, gauge down, momenta up, momenta down)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import traj_restate as tj
from tests.hostprog import last_json, run_child
from tests.traj_restate import U53 as U, chain_diff, chain_energy, chain_norms

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (4, 4, 4, 4)


def within(got, want, n):
    return abs(got - want) <= n * U * abs(want)


@pytest.fixture(scope="module")
def runs():
    out = {}
    for mode in ("coherent", "resident"):
        r = run_child("traj_dropin_child.py", mode, cwd=None, check=False)
        assert r.returncode == 0, (mode, r.stderr[-3000:])
        out[mode] = last_json(r)
        print(mode, out[mode])
    return out


@pytest.mark.parametrize("mode", ["coherent", "resident"])
def test_the_six_calls(mode, runs):
    o = runs[mode]
    rej, acc, nrm = o["reject"], o["accept"], o["norms"]
    ne, nd, nn = chain_energy(SHAPE), chain_diff(SHAPE), chain_norms(SHAPE)
    # the reject: the host's raise and its scribble do not reach the device, the links are the snapshot's again
    assert rej["host_links_are_g_before"] == (mode == "resident")         # coherent: update_gauge kept the host's links current
    assert rej["ddu"] > 1e-3 and rej["ddu_after"] == 0.0
    assert rej["flags_down"] and rej["host_links_are_g_after"]
    assert rej["stencil_after"] == [0, 0, 0, 0]
    # the accept
    assert acc["flags_down"] and acc["stencil_after"] == [0, 0, 0, 0]
    assert acc["final_row_deviation"] < 1e-13 and acc["final_moved"] > 1e-3
    assert within(acc["enepx"], acc["enepx_host"], ne)
    if mode == "coherent":
        assert within(rej["enepx"], rej["enepx_host"], ne) and within(rej["ddu"], rej["ddu_host"], nd)
        assert rej["reject"] == [0, 1, 0, 0] and acc["accept"] == [0, 1, 0, 0]      # the one download that brings hf->gaugefield up to date
        assert not acc["host_links_untouched_by_accept"] and acc["accept_err"] < 1e-13
        assert acc["sync"] == [0, 0, 0, 0]
        # the accumulator holds the last contribution of a force flushed piece by piece: compared with a difference of host arrays
        assert abs(nrm["sum"] - nrm["want_sum"]) <= 1e-10 * nrm["want_sum"] and abs(nrm["max"] - nrm["want_max"]) <= 1e-10 * nrm["want_max"]
    else:
        # snapshot -> end of the trajectory: the drawn momenta go up once, nothing else moves; accept and reject move nothing
        assert rej["window"] == [0, 0, 1, 0] and acc["window"] == [0, 0, 1, 0]
        assert rej["reject"] == [0, 0, 0, 0] and acc["accept"] == [0, 0, 0, 0]
        assert acc["host_links_untouched_by_accept"] and acc["host_links_are_g"]
        assert acc["sync"] == [0, 1, 0, 0]
        assert within(nrm["sum"], nrm["want_sum"], nn) and abs(nrm["max"] - nrm["want_max"]) <= 8 * U * nrm["want_max"]


def test_the_modes_agree(runs):
    """the same two trajectories: the modes differ in where update_momenta runs (host loop / device kernel), i.e. in rounding"""
    c, r = runs["coherent"], runs["resident"]
    for part in ("reject", "accept"):
        for key in ("enepx", "ddu"):
            assert abs(c[part][key] - r[part][key]) <= 1e-9 * abs(c[part][key]), (part, key)


@pytest.mark.parametrize("world", [2, 4])
def test_t_split_ranks(world, tmp_path):
    """Ranks are host processes with tmLQCD's own globals (tests/mp_traj_worker.py, shared-memory transport), coherent mode.  The three
    values are the sums (the maximum) over the WHOLE lattice with the same bits on every rank, as after the reference's MPI_Allreduce /
    MPI_Reduce; after tmlqcd_hip_accept_links every rank's halo slabs are its neighbours' slices bit for bit although nothing was
    exchanged, and tmlqcd_hip_reject_links brings back links and slabs of the second snapshot."""
    worker = os.path.join(ROOT, "tests", "mp_traj_worker.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", TMLQCD_HIP_FLAG_TIMEOUT_S="60")
    job = "tj_%d_%d" % (os.getpid(), world)
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), job, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=400) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    parts = [np.load(os.path.join(str(tmp_path), "traj_%d_of_%d.npz" % (r, world))) for r in range(world)]
    dims = (8, 4, 4, 4)
    local = (8 // world, 4, 4, 4)
    XYZ = 64
    V = local[0] * XYZ
    own = lambda key: np.ascontiguousarray(np.concatenate([p[key][:V] for p in parts]))
    noisy, mom = tj.noisy_gauge(dims), tj.momenta(dims)
    energy, ddu, fsum, fmax = parts[0]["sums"]
    for r in range(world):
        assert np.array_equal(parts[r]["sums"], parts[0]["sums"]), r                      # the same bits on every rank
    extra = world - 1                                                                      # the additions over the ranks
    assert abs(energy - tj.moment_energy(mom)[1]) <= (chain_energy(local) + extra) * U * energy
    assert abs(ddu - tj.snapshot_diff(own("moved"), noisy)[1]) <= (chain_diff(local) + extra) * U * ddu
    _, want_sum, want_max = tj.derivative_norms(own("force"))
    assert abs(fsum - want_sum) <= (chain_norms(local) + extra) * U * want_sum and abs(fmax - want_max) <= 8 * U * want_max
    share = tj.derivative_norms(parts[0]["force"])
    assert share[1] < 0.9 * fsum                                                           # a rank-local sum would not pass
    want = tj.restoresu3(own("moved"))
    for r in range(world):
        up, dn = parts[(r + 1) % world], parts[(r - 1) % world]
        acc = parts[r]["accepted"]
        assert np.abs(acc[:V] - want[r * V:(r + 1) * V]).max() < 1e-13 and tj.row_norm_deviation(acc) < 1e-13
        assert np.array_equal(acc[V:V + XYZ], up["accepted"][:XYZ]) and np.array_equal(acc[V + XYZ:], dn["accepted"][V - XYZ:V]), r
        assert not np.array_equal(parts[r]["moved_again"], acc)
        assert np.array_equal(parts[r]["rejected"], acc) and parts[r]["ddu_after_reject"][0] == 0.0
