"""Child process of tests/test_gpu_trajectory_dropin.py.

A host program in miniature, as tests/flow_dropin_child.py: the stub globals of tests/host_stub/globals.c are loaded first, then
libtmlqcd_dropin.so.  In the residency mode given on the command line it runs two trajectories of update_tm.c on a 4^4 lattice --
gauge monomial (tmlqcd_hip_gauge_derivative) and determinant monomial (cg_her, Qtm_minus_psi, H_eo_tm_inv_psi, deriv_Sb), leapfrog --
with the six calls of the trajectory frame in the reference's order:

  tmlqcd_hip_gauge_snapshot, [momenta drawn on the host], integrate (tmlqcd_hip_force_norms once on the way),
  tmlqcd_hip_moment_energy, tmlqcd_hip_gauge_snapshot_diff, then tmlqcd_hip_reject_links (first trajectory, after the host has raised
  g_update_gauge_copy on its own) or tmlqcd_hip_accept_links (second trajectory)

and prints what it saw as one JSON line: host links, flags, the library's transfer counters around every step, the values with what
the host's own loops give for them."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests import traj_restate as tj  # noqa: E402
from tests.hostprog import HF  # noqa: E402
from tests.util import random_spinor  # noqa: E402

VP, dbl = C.c_void_p, C.c_double
DIMS = (4, 4, 4, 4)
KAPPA, MU, BETA = 0.125, 0.25, 5.6
NSTEPS, EPS = 2, 0.05
EO, OE = 0, 1


def main(mode):
    resident = mode == "resident"
    V = int(np.prod(DIMS))
    N = V // 2
    stub, _, d = hostprog.load()
    g = tj.gauge(DIMS)
    gptr = hostprog.init_lattice(stub, *DIMS, g, KAPPA)
    stub.stub_set_mu(MU)
    grows = (VP * V)(*[gptr + 4 * 144 * i for i in range(V)])
    host_links = np.frombuffer((dbl * (V * 72)).from_address(gptr), dtype=np.float64).reshape(V, 4, 3, 3, 2)
    mom, df = np.zeros((V, 4, 8)), np.zeros((V, 4, 8))
    mrows = (VP * V)(*[mom.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
    drows = (VP * V)(*[df.ctypes.data + 4 * 8 * 8 * i for i in range(V)])
    hf = HF(C.cast(grows, VP), C.cast(mrows, VP), C.cast(drows, VP), 0, 0)
    hp = lambda a: a.ctypes.data_as(VP)
    R = random_spinor(41, N)
    phi, X, Y, w2, w3, hop = (np.zeros((N, 4, 3, 2)) for _ in range(6))

    def counts():
        c = (C.c_ulong * 4)()
        d.tmlqcd_hip_transfer_counts(c)
        return [int(v) for v in c]

    def delta(a, b):
        return [y - x for x, y in zip(a, b)]

    out = {"mode": mode}
    d.tmlqcd_hip_set_residency(1 if resident else 0)
    d.Qtm_plus_psi(hp(phi), hp(R))                                       # det_heatbath: phi = Q_+ R
    norms = {}

    def force(step, probe=False):
        df[:] = 0.0
        d.tmlqcd_hip_gauge_derivative(C.byref(hf), BETA, 1.0, 0.0, 0, 0.0)
        it = d.cg_her(hp(X), hp(phi), 2000, 1e-26, 1, N, C.cast(d.Qtm_pm_psi, VP))   # (the last solution is the starting guess)
        assert it > 0, it
        d.Qtm_minus_psi(hp(Y), hp(X))
        d.H_eo_tm_inv_psi(hp(w2), hp(X), EO, -1.0)
        d.deriv_Sb(OE, hp(Y), hp(w2), C.byref(hf), 1.0)
        d.H_eo_tm_inv_psi(hp(w3), hp(Y), EO, +1.0)
        before_last = df.copy()
        d.deriv_Sb(EO, hp(w3), hp(X), C.byref(hf), 1.0)
        if probe:
            s, m = dbl(), dbl()
            d.tmlqcd_hip_force_norms(C.byref(hf), C.byref(s), C.byref(m))
            if resident:                                                # the whole force is on the device, nothing of it on the host yet
                assert not df.any()
                d.tmlqcd_hip_flush_derivative(C.byref(hf))
                want = df
            else:                                                       # every contribution was flushed; the accumulator holds the last one
                want = df - before_last
            _, exact, mx = tj.derivative_norms(want)
            norms.update(sum=s.value, max=m.value, want_sum=exact, want_max=mx)
        if resident:
            d.tmlqcd_hip_update_momenta(step, C.byref(hf))
        else:
            mom[:] -= step * df                                         # update_momenta.c:67-72 on the host

    def trajectory(seed, probe):
        d.tmlqcd_hip_gauge_snapshot(C.byref(hf))
        c0 = counts()
        mom[:] = tj.momenta(DIMS, seed)                                  # random_su3adj_field
        enep = tj.moment_energy(mom)[1]
        force(0.5 * EPS, probe)
        for k in range(NSTEPS):
            d.tmlqcd_hip_update_gauge(EPS, C.byref(hf))
            force(EPS if k < NSTEPS - 1 else 0.5 * EPS)
        enepx = d.tmlqcd_hip_moment_energy(C.byref(hf))
        ddu = d.tmlqcd_hip_gauge_snapshot_diff(C.byref(hf))
        return c0, counts(), enep, enepx, ddu

    # ---- first trajectory: rejected, after the host has raised the flag on its own
    c0, c1, enep, enepx, ddu = trajectory(51, True)
    r = {"window": delta(c0, c1), "enepx": enepx, "ddu": ddu, "host_links_are_g_before": bool(np.array_equal(host_links, g))}
    if not resident:
        r["enepx_host"] = tj.moment_energy(mom)[1]                       # hf->momenta is the truth in coherent mode
        r["ddu_host"] = tj.snapshot_diff(np.array(host_links), g)[1]
    stub.stub_mark_gauge_dirty()
    host_links[0, 0, 0, 0, 0] += 0.5                                     # ... and scribbled on its links: the snapshot wins
    d.tmlqcd_hip_reject_links(C.byref(hf))
    c2 = counts()
    r["reject"] = delta(c1, c2)
    r["flags_down"] = stub.stub_gauge_flag() == 0 and hf.update_gauge_copy == 0
    r["ddu_after"] = d.tmlqcd_hip_gauge_snapshot_diff(C.byref(hf))
    if resident:
        host_links[0, 0, 0, 0, 0] = g[0, 0, 0, 0, 0]                     # (undo the scribble: the host's array stays the host's)
    r["host_links_are_g_after"] = bool(np.array_equal(host_links, g))
    c3 = counts()
    d.Hopping_Matrix(0, hp(hop), hp(R))
    r["stencil_after"] = delta(c3, counts())
    out["reject"] = r

    # ---- second trajectory: accepted
    c0, c1, enep, enepx, ddu = trajectory(52, False)
    a = {"window": delta(c0, c1), "enepx": enepx, "ddu": ddu}
    if resident:
        d.tmlqcd_hip_sync_momenta_to_host(C.byref(hf))                   # (for the comparison only; after the window)
    a["enepx_host"] = tj.moment_energy(mom)[1]
    c1 = counts()
    before = np.array(host_links)
    d.tmlqcd_hip_accept_links(C.byref(hf), 1)
    c2 = counts()
    a["accept"] = delta(c1, c2)
    a["flags_down"] = stub.stub_gauge_flag() == 0 and hf.update_gauge_copy == 0
    a["host_links_untouched_by_accept"] = bool(np.array_equal(host_links, before))
    a["host_links_are_g"] = bool(np.array_equal(host_links, g))
    c3 = counts()
    d.Hopping_Matrix(0, hp(hop), hp(R))
    a["stencil_after"] = delta(c3, counts())
    d.tmlqcd_hip_sync_gauge_to_host(C.byref(hf))                         # resident: the final sync; coherent: nothing left to do
    a["sync"] = delta(c3, counts())
    final = np.array(host_links)
    a["final_row_deviation"] = tj.row_norm_deviation(final)
    a["final_moved"] = float(np.abs(final - g).max())
    if not resident:
        a["accept_err"] = float(np.abs(final - tj.restoresu3(before)).max())
    out["accept"] = a
    out["norms"] = norms
    d.tmlqcd_hip_finalize()
    hostprog.emit(out)


if __name__ == "__main__":
    main(sys.argv[1])
