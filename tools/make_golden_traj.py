"""TEST INFRASTRUCTURE ONLY: fixtures of the trajectory frame (tests/golden/ref_traj_4x4.npz, ref_traj_scalars_4x4.json,
ref_traj_scalars_8x6x4x12.json).

Run once on a CPU machine after build() (which makes oracle/_ref/libtmref.so from the reference tree):

    python tools/make_golden_traj.py --ref /path/to/tmLQCD [--keep-lib]       (or TMLQCD_REF=/path/to/tmLQCD in the environment)

monomial/moment_energy.c -- and expo.c if libtmref.so does not define restoresu3_in_place -- are compiled here, in place from the
reference tree, into a temporary directory (nothing is copied into this repository) and linked with tools/traj_harness.c against
libtmref.so.  moment_energy is the reference's function; the copy loops, the reunitarisation, the ddU sum of update_tm.c and the norm
loop of monitor_forces.c are restated by the harness on the reference's own macros.

Inputs come from tests/traj_restate.py (seeded), so the fixtures hold results only:
  reunitarized        restoresu3_in_place on traj_restate.noisy_gauge (4^4 only: the links)
  moment_energy       of traj_restate.momenta
  gauge_diff          between traj_restate.gauge and the same links after the CPU oracle's update_gauge(momenta, 1e-3); 0.0 on equal fields
  force_sum, _max     of traj_restate.derivative
The generator refuses to write a fixture the NumPy restatement does not reproduce: links to 1e-15, the two Kahan sums to 4 x 2^-53 of
math.fsum, the maximum exactly, the plain serial sum of monitor_forces.c to (links - 1) x 2^-53 (the bound of recursive summation).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DEFS = ["-DALIGN=", "-DALIGN32=", "-DALIGN_BASE=0x00", "-DALIGN_BASE32=0x00", "-DHAVE_CLOCK_GETTIME=1", "-D_GAUGE_COPY=1", "-D_x86_64=1"]
SHAPES = {"4x4": (4, 4, 4, 4), "8x6x4x12": (8, 6, 4, 12)}


def build_lib(ref, tmp):
    refso = os.path.join(ROOT, "oracle", "_ref", "libtmref.so")
    if not os.path.exists(refso):
        sys.exit("oracle/_ref/libtmref.so missing: run build() first")
    have = subprocess.run(["nm", "-D", "--defined-only", refso], stdout=subprocess.PIPE, text=True, check=True).stdout
    have = {l.split()[-1] for l in have.splitlines() if l.strip()}
    srcs = ["monomial/moment_energy.c"] + ([] if "restoresu3_in_place" in have else ["expo.c"])
    objs = []
    for f in srcs + [os.path.join(ROOT, "tools", "traj_harness.c")]:
        o = os.path.join(tmp, os.path.basename(f)[:-2] + ".o")
        src = f if os.path.isabs(f) else os.path.join(ref, f)
        subprocess.check_call(["gcc", "-std=gnu99", "-fcommon", "-fPIC", "-O2", "-I" + ref] + DEFS + ["-c", src, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libtmtraj.so")
    subprocess.check_call(["gcc", "-shared", "-o", so] + objs + ["-L" + os.path.dirname(refso), "-l:libtmref.so",
                          "-Wl,-rpath," + os.path.dirname(refso), "-Wl,-rpath,$ORIGIN", "-Wl,--no-undefined", "-lm"])
    return so


def gen(tag, so):
    import numpy as np
    sys.path.insert(0, ROOT)
    from oracle.oraclebind import Oracle
    from oracle.refbind import RefLattice
    from tests import traj_restate as tj
    dims = SHAPES[tag]
    r = RefLattice(*dims, kappa=0.125, mu=0.0)   # sets VOLUME and the globals of libtmref.so
    V = r.V
    tl = C.CDLL(so)
    vp, pd = C.c_void_p, C.POINTER(C.c_double)
    tl.tmtraj_moment_energy.argtypes = [vp]
    tl.tmtraj_moment_energy.restype = C.c_double
    tl.tmtraj_gauge_diff.argtypes = [vp, vp]
    tl.tmtraj_gauge_diff.restype = C.c_double
    tl.tmtraj_snapshot.argtypes = [vp, vp]
    tl.tmtraj_restore.argtypes = [vp, vp]
    tl.tmtraj_reunitarize.argtypes = [vp]
    tl.tmtraj_force_norms.argtypes = [vp, pd, pd]
    hp = lambda a: a.ctypes.data_as(vp)
    u = tj.U53

    g, noisy, mom, df = tj.gauge(dims), tj.noisy_gauge(dims), tj.momenta(dims), tj.derivative(dims)
    assert g.shape == (V, 4, 3, 3, 2)
    # snapshot, update, reject: the two copy loops
    tmp = np.zeros_like(g)
    tl.tmtraj_snapshot(hp(tmp), hp(g))
    assert np.array_equal(tmp, g)
    moved = g.copy()
    Oracle(*dims, kappa=0.125, mu=0.0).update_gauge(moved, mom, tj.DIFF_STEP)
    diff = tl.tmtraj_gauge_diff(hp(moved), hp(tmp))
    diff_same = tl.tmtraj_gauge_diff(hp(tmp), hp(g))
    back = moved.copy()
    tl.tmtraj_restore(hp(back), hp(tmp))
    assert np.array_equal(back, g) and diff_same == 0.0
    plain, exact = tj.snapshot_diff(moved, g)
    assert abs(diff - exact) <= 4 * u * exact, (diff, exact)
    # accept: restoresu3_in_place
    reun = noisy.copy()
    tl.tmtraj_reunitarize(hp(reun))
    err = float(np.abs(reun - tj.restoresu3(noisy)).max())
    assert err < 1e-15, err
    assert tj.row_norm_deviation(noisy) > 1e-4 and tj.row_norm_deviation(reun) < 1e-14
    again = reun.copy()
    tl.tmtraj_reunitarize(hp(again))
    # energies and norms
    en = tl.tmtraj_moment_energy(hp(mom))
    eplain, eexact = tj.moment_energy(mom)
    assert abs(en - eexact) <= 4 * u * eexact, (en, eexact)
    s, m = C.c_double(), C.c_double()
    tl.tmtraj_force_norms(hp(df), C.byref(s), C.byref(m))
    fplain, fexact, fmax = tj.derivative_norms(df)
    assert m.value == fmax and abs(s.value - fexact) <= (4 * V - 1) * u * fexact, (s.value, fexact, m.value, fmax)
    scal = {"dims": list(dims), "seeds": {"gauge": tj.GAUGE_SEED, "noise": tj.NOISE_SEED, "momenta": tj.MOM_SEED, "derivative": tj.DERIV_SEED},
            "noise": tj.NOISE, "diff_step": tj.DIFF_STEP, "moment_energy": en, "gauge_diff": diff, "gauge_diff_equal_fields": diff_same,
            "force_sum": s.value, "force_max": m.value, "noisy_row_deviation": tj.row_norm_deviation(noisy),
            "reunitarize_twice_max_change": float(np.abs(again - reun).max())}
    json.dump(scal, open(os.path.join(GOLD, "ref_traj_scalars_%s.json" % tag), "w"), indent=1)
    if tag == "4x4":
        np.savez_compressed(os.path.join(GOLD, "ref_traj_%s.npz" % tag), reunitarized=reun)
    print("%s: moment_energy %.15e (fsum %+.1f ulp)  gauge_diff %.15e (%+.1f ulp)  force sum %.15e (%+.1f ulp) max %.15e  restoresu3 vs NumPy %.1e" %
          (tag, en, (en - eexact) / (u * eexact), diff, (diff - exact) / (u * exact), s.value, (s.value - fexact) / (u * fexact), m.value, err), file=sys.stderr)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TMLQCD_REF"), help="the reference tmLQCD source tree (default: $TMLQCD_REF)")
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "SO"))
    ap.add_argument("--keep-lib", action="store_true", help="also leave the harness library as oracle/_ref/libtmtraj.so (not committed; tools/traj_speed.py times its host loops)")
    a = ap.parse_args()
    if a.child:   # one lattice per process: the reference keeps its state in C globals
        gen(a.child[0], a.child[1])
        sys.exit(0)
    if not a.ref or not os.path.isdir(a.ref):
        sys.exit("make_golden_traj.py: give the reference tmLQCD source tree with --ref (or TMLQCD_REF)")
    with tempfile.TemporaryDirectory() as tmp:
        so = build_lib(a.ref, tmp)
        for tag in SHAPES:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", tag, so])
        if a.keep_lib:
            import shutil
            shutil.copy(so, os.path.join(ROOT, "oracle", "_ref", "libtmtraj.so"))
