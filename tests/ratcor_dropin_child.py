"""Child process of tests/test_gpu_ratcor_dropin.py.

A host program in miniature (tests/hostprog.py): the stub globals of tests/host_stub/globals.c (with its sw / sw_inv arrays)
plus the doublet's globals are loaded first, then libtmlqcd_dropin.so.  Calls the eight symbols tmlqcd_hip_{ratcor, cloverratcor,
ndratcor, ndcloverratcor}_{heatbath, acc} on host arrays in the residency mode given on the command line, with g_mu != 0 (the
single-flavour bodies run at twisted mass 0 and leave g_mu alone), the clover types after tmlqcd_hip_sw_term and tmlqcd_hip_sw_invert(EE,
0.) respectively sw_invert_nd, and prints the deviations from the reference's fixture (tests/golden/ref_ratcor_4x4.npz,
ref_ratcor_scalars_4x4.json) as one JSON line: relative for energies and fields, differences for the counts.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import hostprog  # noqa: E402
from tests.hostprog import rel_max  # noqa: E402

dbl, cint = C.c_double, C.c_int
G_MU = 0.17
ORDER = ("ratcor", "ndratcor", "cloverratcor", "ndcloverratcor")         # the single-flavour clover type before sw_invert_nd overwrites sw_inv


def main(mode):
    stub, ndg, d = hostprog.load(extra_c=hostprog.ND_GLOBALS)
    gold = os.path.join(ROOT, "tests", "golden")
    arrs = np.load(os.path.join(gold, "ref_ratcor_4x4.npz"))
    base = np.load(os.path.join(gold, "ref_nd_4x4.npz"))
    s = json.load(open(os.path.join(gold, "ref_ratcor_scalars_4x4.json")))
    T = L = 4
    V = T * L ** 3
    N = V // 2
    hostprog.init_lattice(stub, T, L, L, L, base["gauge"], s["kappa"])
    stub.stub_set_mu(G_MU)
    ndg.nd_set(s["mubar"], s["epsbar"], s["invmaxev"])
    stub.stub_init_clover(1)                                            # the host program's sw / sw_inv (init_sw_fields)
    errs = {}
    with hostprog.HostFields(stub, d, mode, modes=("coherent", "resident")) as hf:
        clover_made = False
        for name in ORDER:
            t = s["types"][name]
            c = t["fit"]
            if t["sw"] and not clover_made:
                d.tmlqcd_hip_sw_term(s["kappa"], s["c_sw"])
                d.tmlqcd_hip_sw_invert(0, 0.0)
                errs["sw_invert_failures"] = float(d.tmlqcd_hip_sw_invert_failures())
                clover_made = True
            if t["sw"] and t["nd"]:
                d.sw_invert_nd(s["mubar"] ** 2 - s["epsbar"] ** 2)
                errs["sw_invert_nd_failures"] = float(d.tmlqcd_hip_sw_invert_failures())
            n = c["np"]
            mu, rmu = (dbl * n)(*c["mu"]), (dbl * n)(*c["rmu"])
            pf = [hf.arr(N, base[k]) for k in (("k_s", "k_c") if t["nd"] else ("k_s",))]
            sfx = ("_up", "_dn")[:len(pf)]
            e, napp = dbl(), cint()
            rest = (mu, rmu, c["A"], n, c["max_iter"], c["accprec"], c["rel_prec"], C.byref(e), C.byref(napp))
            it = getattr(d, "tmlqcd_hip_%s_heatbath" % name)(*[p[1] for p in pf], *rest)
            hb = c["heatbath"]
            errs[name + "_heatbath_iters"] = abs(it - hb["iters"])
            errs[name + "_heatbath_napp"] = abs(napp.value - hb["napp"])
            errs[name + "_energy0"] = abs(e.value - hb["energy0"]) / hb["energy0"]
            errs[name + "_pf"] = max(rel_max(hf.copy(p), arrs[name + "_pf" + x]) for p, x in zip(pf, sfx))
            it = getattr(d, "tmlqcd_hip_%s_acc" % name)(*[p[1] for p in pf], *rest)
            ac = c["acc"]
            errs[name + "_acc_iters"] = abs(it - ac["iters"])
            errs[name + "_acc_napp"] = abs(napp.value - ac["napp"])
            errs[name + "_energy1"] = abs(e.value - ac["energy1"]) / abs(ac["energy1"])
        errs["g_mu_moved"] = abs(stub.stub_get_mu() - G_MU)
    hostprog.emit(errs)


if __name__ == "__main__":
    main(sys.argv[1])
