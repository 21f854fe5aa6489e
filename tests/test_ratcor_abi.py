"""CPU: the correction monomials (ratcor family) are declared, exported and mirrored -- core library, drop-in and the ctypes
layer name the same functions, and the option that selects the path of apply_Z is documented next to its siblings."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")

CORE = ["tmhip_rat_sum", "tmhip_rat_sum_nd", "tmhip_diff_sqnorm", "tmhip_diff_sqnorm_nd", "tmhip_apply_Z", "tmhip_apply_Z_nd",
        "tmhip_ratcor_heatbath", "tmhip_ratcor_acc", "tmhip_ndratcor_heatbath", "tmhip_ndratcor_acc"]
DROPIN = ["tmlqcd_hip_%s_%s" % (t, b) for t in ("ratcor", "cloverratcor", "ndratcor", "ndcloverratcor") for b in ("heatbath", "acc")]
METHODS = ["rat_sum", "rat_sum_nd", "diff_sqnorm", "diff_sqnorm_nd", "apply_Z", "apply_Z_nd", "ratcor_heatbath", "ratcor_acc",
           "ndratcor_heatbath", "ndratcor_acc"]


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def declared(name):
    txt = re.sub(r"/\*.*?\*/", "", header(name), flags=re.S)
    return set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", txt))


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, lib)], capture_output=True, text=True, check=True).stdout
    return set(l.split()[-1] for l in out.splitlines() if l.strip())


def test_core_symbols_are_declared_and_exported():
    dec, exp = declared("tmlqcd_hip.h"), exported("libtmlqcd_hip.so")
    for n in CORE:
        assert n in dec, n
        assert n in exp, n


def test_dropin_symbols_are_declared_and_exported():
    dec, exp = declared("tmlqcd_dropin.h"), exported("libtmlqcd_dropin.so")
    for n in DROPIN:
        assert n in dec, n
        assert n in exp, n


def test_python_mirror_declares_them():
    import tmlqcd_amd
    lib = tmlqcd_amd.load_library()
    for n in CORE:
        f = getattr(lib, n)
        assert f.argtypes is not None and len(f.argtypes) >= 4, n
    for m in METHODS:
        assert callable(getattr(tmlqcd_amd.Lattice, m)), m
    # the bodies take the operator, so that one function serves the tm and the clover type
    for m in ("apply_Z", "apply_Z_nd", "ratcor_heatbath", "ratcor_acc", "ndratcor_heatbath", "ndratcor_acc"):
        assert "op" in inspect.signature(getattr(tmlqcd_amd.Lattice, m)).parameters, m


def test_option_and_the_six_term_cap_are_documented_in_the_header():
    txt = header("tmlqcd_hip.h")
    assert '"ratcor_fused"' in txt
    opts = txt[txt.index('"rat_batch" shifts per group'):]
    assert '"ratcor_fused"' in opts[:opts.index('"gauge_global_sums"')]          # listed next to "rat_batch" / "poly_batch"
    assert "at most SIX times" in txt and "check_C_psi" in txt
    assert "ratcor_monomial.c:183-218" in txt and "ndratcor_monomial.c:202-245" in txt
