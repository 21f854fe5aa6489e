"""CPU: the polynomial monomial's entry points are exported and declared -- the core C-ABI (include/tmlqcd_hip.h) with its Python
mirror, the two building blocks under their reference names in the drop-in, and the three monomial bodies of the drop-in."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ["tmhip_assign_mul_add_mul_add_mul_add_mul_r", "tmhip_comb4_ndpsi", "tmhip_Ptilde_ndpsi", "tmhip_ndpoly_derivative", "tmhip_ndpoly_heatbath",
        "tmhip_ndpoly_acc"]
DROPIN = ["assign_mul_add_mul_add_mul_add_mul_r", "Ptilde_ndpsi", "tmlqcd_hip_ndpoly_derivative", "tmlqcd_hip_ndpoly_heatbath", "tmlqcd_hip_ndpoly_acc"]
METHODS = ["assign_mul_add_mul_add_mul_add_mul_r", "comb4_ndpsi", "Ptilde_ndpsi", "ndpoly_derivative", "ndpoly_heatbath", "ndpoly_acc"]


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def _declaration(hdr, name):
    m = re.search(r"\bint\s+%s\(tmhip_ctx \*ctx([^;]*)\)\s*;" % name, hdr)
    assert m, name
    return m.group(1)


def test_core_symbols_exported_and_declared():
    syms = _exports(os.path.join(LIB, "libtmlqcd_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    for n in CORE:
        assert n in syms, n
        _declaration(hdr, n)
    assert '"poly_batch"' in hdr


def test_python_mirror_declares_them_with_matching_argument_counts():
    from tmlqcd_amd import hip
    lib = hip.load_library()
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in CORE:
        args = getattr(lib, n).argtypes
        assert args is not None, n
        assert len(args) == 1 + _declaration(hdr, n).count(","), n          # ctx + one per comma of the C declaration
    for m in METHODS:
        assert callable(getattr(hip.Lattice, m)), m


def test_dropin_carries_the_reference_names_and_the_monomial_bodies():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    for n in DROPIN:
        assert n in syms and re.search(r"\b%s\(" % n, hdr), n
    # linalg/assign_mul_add_mul_add_mul_add_mul_r.h and Ptilde_nd.h: the reference's signatures
    assert re.search(r"void\s+assign_mul_add_mul_add_mul_add_mul_r\(\s*spinor\s*\*\s*const\s+R\s*,\s*spinor\s*\*\s*const\s+S\s*,\s*spinor\s*\*\s*const\s+U\s*,"
                     r"\s*spinor\s*\*\s*const\s+V\s*,\s*const\s+double\s+c1\s*,\s*const\s+double\s+c2\s*,\s*const\s+double\s+c3\s*,\s*const\s+double\s+c4\s*,"
                     r"\s*const\s+int\s+N\s*\)\s*;", hdr)
    assert re.search(r"void\s+Ptilde_ndpsi\(\s*spinor\s*\*\s*R_s\s*,\s*spinor\s*\*\s*R_c\s*,\s*double\s*\*\s*dd\s*,\s*int\s+n\s*,\s*spinor\s*\*\s*S_s\s*,"
                     r"\s*spinor\s*\*\s*S_c\s*,\s*matrix_mult_nd\s+Qsq\s*\)\s*;", hdr)
