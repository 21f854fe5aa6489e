"""CPU: the rational monomials' entry points are exported and declared -- the core C-ABI (include/tmlqcd_hip.h), the two building
blocks under their reference names and signatures in the drop-in, and the monomial bodies of the drop-in."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ["tmhip_deriv_Sb_batch", "tmhip_Q_tau1_sub_const_ndpsi", "tmhip_assign_add_mul",
        "tmhip_ndrat_force", "tmhip_ndrat_derivative", "tmhip_ndrat_heatbath", "tmhip_ndrat_acc",
        "tmhip_rat_force", "tmhip_rat_derivative", "tmhip_rat_heatbath", "tmhip_rat_acc"]
BODIES = ["tmlqcd_hip_ndrat_derivative", "tmlqcd_hip_ndrat_heatbath", "tmlqcd_hip_ndrat_acc",
          "tmlqcd_hip_rat_derivative", "tmlqcd_hip_rat_heatbath", "tmlqcd_hip_rat_acc"]


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_core_symbols_exported_and_declared():
    syms = _exports(os.path.join(LIB, "libtmlqcd_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    for n in CORE:
        assert n in syms, n
        assert re.search(r"\bint\s+%s\(tmhip_ctx \*ctx" % n, hdr), n
    assert '"rat_batch"' in hdr


def test_python_mirror_declares_them():
    from tmlqcd_amd import hip
    lib = hip.load_library()
    for n in CORE:
        assert getattr(lib, n).argtypes is not None, n


def test_dropin_carries_the_building_blocks_under_their_reference_signatures():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    # operator/tm_operators_nd.h: Q_tau1_sub_const_ndpsi(l_strange, l_charm, k_strange, k_charm, z, Cpol, invev)
    assert re.search(r"void\s+Q_tau1_sub_const_ndpsi\(\s*spinor\s*\*\s*const\s+l_strange\s*,\s*spinor\s*\*\s*const\s+l_charm\s*,\s*spinor\s*\*\s*const\s+k_strange\s*,"
                     r"\s*spinor\s*\*\s*const\s+k_charm\s*,\s*const\s+_Complex\s+double\s+z\s*,\s*const\s+double\s+Cpol\s*,\s*const\s+double\s+invev\s*\)\s*;", hdr)
    # linalg/assign_add_mul.h: assign_add_mul(P, Q, c, N)
    assert re.search(r"void\s+assign_add_mul\(\s*spinor\s*\*\s*const\s+P\s*,\s*spinor\s*\*\s*const\s+Q\s*,\s*const\s+_Complex\s+double\s+c\s*,\s*const\s+int\s+N\s*\)\s*;", hdr)
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    assert {"Q_tau1_sub_const_ndpsi", "assign_add_mul"} <= syms


def test_dropin_carries_the_monomial_bodies():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    for n in BODIES:
        assert n in syms and re.search(r"\b%s\(" % n, hdr), n
