"""CPU: the chronological guess and its complex linalg are exported and declared -- the core C-ABI (include/tmlqcd_hip.h), the five
symbols under their reference names and signatures in the drop-in, and the Python mirror."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ["tmhip_scalar_prod", "tmhip_assign_diff_mul", "tmhip_mul", "tmhip_multi_scalar_prod", "tmhip_multi_assign_diff_mul",
        "tmhip_lincomb", "tmhip_chrono_guess", "tmhip_chrono_add_solution"]
DROPIN = ["scalar_prod", "assign_diff_mul", "mul", "chrono_guess", "chrono_add_solution"]
W = r"\s*"


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_core_symbols_exported_and_declared():
    syms = _exports(os.path.join(LIB, "libtmlqcd_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read()
    for n in CORE:
        assert n in syms, n
        assert re.search(r"\bint\s+%s\(tmhip_ctx \*ctx" % n, hdr), n
    assert "tmhip_csg_solve" in syms and re.search(r"\bint\s+tmhip_csg_solve\(int n", hdr)
    assert '"csg_batch"' in hdr and re.search(r"#define\s+TMHIP_CSG_MAX\s+20\b", hdr)


def test_python_mirror_declares_them():
    from tmlqcd_amd import hip
    lib = hip.load_library()
    for n in CORE:
        assert getattr(lib, n).argtypes is not None, n
    for m in ("scalar_prod", "assign_diff_mul", "mul", "multi_scalar_prod", "multi_assign_diff_mul", "lincomb", "chrono_guess",
              "chrono_add_solution"):
        assert callable(getattr(hip.Lattice, m)), m


def test_dropin_carries_them_under_their_reference_signatures():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    sp, spc = r"spinor\s*\*\s*const\s+", r"const\s+spinor\s*\*\s*const\s+"
    # linalg/scalar_prod.h, assign_diff_mul.h, mul.h
    assert re.search(r"_Complex\s+double\s+scalar_prod\(" + W + spc + "S" + W + "," + W + spc + "R" + W + r",\s*const\s+int\s+N\s*,\s*const\s+int\s+parallel\s*\)\s*;", hdr)
    assert re.search(r"void\s+assign_diff_mul\(" + W + sp + "S" + W + "," + W + sp + "R" + W + r",\s*const\s+_Complex\s+double\s+c\s*,\s*const\s+int\s+N\s*\)\s*;", hdr)
    assert re.search(r"void\s+mul\(" + W + sp + "R" + W + r",\s*const\s+_Complex\s+double\s+c\s*," + W + sp + "S" + W + r",\s*const\s+int\s+N\s*\)\s*;", hdr)
    # solver/chrono_guess.h
    assert re.search(r"int\s+chrono_guess\(" + W + sp + "trial" + W + "," + W + sp + "phi" + W + r",\s*spinor\s*\*\*\s*const\s+v\s*,\s*int\s+index_array\[\]\s*,"
                     r"\s*const\s+int\s+_N\s*,\s*const\s+int\s+_n\s*,\s*const\s+int\s+V\s*,\s*matrix_mult\s+f\s*\)\s*;", hdr)
    assert re.search(r"void\s+chrono_add_solution\(" + W + sp + "trial" + W + r",\s*spinor\s*\*\*\s*const\s+v\s*,\s*int\s+index_array\[\]\s*,"
                     r"\s*const\s+int\s+_N\s*,\s*int\s*\*\s*_n\s*,\s*const\s+int\s+V\s*\)\s*;", hdr)
    assert set(DROPIN) <= _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))


def test_resource_guard_lists_the_batched_kernels():
    table = open(os.path.join(LIB, "resource_usage.txt")).read()
    for k, tag in (("csg_dot_kernel", "batched scalar_prod"), ("csg_axpy_kernel", "batched assign_diff_mul"), ("csg_lincomb_kernel", "lincomb")):
        rows = [l for l in table.splitlines() if l.startswith("void %s<" % k)]
        assert rows and all(tag + " (>= 8 waves)" in l and l.rstrip().endswith("ok") for l in rows), k
