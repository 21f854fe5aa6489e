"""CPU: the entry points of the clover rational monomial, the batched sw_spinor_eo and the tr-log energies are exported and declared --
the core C-ABI (include/tmlqcd_hip.h) with the argument counts its Python mirror (tmlqcd_amd/hip.py) uses, sw_trace / sw_trace_nd under
their reference names and signatures in the drop-in (include/tmlqcd_dropin.h), and the CLOVERRAT bodies of the drop-in."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ["tmhip_sw_spinor_eo_batch", "tmhip_sw_trace", "tmhip_sw_trace_nd", "tmhip_sw_trace_failures",
        "tmhip_cloverrat_force", "tmhip_cloverrat_derivative", "tmhip_cloverrat_heatbath", "tmhip_cloverrat_acc"]
# the reference's prototypes (operator/clover_leaf.h)
DROPIN = {
    "sw_trace": r"double\s+sw_trace\(\s*const\s+int\s+ieo\s*,\s*const\s+double\s+mu\s*\)\s*;",
    "sw_trace_nd": r"double\s+sw_trace_nd\(\s*const\s+int\s+ieo\s*,\s*const\s+double\s+mu\s*,\s*const\s+double\s+eps\s*\)\s*;",
}
BODIES = ["tmlqcd_hip_cloverrat_derivative", "tmlqcd_hip_cloverrat_heatbath", "tmlqcd_hip_cloverrat_acc", "tmlqcd_hip_sw_trace_failures"]


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def _nargs(hdr, name):
    """number of parameters of `int name(...)` as the header declares it"""
    m = re.search(r"\bint\s+%s\(([^;]*?)\)\s*;" % name, hdr, re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_core_symbols_exported_declared_and_mirrored_with_matching_argument_counts():
    from tmlqcd_amd import hip
    lib = hip.load_library()
    syms = _exports(os.path.join(LIB, "libtmlqcd_hip.so"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmlqcd_hip.h")).read(), flags=re.S)
    for n in CORE:
        assert n in syms, n
        assert re.search(r"\bint\s+%s\(tmhip_ctx \*ctx" % n, hdr), n
        assert getattr(lib, n).argtypes is not None and len(getattr(lib, n).argtypes) == _nargs(hdr, n), n
    # the batched call takes the pairs the way deriv_Sb_batch does, and the clover monomial the arguments of rat plus (kappa, c_sw, trlog)
    assert _nargs(hdr, "tmhip_sw_spinor_eo_batch") == _nargs(hdr, "tmhip_deriv_Sb_batch")
    assert _nargs(hdr, "tmhip_cloverrat_force") == _nargs(hdr, "tmhip_rat_force") + 3
    assert _nargs(hdr, "tmhip_cloverrat_derivative") == _nargs(hdr, "tmhip_rat_derivative") + 3
    assert _nargs(hdr, "tmhip_cloverrat_heatbath") == _nargs(hdr, "tmhip_rat_heatbath")
    assert _nargs(hdr, "tmhip_cloverrat_acc") == _nargs(hdr, "tmhip_rat_acc")


def test_lattice_has_a_method_for_every_entry_point():
    from tmlqcd_amd import Lattice
    for n in CORE:
        assert callable(getattr(Lattice, n[len("tmhip_"):])), n


def test_dropin_carries_the_trlog_energies_under_their_reference_signatures():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    for n, rx in DROPIN.items():
        assert n in syms, n
        assert re.search(rx, hdr), n
    assert not re.search(r"Not here:[^/]*sw_trace", hdr)


def test_dropin_carries_the_monomial_bodies():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    for n in BODIES:
        assert n in syms and re.search(r"\b%s\(" % n, hdr), n


def test_resource_guard_lists_the_new_kernels_within_their_floors():
    """the table the build writes (tools/check_resources.py): no scratch, three waves per SIMD for the batched kernel, two for the traces"""
    rows = open(os.path.join(LIB, "resource_usage.txt")).read().splitlines()
    for name, floor in (("sw_spinor_eo_batch_kernel", 3), ("sw_trace_kernel<true>", 2), ("sw_trace_kernel<false>", 2)):
        row = [r for r in rows if re.match(r"(void )?%s\s" % re.escape(name), r)]
        assert len(row) == 1, name
        assert "(>= %d waves)" % floor in row[0] and row[0].rstrip().endswith("ok"), row[0]
