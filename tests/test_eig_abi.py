"""CPU: the eigenvalue measurement's entry points are exported, declared and mirrored -- the core C-ABI (include/tmlqcd_hip.h) with
its Python mirror, the solver bit TMHIP_S_EIG on exactly the three Hermitian positive single-flavour rows of the operator table,
the three symbols of the drop-in (include/tmlqcd_dropin.h), and the resource rules of the new kernels."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ("tmhip_eigenvalues", "tmhip_eigenvalues_nd", "tmhip_eig_set_interval", "tmhip_eig_dots", "tmhip_eig_project", "tmhip_basis_rotate",
        "tmhip_eig_small")
DROPIN = ("eigenvalues_bi", "tmlqcd_hip_phmc_compute_ev", "tmlqcd_hip_eigenvalues")


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_core_symbols_exported_declared_and_mirrored():
    import tmlqcd_amd
    import tmlqcd_amd.hip as h
    syms, hdr = _exports(os.path.join(LIB, "libtmlqcd_hip.so")), _read("include", "tmlqcd_hip.h")
    lib = tmlqcd_amd.load_library()
    for name in CORE:
        assert name in syms, name
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(getattr(lib, name).argtypes) == len(args.split(",")), name
    assert re.search(r"#define\s+TMHIP_EIG_MAX_BASIS\s+64\b", hdr)
    for name in ("eigenvalues", "eigenvalues_nd", "eig_dots", "eig_project", "basis_rotate", "eig_set_interval"):
        assert hasattr(tmlqcd_amd.Lattice, name), name
    assert callable(h.eig_small)


def test_the_solver_bit_sits_on_the_three_hermitian_positive_rows():
    text = _read("tmlqcd_amd", "csrc", "op_table.h")
    assert re.search(r"\bTMHIP_S_EIG\s*=\s*64\b", text)
    rows = re.findall(r"\bX\(([^)]*)\)", text.split("#define TMHIP_OP_TABLE(X)")[1].split("struct tmhip_op_row")[0])
    rows = [tuple(c.strip() for c in r.split(",")) for r in rows]
    single = [r for r in rows if r[1].endswith("_psi")]
    assert {r[1] for r in single if "TMHIP_S_EIG" in r[5].split(" | ")} == {"Qtm_pm_psi", "Qsw_pm_psi", "Q_pm_psi"}
    doublet = [r for r in rows if r[1].endswith("_ndpsi")]
    assert [r[5] for r in doublet] == ["TMHIP_S_ND", "TMHIP_S_ND"]


def test_dropin_declares_and_exports_the_three_symbols():
    hdr = _read("include", "tmlqcd_dropin.h")
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    assert re.search(r"double\s+eigenvalues_bi\(\s*int\s*\*\s*nev\s*,\s*const\s+int\s+max_iterations\s*,\s*const\s+double\s+prec\s*,\s*const\s+int\s+maxmin\s*,"
                     r"\s*matrix_mult_bi\s+Qsq\s*\)\s*;", hdr)
    assert re.search(r"int\s+tmlqcd_hip_phmc_compute_ev\(\s*const\s+int\s+trajectory_counter\s*,\s*const\s+int\s+id\s*,\s*const\s+char\s*\*\s*name\s*,"
                     r"\s*const\s+double\s+EVMin\s*,\s*const\s+int\s+clover\s*,\s*const\s+double\s+prec\s*,\s*double\s*\*\s*ev_min\s*,\s*double\s*\*\s*ev_max\s*\)\s*;", hdr)
    assert re.search(r"double\s+tmlqcd_hip_eigenvalues\(\s*int\s*\*\s*nev\s*,\s*const\s+int\s+max_iterations\s*,\s*const\s+double\s+prec\s*,\s*const\s+int\s+maxmin\s*,"
                     r"\s*spinor\s*\*\s*evecs\s*,\s*double\s*\*\s*evals\s*\)\s*;", hdr)
    src = _read("tmlqcd_amd", "csrc", "dropin.cpp")
    for fn in ("Qtm_pm_ndbipsi", "Qsw_pm_ndbipsi"):
        assert re.search(r"void\s+%s\([^)]*\)\s*__attribute__\(\(weak\)\)" % fn, src), fn
        assert fn not in syms, fn                    # the reference's functions: weak references, never defined here
    for name in DROPIN:
        assert name in syms, name


def test_resource_guard_covers_the_new_kernels():
    table = _read("tmlqcd_amd", "lib", "resource_usage.txt")
    for k, floor in (("eighip::eig_dots_kernel", 8), ("eighip::eig_project_kernel", 8), ("eighip::eig_scale_kernel", 8), ("eighip::eig_cheb_kernel", 8),
                     ("eighip::basis_rotate_kernel<8>", 8), ("eighip::basis_rotate_kernel<16>", 6), ("eighip::basis_rotate_kernel<32>", 3),
                     ("eighip::basis_rotate_kernel<64>", 1)):
        row = [l for l in table.splitlines() if k in l]
        assert row and "(>= %d waves)" % floor in row[0] and row[0].rstrip().endswith("ok"), k
