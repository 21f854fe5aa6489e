"""CPU: BiCGstab's entry points are exported and declared -- the core C-ABI (include/tmlqcd_hip.h) with its Python mirror, the three
reference-named symbols of the drop-in (include/tmlqcd_dropin.h) under the reference's signatures, and the operator ids appended
behind the two the multi-shift solver pinned."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ("tmhip_bicgstab_complex", "tmhip_assign_add_mul_add_mul", "tmhip_assign_mul_bra_add_mul_ket_add", "tmhip_bicg_update",
        "tmhip_bicg_pair_dot", "tmhip_bicg_sub", "tmhip_bicg_dir")
DROPIN = ("bicgstab_complex", "assign_add_mul_add_mul", "assign_mul_bra_add_mul_ket_add")


def _exports(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_core_symbols_exported_declared_and_mirrored():
    import tmlqcd_amd
    syms, hdr = _exports(os.path.join(LIB, "libtmlqcd_hip.so")), _header("tmlqcd_hip.h")
    lib = tmlqcd_amd.load_library()
    for name in CORE:
        assert name in syms, name
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        assert len(getattr(lib, name).argtypes) == len(m.group(1).split(",")), name
    for name in ("bicgstab_complex", "assign_add_mul_add_mul", "assign_mul_bra_add_mul_ket_add", "bicg_update", "bicg_pair_dot"):
        assert hasattr(tmlqcd_amd.Lattice, name), name


def test_dropin_declares_the_reference_signatures_and_exports_them():
    hdr = _header("tmlqcd_dropin.h")
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    cc = r"const\s+_Complex\s+double\s+"
    sp = r"spinor\s*\*\s*const\s+"
    # linalg/assign_add_mul_add_mul.h:26, linalg/assign_mul_bra_add_mul_ket_add.h:26
    for name in ("assign_add_mul_add_mul", "assign_mul_bra_add_mul_ket_add"):
        assert re.search(r"void\s+%s\(\s*%sR\s*,\s*%sS\s*,\s*%sU\s*,\s*%sc1\s*,\s*%sc2\s*,\s*const\s+int\s+N\s*\)\s*;" % (name, sp, sp, sp, cc, cc), hdr), name
    # solver/bicgstab_complex.h:26
    assert re.search(r"int\s+bicgstab_complex\(\s*%sP\s*,\s*%sQ\s*,\s*const\s+int\s+max_iter\s*,\s*double\s+eps_sq\s*,\s*const\s+int\s+rel_prec\s*,"
                     r"\s*const\s+int\s+N\s*,\s*matrix_mult\s+f\s*\)\s*;" % (sp, sp), hdr)
    for name in DROPIN:
        assert name in syms, name


def test_operator_ids_appended_behind_the_pinned_ones():
    import tmlqcd_amd.hip as h
    hdr = _header("tmlqcd_hip.h")
    assert "TMHIP_OP_QSW_PM = 5" in hdr and "TMHIP_OP_Q_PM_FULL = 6" in hdr
    ids = {n: int(v) for n, v in re.findall(r"\b(TMHIP_OP_[A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    want = {"TMHIP_OP_MTM_PLUS_SYM": 7, "TMHIP_OP_MTM_MINUS_SYM": 8, "TMHIP_OP_QSW_PLUS": 9, "TMHIP_OP_QSW_MINUS": 10, "TMHIP_OP_MSW_PLUS": 11,
            "TMHIP_OP_D_PSI": 12}
    for n, v in want.items():
        assert ids.get(n) == v, n
    assert sorted(ids.values()) == list(range(13))
    assert h.BICG_OPS == {"Qtm_plus_psi": ids["TMHIP_OP_QTM_PLUS"], "Qtm_minus_psi": ids["TMHIP_OP_QTM_MINUS"], "Mtm_plus_psi": ids["TMHIP_OP_MTM_PLUS"],
                          "Mtm_minus_psi": ids["TMHIP_OP_MTM_MINUS"], "Mtm_plus_sym_psi": 7, "Mtm_minus_sym_psi": 8, "Qsw_plus_psi": 9,
                          "Qsw_minus_psi": 10, "Msw_plus_psi": 11, "D_psi": 12}
    assert h.OPS == {"Qtm_pm_psi": 0, "Qtm_plus_psi": 1, "Qtm_minus_psi": 2, "Mtm_plus_psi": 3, "Mtm_minus_psi": 4, "Qsw_pm_psi": 5}   # cg_her's set is unchanged


def test_resource_guard_covers_the_new_kernels():
    table = open(os.path.join(LIB, "resource_usage.txt")).read()
    for k in ("cplx3_kernel<0>", "cplx3_kernel<1>", "bicghip::dot_kernel<false>", "bicghip::dot_kernel<true>", "bicghip::sub_kernel",
              "bicghip::update_kernel", "bicghip::dir_kernel"):
        row = [l for l in table.splitlines() if k in l]
        assert row and "(>= 8 waves)" in row[0] and row[0].rstrip().endswith("ok"), k
