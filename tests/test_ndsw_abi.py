"""CPU: the clover doublet's entry points are exported and declared -- the core C-ABI (include/tmlqcd_hip.h) with the argument counts
its Python mirror (tmlqcd_amd/hip.py) uses, the operators under their reference names and signatures in the drop-in
(include/tmlqcd_dropin.h), and the NDCLOVERRAT bodies of the drop-in."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tmlqcd_amd", "lib")
CORE = ["tmhip_sw_invert_nd", "tmhip_get_clover_nd", "tmhip_sw_invert_failures", "tmhip_assign_mul_one_sw_pm_imu_eps", "tmhip_clover_inv_nd",
        "tmhip_clover_gamma5_nd", "tmhip_Qsw_ndpsi", "tmhip_Qsw_dagger_ndpsi", "tmhip_Qsw_pm_ndpsi", "tmhip_Qsw_tau1_sub_const_ndpsi",
        "tmhip_H_eo_sw_ndpsi", "tmhip_Msw_ee_inv_ndpsi", "tmhip_cg_her_nd_op", "tmhip_cg_mms_tm_nd_op", "tmhip_sw_deriv_nd",
        "tmhip_ndcloverrat_force", "tmhip_ndcloverrat_derivative", "tmhip_ndcloverrat_heatbath", "tmhip_ndcloverrat_acc"]
FOUR = r"\(\s*spinor\s*\*\s*const\s+l_strange\s*,\s*spinor\s*\*\s*const\s+l_charm\s*,\s*spinor\s*\*\s*const\s+k_strange\s*,\s*spinor\s*\*\s*const\s+k_charm\s*"
# the reference's prototypes (operator/tm_operators_nd.h, operator/clovertm_operators.h, operator/clover_leaf.h)
DROPIN = {
    "sw_invert_nd": r"void\s+sw_invert_nd\(\s*const\s+double\s+mshift\s*\)\s*;",
    "sw_deriv_nd": r"void\s+sw_deriv_nd\(\s*const\s+int\s+ieo\s*\)\s*;",
    "assign_mul_one_sw_pm_imu_eps": r"void\s+assign_mul_one_sw_pm_imu_eps\(\s*const\s+int\s+ieo\s*,\s*spinor\s*\*\s*const\s+k_s\s*,\s*spinor\s*\*\s*const\s+k_c\s*,"
                                    r"\s*const\s+spinor\s*\*\s*const\s+l_s\s*,\s*const\s+spinor\s*\*\s*const\s+l_c\s*,\s*const\s+double\s+mu\s*,\s*const\s+double\s+eps\s*\)\s*;",
    "clover_inv_nd": r"void\s+clover_inv_nd\(\s*const\s+int\s+ieo\s*,\s*spinor\s*\*\s*const\s+l_c\s*,\s*spinor\s*\*\s*const\s+l_s\s*\)\s*;",
    "clover_gamma5_nd": r"void\s+clover_gamma5_nd\(\s*const\s+int\s+ieo\s*,\s*spinor\s*\*\s*const\s+l_c\s*,\s*spinor\s*\*\s*const\s+l_s\s*,"
                        r"\s*const\s+spinor\s*\*\s*const\s+k_c\s*,\s*const\s+spinor\s*\*\s*const\s+k_s\s*,\s*const\s+spinor\s*\*\s*const\s+j_c\s*,"
                        r"\s*const\s+spinor\s*\*\s*const\s+j_s\s*,\s*const\s+double\s+mubar\s*,\s*const\s+double\s+epsbar\s*\)\s*;",
    "Qsw_ndpsi": r"void\s+Qsw_ndpsi" + FOUR + r"\)\s*;",
    "Qsw_dagger_ndpsi": r"void\s+Qsw_dagger_ndpsi" + FOUR + r"\)\s*;",
    "Qsw_pm_ndpsi": r"void\s+Qsw_pm_ndpsi" + FOUR + r"\)\s*;",
    "Qsw_tau1_sub_const_ndpsi": r"void\s+Qsw_tau1_sub_const_ndpsi" + FOUR + r",\s*const\s+_Complex\s+double\s+z\s*,\s*const\s+double\s+Cpol\s*,\s*const\s+double\s+invev\s*\)\s*;",
    "H_eo_sw_ndpsi": r"void\s+H_eo_sw_ndpsi" + FOUR + r"\)\s*;",
    "Msw_ee_inv_ndpsi": r"void\s+Msw_ee_inv_ndpsi" + FOUR + r"\)\s*;",
}
BODIES = ["tmlqcd_hip_ndcloverrat_derivative", "tmlqcd_hip_ndcloverrat_heatbath", "tmlqcd_hip_ndcloverrat_acc", "tmlqcd_hip_sw_invert_failures"]


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
    assert re.search(r"TMHIP_ND_OP_QTM_PM\s*=\s*0\s*,\s*TMHIP_ND_OP_QSW_PM\s*=\s*1", hdr)
    assert hip.ND_OPS == {"Qtm_pm_ndpsi": 0, "Qsw_pm_ndpsi": 1}
    # the un-suffixed solver calls keep their signatures
    assert _nargs(hdr, "tmhip_cg_her_nd") + 1 == _nargs(hdr, "tmhip_cg_her_nd_op")
    assert _nargs(hdr, "tmhip_cg_mms_tm_nd") + 1 == _nargs(hdr, "tmhip_cg_mms_tm_nd_op")


def test_lattice_has_a_method_for_every_entry_point():
    from tmlqcd_amd import Lattice
    for n in CORE:
        if n in ("tmhip_cg_her_nd_op", "tmhip_cg_mms_tm_nd_op"):
            continue      # the op argument of Lattice.cg_her_nd / cg_mms_tm_nd
        assert callable(getattr(Lattice, n[len("tmhip_"):])), n


def test_dropin_carries_the_operators_under_their_reference_signatures():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    for n, rx in DROPIN.items():
        assert n in syms, n
        assert re.search(rx, hdr), n
    assert "Qsw_pm_ndpsi" in re.search(r"/\* solver/cg_her_nd\.c.*?\*/", hdr, re.S).group(0)


def test_dropin_carries_the_monomial_bodies():
    hdr = open(os.path.join(ROOT, "include", "tmlqcd_dropin.h")).read()
    syms = _exports(os.path.join(LIB, "libtmlqcd_dropin.so"))
    for n in BODIES:
        assert n in syms and re.search(r"\b%s\(" % n, hdr), n
