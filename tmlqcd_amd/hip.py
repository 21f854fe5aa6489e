"""ctypes mirror of include/tmlqcd_hip.h (host-side plumbing only; no numerics here).

Function names follow the reference (operator/tm_operators.h, linalg/*.h, solver/cg_her.h);
host arrays are numpy float64 in the reference's AoS layouts:
  spinor field [nsites][4][3][2]  (su3.h:60-63),  gauge field [VPR][4][3][3][2]  (su3.h:40-43).
"""
import ctypes as C
import os
import numpy as np

EO, OE = 0, 1
FIELD_EO, FIELD_FULL = 0, 1
# The operator ids of include/tmlqcd_hip.h by the reference's function: TMHIP_OP_* and TMHIP_ND_OP_* (tests/test_op_table.py holds
# both maps against the header).  Which solver takes which row is the library's business (csrc/op_table.h): it refuses the others.
ALL_OPS = {"Qtm_pm_psi": 0, "Qtm_plus_psi": 1, "Qtm_minus_psi": 2, "Mtm_plus_psi": 3, "Mtm_minus_psi": 4, "Qsw_pm_psi": 5, "Q_pm_psi": 6,
           "Mtm_plus_sym_psi": 7, "Mtm_minus_sym_psi": 8, "Qsw_plus_psi": 9, "Qsw_minus_psi": 10, "Msw_plus_psi": 11, "D_psi": 12}
ND_OPS = {"Qtm_pm_ndpsi": 0, "Qsw_pm_ndpsi": 1}
# the names each wrapper below accepts (Q_pm_psi and D_psi: FULL fields, N = VOLUME; the others EO fields, N = VOLUME/2)
OPS, MMS_OPS, BICG_OPS = ({n: ALL_OPS[n] for n in names.split()} for names in (
    "Qtm_pm_psi Qtm_plus_psi Qtm_minus_psi Mtm_plus_psi Mtm_minus_psi Qsw_pm_psi", "Qtm_pm_psi Qsw_pm_psi Q_pm_psi",
    "Qtm_plus_psi Qtm_minus_psi Mtm_plus_psi Mtm_minus_psi Mtm_plus_sym_psi Mtm_minus_sym_psi Qsw_plus_psi Qsw_minus_psi Msw_plus_psi D_psi"))
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class TmHipError(RuntimeError):
    pass


def library_path():
    # TMLQCD_HIP_LIB: another build of the same library (A/B runs of kernel variants, tools/)
    return os.environ.get("TMLQCD_HIP_LIB") or os.path.join(_HERE, "lib", "libtmlqcd_hip.so")


class GaugeInfo(C.Structure):
    """tmhip_gauge_info (include/tmlqcd_hip.h): what the reference keeps in GaugeInfo after read_gauge_field."""
    _fields_ = [("gauge_read", C.c_int), ("suma", C.c_uint), ("sumb", C.c_uint), ("suma_stored", C.c_uint), ("sumb_stored", C.c_uint),
                ("prec", C.c_int), ("lx", C.c_int), ("ly", C.c_int), ("lz", C.c_int), ("lt", C.c_int),
                ("xlf_info", C.c_char * 1024), ("ildg_data_lfn", C.c_char * 512)]


class SpinorInfo(C.Structure):
    """tmhip_spinor_info (include/tmlqcd_hip.h): what read_spinor found -- precision, propagator type, the record read, both checksums."""
    _fields_ = [("prec", C.c_int), ("prop_type", C.c_int), ("position", C.c_int), ("checksum_read", C.c_int),
                ("suma", C.c_uint), ("sumb", C.c_uint), ("suma_stored", C.c_uint), ("sumb_stored", C.c_uint)]


class _Geom(C.Structure):
    _fields_ = [("T", C.c_int), ("LX", C.c_int), ("LY", C.c_int), ("LZ", C.c_int),
                ("nproc_t", C.c_int), ("proc_t", C.c_int)]


def load_library():
    """Load libtmlqcd_hip.so.  Fails loudly: there is no fallback path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise TmHipError("%s not built -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(or make -C tmlqcd_amd/csrc); there is no CPU fallback" % path)
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    pd = C.POINTER(C.c_double)
    sig = {
        "tmhip_create": [C.POINTER(_Geom), i, C.POINTER(vp)],
        "tmhip_sync": [vp],
        "tmhip_set_boundary": [vp, d, pd],
        "tmhip_set_mu": [vp, d],
        "tmhip_set_mu3": [vp, d],
        "tmhip_set_gauge": [vp, vp],
        "tmhip_field_alloc": [vp, i, C.POINTER(vp)],
        "tmhip_field_upload": [vp, vp, vp, i],
        "tmhip_field_download": [vp, vp, vp, i],
        "tmhip_field_zero": [vp, vp],
        "tmhip_field_raw": [vp, vp, vp, i, C.POINTER(i)],
        "tmhip_hopping_matrix": [vp, i, vp, vp],
        "tmhip_hopping_matrix_nocom": [vp, i, vp, vp],
        "tmhip_tm_times_hopping_matrix": [vp, i, vp, vp, d, d],
        "tmhip_tm_sub_hopping_matrix": [vp, i, vp, vp, vp, d, d],
        "tmhip_D_psi": [vp, vp, vp],
        "tmhip_mul_one_pm_imu_inv": [vp, vp, d, i],
        "tmhip_assign_mul_one_pm_imu_inv": [vp, vp, vp, d, i],
        "tmhip_assign_mul_one_pm_imu": [vp, vp, vp, d, i],
        "tmhip_mul_one_pm_imu": [vp, vp, d],
        "tmhip_mul_one_pm_imu_sub_mul": [vp, vp, vp, vp, d, i],
        "tmhip_mul_one_pm_imu_sub_mul_gamma5": [vp, vp, vp, vp, d],
        "tmhip_gamma5": [vp, vp, vp, i],
        "tmhip_H_eo_tm_inv_psi": [vp, vp, vp, i, d],
        "tmhip_Qtm_plus_psi": [vp, vp, vp], "tmhip_Qtm_minus_psi": [vp, vp, vp],
        "tmhip_Mtm_plus_psi": [vp, vp, vp], "tmhip_Mtm_minus_psi": [vp, vp, vp],
        "tmhip_Qtm_pm_psi": [vp, vp, vp],
        "tmhip_Qtm_plus_sym_psi": [vp, vp, vp], "tmhip_Qtm_minus_sym_psi": [vp, vp, vp],
        "tmhip_Mtm_plus_sym_psi": [vp, vp, vp], "tmhip_Mtm_minus_sym_psi": [vp, vp, vp],
        "tmhip_Mtm_plus_sym_dagg_psi": [vp, vp, vp], "tmhip_Qtm_pm_sym_psi": [vp, vp, vp],
        "tmhip_mul_one_sub_mul_gamma5": [vp, vp, vp, vp],
        "tmhip_M_full": [vp, vp, vp, vp, vp],
        "tmhip_square_norm": [vp, vp, i, i, pd],
        "tmhip_scalar_prod_r": [vp, vp, vp, i, i, pd],
        "tmhip_assign_add_mul_r": [vp, vp, vp, d, i],
        "tmhip_assign_mul_add_r": [vp, vp, d, vp, i],
        "tmhip_assign_mul_add_r_and_square": [vp, vp, d, vp, i, i, pd],
        "tmhip_diff": [vp, vp, vp, vp, i],
        "tmhip_assign": [vp, vp, vp, i],
        "tmhip_add": [vp, vp, vp, vp, i],
        "tmhip_mul_r": [vp, vp, d, vp, i],
        "tmhip_cg_her": [vp, vp, vp, i, d, i, i, i, C.POINTER(i), pd, i],
        "tmhip_assign_add_mul_add_mul": [vp, vp, vp, vp, d, d, d, d, i],
        "tmhip_assign_mul_bra_add_mul_ket_add": [vp, vp, vp, vp, d, d, d, d, i],
        "tmhip_bicgstab_complex": [vp, vp, vp, i, d, i, i, i, C.POINTER(i), pd, i],
        "tmhip_bicg_update": [vp, vp, vp, vp, vp, vp, vp, pd, pd, i, pd],
        "tmhip_bicg_pair_dot": [vp, vp, vp, i, pd],
        "tmhip_bicg_sub": [vp, vp, vp, vp, pd, i],
        "tmhip_bicg_dir": [vp, vp, vp, vp, pd, pd, i],
        "tmhip_set_clover": [vp, vp, vp],
        "tmhip_sw_term": [vp, vp, d, d],
        "tmhip_momenta_upload": [vp, vp], "tmhip_momenta_download": [vp, vp], "tmhip_update_momenta": [vp, d],
        "tmhip_update_gauge": [vp, d], "tmhip_gauge_download": [vp, vp],
        "tmhip_gauge_snapshot": [vp], "tmhip_gauge_restore": [vp], "tmhip_gauge_snapshot_free": [vp], "tmhip_gauge_reunitarize": [vp],
        "tmhip_gauge_snapshot_diff": [vp, pd], "tmhip_moment_energy": [vp, pd], "tmhip_derivative_norms": [vp, pd, pd],
        "tmhip_derivative_upload": [vp, vp], "tmhip_transfer_counts": [vp, C.POINTER(C.c_longlong)],
        "tmhip_bench_trajectory_forms": [vp, i, i, pd],
        "tmhip_gauge_derivative": [vp, d, d, d, i, d],
        "tmhip_measure_plaquette": [vp, pd], "tmhip_measure_gauge_action": [vp, d, pd], "tmhip_measure_rectangles": [vp, pd],
        "tmhip_measure_field_strength": [vp, pd, pd], "tmhip_flow_begin": [vp], "tmhip_flow_step": [vp, d],
        "tmhip_flow_observables": [vp, pd, pd, pd], "tmhip_flow_download": [vp, vp], "tmhip_flow_end": [vp],
        "tmhip_gradient_flow": [vp, d, d, i, pd, C.POINTER(i)],
        "tmhip_slice_correlators": [vp, vp, vp, i, pd, pd, pd], "tmhip_polyakov_loop": [vp, i, pd, pd],
        "tmhip_measure_oriented_plaquettes": [vp, pd],
        "tmhip_gauge_unpack_ildg": [vp, vp, i, C.POINTER(C.c_uint)], "tmhip_gauge_pack_ildg": [vp, vp, i, C.POINTER(C.c_uint)],
        "tmhip_read_gauge_field": [vp, C.c_char_p, i, i, vp, C.POINTER(GaugeInfo)],
        "tmhip_write_gauge_field": [vp, C.c_char_p, i, C.c_char_p, C.POINTER(C.c_uint)],
        "tmhip_spinor_pack": [vp, vp, vp, vp, i, C.POINTER(C.c_uint)], "tmhip_spinor_unpack": [vp, vp, vp, vp, i, C.POINTER(C.c_uint)],
        "tmhip_read_spinor": [vp, vp, vp, C.c_char_p, i, i, C.POINTER(SpinorInfo)],
        "tmhip_write_spinor": [vp, C.c_char_p, i, C.POINTER(vp), C.POINTER(vp), i, i, C.POINTER(C.c_uint)],
        "tmhip_write_lime_message": [C.c_char_p, i, C.c_char_p, C.c_char_p, i, i],
        "tmhip_source_point": [vp, vp, vp, i, i, C.c_longlong],
        "tmhip_bench_spinor_io": [vp, vp, vp, i, i, i, pd],
        "tmhip_gauge_su3_deviation": [vp, pd],
        "tmhip_gauge_pack_stats": [vp, C.POINTER(C.c_longlong)], "tmhip_gauge_pack_build_ms": [vp, pd],
        "tmhip_gauge_pack_launches": [vp, C.POINTER(C.c_longlong)], "tmhip_gauge_pack_format": [vp, C.POINTER(i)],
        "tmhip_derivative_zero": [vp],
        "tmhip_swpm_zero": [vp], "tmhip_sw_spinor_eo": [vp, i, vp, vp, d], "tmhip_sw_deriv": [vp, i, d],
        "tmhip_sw_all": [vp, vp, d, d], "tmhip_get_swpm": [vp, vp, vp],
        "tmhip_deriv_Sb": [vp, i, vp, vp, d],
        "tmhip_derivative_download": [vp, vp, i],
        "tmhip_multi_deriv_Sb": [i, C.POINTER(vp), i, C.POINTER(vp), C.POINTER(vp), d],
        "tmhip_multi_sw_all": [i, C.POINTER(vp), d, d],
        "tmhip_multi_update_gauge": [i, C.POINTER(vp), d],
        "tmhip_sw_invert": [vp, i, d],
        "tmhip_get_clover": [vp, vp, vp],
        "tmhip_clover_inv": [vp, vp, i, d],
        "tmhip_clover_gamma5": [vp, i, vp, vp, vp, d],
        "tmhip_clover": [vp, i, vp, vp, vp, d],
        "tmhip_H_eo_sw_inv_psi": [vp, vp, vp, i, i, d],
        "tmhip_Qsw_pm_psi": [vp, vp, vp],
        "tmhip_Msw_plus_psi": [vp, vp, vp],
        "tmhip_Qsw_psi": [vp, vp, vp], "tmhip_Qsw_plus_psi": [vp, vp, vp], "tmhip_Qsw_minus_psi": [vp, vp, vp],
        "tmhip_Qsw_sq_psi": [vp, vp, vp], "tmhip_Msw_psi": [vp, vp, vp], "tmhip_Msw_minus_psi": [vp, vp, vp],
        "tmhip_Msw_full": [vp, vp, vp, vp, vp],
        "tmhip_assign_mul_one_sw_pm_imu": [vp, i, vp, vp, d], "tmhip_assign_mul_one_sw_pm_imu_inv": [vp, i, vp, vp, d],
        "tmhip_Qsw_pm_psi_32": [vp, vp, vp],
        "tmhip_field_alloc32": [vp, C.POINTER(vp)],
        "tmhip_field_upload32": [vp, vp, vp, i],
        "tmhip_field_download32": [vp, vp, vp, i],
        "tmhip_assign_to_32": [vp, vp, vp, i],
        "tmhip_assign_to_64": [vp, vp, vp, i],
        "tmhip_add_from_32": [vp, vp, vp, i],
        "tmhip_hopping_matrix_32": [vp, i, vp, vp],
        "tmhip_Qtm_pm_psi_32": [vp, vp, vp],
        "tmhip_square_norm_32": [vp, vp, i, i, pd],
        "tmhip_scalar_prod_r_32": [vp, vp, vp, i, i, pd],
        "tmhip_assign_add_mul_r_32": [vp, vp, vp, C.c_float, i],
        "tmhip_assign_mul_add_r_32": [vp, vp, C.c_float, vp, i],
        "tmhip_mixed_cg_her": [vp, vp, vp, i, d, i, i, i, d, i, C.POINTER(i), C.POINTER(i)],
        "tmhip_mixed_cg_restarts": [vp, C.POINTER(i), i, C.POINTER(i)],
        "tmhip_rg_mixed_cg_her": [vp, vp, vp, i, d, i, i, i, d, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)],
        "tmhip_comm_get_unique_id": [C.c_char_p],
        "tmhip_comm_init": [vp, C.c_char_p],
        "tmhip_comm_init_shm": [vp, C.c_char_p],
        "tmhip_comm_init_ipc": [vp],
        "tmhip_comm_faces_direct": [vp, C.POINTER(i)],
        "tmhip_comm_sums_direct": [vp],
        "tmhip_comm_set_loopback": [vp, i],
        "tmhip_comm_count": [vp, C.POINTER(i), C.POINTER(i)],
        "tmhip_comm_is_split": [vp],
        "tmhip_comm_stream_delay_ms": [vp, i],
        "tmhip_bench_hopping": [vp, vp, vp, vp, i, pd],
        "tmhip_multi_hopping_matrix": [i, C.POINTER(vp), i, C.POINTER(vp), C.POINTER(vp)],
        "tmhip_event_record": [vp, i],
        "tmhip_event_elapsed_ms": [vp, i, i, pd],
        "tmhip_set_option": [vp, C.c_char_p, i],
        "tmhip_set_nd": [vp, d, d, d],
        "tmhip_M_ee_inv_ndpsi": [vp, vp, vp, vp, vp, d, d],
        "tmhip_M_oo_sub_g5_ndpsi": [vp, vp, vp, vp, vp, vp, vp, d, d],
        "tmhip_Qtm_ndpsi": [vp, vp, vp, vp, vp], "tmhip_Qtm_dagger_ndpsi": [vp, vp, vp, vp, vp],
        "tmhip_Qtm_pm_ndpsi": [vp, vp, vp, vp, vp],
        "tmhip_H_eo_tm_ndpsi": [vp, vp, vp, vp, vp, i],
        "tmhip_cg_her_nd": [vp, vp, vp, vp, vp, i, d, i, i, C.POINTER(i)],
        "tmhip_cg_mms_tm_nd": [vp, C.POINTER(vp), C.POINTER(vp), vp, vp, pd, i, i, d, i, C.POINTER(i)],
        "tmhip_nd_active_shifts": [vp],
        "tmhip_M_ee_inv_ndpsi_32": [vp, vp, vp, vp, vp, C.c_float, C.c_float],
        "tmhip_M_oo_sub_g5_ndpsi_32": [vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float],
        "tmhip_Qtm_pm_ndpsi_32": [vp, vp, vp, vp, vp],
        "tmhip_rg_mixed_cg_her_nd": [vp, vp, vp, vp, vp, i, d, i, i, i, d, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)],
        "tmhip_cg_mms_tm":[vp, C.POINTER(vp), vp, pd, i, i, d, i, i, i, C.POINTER(i), pd],
        "tmhip_mms_active_shifts": [vp],
        "tmhip_mms_form": [vp],
        "tmhip_deriv_Sb_batch": [vp, i, i, C.POINTER(vp), C.POINTER(vp), pd],
        "tmhip_Q_tau1_sub_const_ndpsi": [vp, vp, vp, vp, vp, d, d, d, d],
        "tmhip_assign_add_mul": [vp, vp, vp, d, d, i],
        "tmhip_scalar_prod": [vp, vp, vp, i, i, pd], "tmhip_assign_diff_mul": [vp, vp, vp, d, d, i], "tmhip_mul": [vp, vp, d, d, vp, i],
        "tmhip_multi_scalar_prod": [vp, i, C.POINTER(vp), vp, i, pd], "tmhip_multi_assign_diff_mul": [vp, i, C.POINTER(vp), vp, pd, i],
        "tmhip_lincomb": [vp, vp, i, C.POINTER(vp), pd, i],
        "tmhip_chrono_guess": [vp, vp, vp, C.POINTER(vp), i, i, i, pd, pd], "tmhip_chrono_add_solution": [vp, vp, vp, i],
        "tmhip_csg_solve": [i, pd, pd],
        "tmhip_ndrat_force": [vp, C.POINTER(vp), C.POINTER(vp), pd, pd, i, d],
        "tmhip_ndrat_derivative": [vp, vp, vp, pd, pd, i, d, i, d, i, C.POINTER(i)],
        "tmhip_ndrat_heatbath": [vp, vp, vp, pd, pd, i, d, i, d, i, pd, C.POINTER(i)],
        "tmhip_ndrat_acc": [vp, vp, vp, pd, pd, i, i, d, i, pd, C.POINTER(i)],
        "tmhip_sw_invert_nd": [vp, d], "tmhip_get_clover_nd": [vp, vp], "tmhip_sw_invert_failures": [vp, C.POINTER(i)],
        "tmhip_assign_mul_one_sw_pm_imu_eps": [vp, i, vp, vp, vp, vp, d, d],
        "tmhip_clover_inv_nd": [vp, i, vp, vp],
        "tmhip_clover_gamma5_nd": [vp, i, vp, vp, vp, vp, vp, vp, d, d],
        "tmhip_Qsw_ndpsi": [vp, vp, vp, vp, vp], "tmhip_Qsw_dagger_ndpsi": [vp, vp, vp, vp, vp],
        "tmhip_Qsw_pm_ndpsi": [vp, vp, vp, vp, vp],
        "tmhip_Qsw_tau1_sub_const_ndpsi": [vp, vp, vp, vp, vp, d, d, d, d],
        "tmhip_H_eo_sw_ndpsi": [vp, vp, vp, vp, vp], "tmhip_Msw_ee_inv_ndpsi": [vp, vp, vp, vp, vp],
        "tmhip_cg_her_nd_op": [vp, vp, vp, vp, vp, i, d, i, i, i, C.POINTER(i)],
        "tmhip_cg_mms_tm_nd_op": [vp, C.POINTER(vp), C.POINTER(vp), vp, vp, pd, i, i, d, i, i, C.POINTER(i)],
        "tmhip_mixed_cg_mms_tm_nd": [vp, C.POINTER(vp), C.POINTER(vp), vp, vp, pd, i, i, d, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)],
        "tmhip_sw_deriv_nd": [vp, i],
        "tmhip_ndcloverrat_force": [vp, C.POINTER(vp), C.POINTER(vp), pd, pd, i, d, d, d, i],
        "tmhip_ndcloverrat_derivative": [vp, vp, vp, pd, pd, i, d, d, d, i, i, d, i, C.POINTER(i)],
        "tmhip_ndcloverrat_heatbath": [vp, vp, vp, pd, pd, i, d, i, d, i, pd, C.POINTER(i)],
        "tmhip_ndcloverrat_acc": [vp, vp, vp, pd, pd, i, i, d, i, pd, C.POINTER(i)],
        "tmhip_rat_force": [vp, C.POINTER(vp), pd, i],
        "tmhip_rat_derivative": [vp, vp, pd, pd, i, i, d, i, C.POINTER(i)],
        "tmhip_rat_heatbath": [vp, vp, pd, pd, i, i, d, i, pd, C.POINTER(i)],
        "tmhip_rat_acc": [vp, vp, pd, pd, i, i, d, i, pd, C.POINTER(i)],
        "tmhip_sw_spinor_eo_batch": [vp, i, i, C.POINTER(vp), C.POINTER(vp), pd],
        "tmhip_sw_trace": [vp, i, d, i, pd], "tmhip_sw_trace_nd": [vp, i, d, d, i, pd], "tmhip_sw_trace_failures": [vp],
        "tmhip_cloverrat_force": [vp, C.POINTER(vp), pd, i, d, d, i],
        "tmhip_cloverrat_derivative": [vp, vp, pd, pd, i, d, d, i, i, d, i, C.POINTER(i)],
        "tmhip_cloverrat_heatbath": [vp, vp, pd, pd, i, i, d, i, pd, C.POINTER(i)],
        "tmhip_cloverrat_acc": [vp, vp, pd, pd, i, i, d, i, pd, C.POINTER(i)],
        "tmhip_rat_sum": [vp, vp, vp, C.POINTER(vp), pd, i, d],
        "tmhip_rat_sum_nd": [vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp), pd, i, d],
        "tmhip_diff_sqnorm": [vp, vp, vp, pd], "tmhip_diff_sqnorm_nd": [vp, vp, vp, vp, vp, pd],
        "tmhip_apply_Z": [vp, vp, vp, pd, pd, d, i, i, d, i, i, pd, C.POINTER(i)],
        "tmhip_apply_Z_nd": [vp, vp, vp, vp, vp, pd, pd, d, i, i, d, i, i, pd, C.POINTER(i)],
        "tmhip_ratcor_heatbath": [vp, vp, pd, pd, d, i, i, d, i, i, pd, C.POINTER(i), C.POINTER(i)],
        "tmhip_ratcor_acc": [vp, vp, pd, pd, d, i, i, d, i, i, pd, C.POINTER(i), C.POINTER(i)],
        "tmhip_ndratcor_heatbath": [vp, vp, vp, pd, pd, d, i, i, d, i, i, pd, C.POINTER(i), C.POINTER(i)],
        "tmhip_ndratcor_acc": [vp, vp, vp, pd, pd, d, i, i, d, i, i, pd, C.POINTER(i), C.POINTER(i)],
        "tmhip_assign_mul_add_mul_add_mul_add_mul_r": [vp, vp, vp, vp, vp, d, d, d, d],
        "tmhip_comb4_ndpsi": [vp] + [vp] * 10 + [d, d, d, d],
        "tmhip_Ptilde_ndpsi": [vp, vp, vp, pd, i, vp, vp, d, d, i],
        "tmhip_ndpoly_derivative": [vp, vp, vp, pd, i, d, d],
        "tmhip_ndpoly_heatbath": [vp, vp, vp, pd, i, d, d, pd, i, d, d, pd],
        "tmhip_ndpoly_acc": [vp, vp, vp, pd, i, d, d, pd, pd, i, d, d, d, pd, C.POINTER(i), pd],
        "tmhip_eigenvalues": [vp, i, i, i, i, d, i, C.POINTER(vp), pd, pd, C.POINTER(i), C.POINTER(i)],
        "tmhip_eigenvalues_nd": [vp, i, i, i, d, i, C.POINTER(vp), C.POINTER(vp), pd, pd, C.POINTER(i), C.POINTER(i)],
        "tmhip_eig_set_interval": [vp, d, d],
        "tmhip_eig_dots": [vp, i, C.POINTER(vp), C.POINTER(vp), vp, vp, i, pd],
        "tmhip_eig_project": [vp, i, C.POINTER(vp), C.POINTER(vp), vp, vp, pd, i, pd],
        "tmhip_basis_rotate": [vp, i, i, C.POINTER(vp), C.POINTER(vp), pd, i],
        "tmhip_eig_small": [i, pd, pd],
        "tmhip_cvfield_alloc": [vp, C.POINTER(vp)], "tmhip_cvfield_upload": [vp, vp, vp], "tmhip_cvfield_download": [vp, vp, vp],
        "tmhip_cvfield_zero": [vp, vp], "tmhip_cvfield_upload_slices": [vp, vp, vp, i, i], "tmhip_cvfield_download_slices": [vp, vp, vp, i, i],
        "tmhip_laph_apply": [vp, vp, vp, i, i], "tmhip_laph_apply_dot": [vp, vp, vp, i, i, pd],
        "tmhip_laph_apply_filter": [vp, vp, vp, vp, i, i, pd],
        "tmhip_laph_dots": [vp, i, C.POINTER(vp), vp, i, i, C.POINTER(i), pd],
        "tmhip_laph_project": [vp, i, C.POINTER(vp), vp, pd, i, i, C.POINTER(i), pd],
        "tmhip_laph_normalise": [vp, vp, vp, i, i, C.POINTER(i), pd],
        "tmhip_laph_rotate": [vp, i, i, C.POINTER(vp), pd, i, i, C.POINTER(i)],
        "tmhip_laph_set_interval": [vp, d, d], "tmhip_laph_timing": [vp, pd],
        "tmhip_laph_eigensystem": [vp, i, i, i, d, i, C.POINTER(vp), pd, pd, C.POINTER(i), C.POINTER(i)],
        "tmhip_laph_write": [vp, C.c_char_p, i, i, i, i, C.POINTER(vp), pd],
        "tmhip_get_option": [vp, C.c_char_p, C.POINTER(i)],
    }
    for name, args in sig.items():
        f = getattr(lib, name)
        f.argtypes = args
        f.restype = i
    lib.tmhip_destroy.argtypes = [vp]
    lib.tmhip_destroy.restype = None
    lib.tmhip_field_free.argtypes = [vp, vp]
    lib.tmhip_field_free.restype = None
    lib.tmhip_cvfield_free.argtypes = [vp, vp]
    lib.tmhip_cvfield_free.restype = None
    lib.tmhip_field_even.argtypes = [vp]
    lib.tmhip_field_even.restype = vp
    lib.tmhip_field_odd.argtypes = [vp]
    lib.tmhip_field_odd.restype = vp
    lib.tmhip_version.restype = C.c_char_p
    lib.tmhip_device_count.restype = i
    _LIB = lib
    return lib


def _ck(rc, what):
    if rc != 0:
        raise TmHipError("%s failed (rc=%d); see stderr" % (what, rc))


def _hp(a):
    if a.dtype != np.float64 or not a.flags["C_CONTIGUOUS"]:
        raise TmHipError("host arrays must be C-contiguous float64")
    return a.ctypes.data_as(C.c_void_p)


def csg_solve(G, b):
    """The small solve of chrono_guess alone (tmhip_csg_solve; host code, no device needed): y with G y = b."""
    G = np.array(G, dtype=np.complex128, order="C")
    b = np.array(b, dtype=np.complex128, order="C")
    pd = C.POINTER(C.c_double)
    _ck(load_library().tmhip_csg_solve(len(b), G.view(np.float64).ctypes.data_as(pd), b.view(np.float64).ctypes.data_as(pd)), "csg_solve")
    return b


def eig_small(A):
    """The small symmetric eigenproblem of the eigensolver alone (tmhip_eig_small; host code, no device needed): (w ascending, Y with
    the eigenvectors by column) of the real symmetric matrix A, n <= 64."""
    Y = np.array(A, dtype=np.float64, order="C")
    n = Y.shape[0]
    w = np.zeros(n)
    pd = C.POINTER(C.c_double)
    _ck(load_library().tmhip_eig_small(n, Y.ctypes.data_as(pd), w.ctypes.data_as(pd)), "eig_small")
    return w, Y


def write_lime_message(filename, record_type, text, mb, me, append=True):
    """One message record of a LIME file (tmhip_write_lime_message): the "propagator-type", "inversion-info", ... records around the
    data of a propagator file; the text is the caller's."""
    _ck(load_library().tmhip_write_lime_message(str(filename).encode(), 1 if append else 0, record_type.encode(), text.encode(), mb, me),
        "tmhip_write_lime_message")


class Field:
    """A device-resident spinor field (opaque handle); prec 32 = the reference's spinor32."""

    def __init__(self, lat, kind=FIELD_EO, handle=None, owner=True, prec=64):
        self.lat, self.kind, self.owner, self.prec = lat, kind, owner, prec
        if handle is None:
            h = C.c_void_p()
            if prec == 32:
                _ck(lat.lib.tmhip_field_alloc32(lat.h, C.byref(h)), "tmhip_field_alloc32")
            else:
                _ck(lat.lib.tmhip_field_alloc(lat.h, kind, C.byref(h)), "tmhip_field_alloc")
            handle = h
        self.h = handle

    def upload(self, host, nsites=None):
        nsites = nsites if nsites is not None else (self.lat.V if self.kind == FIELD_FULL else self.lat.Vh)
        if self.prec == 32:
            if host.dtype != np.float32 or not host.flags["C_CONTIGUOUS"]:
                raise TmHipError("fp32 fields take C-contiguous float32 arrays")
            _ck(self.lat.lib.tmhip_field_upload32(self.lat.h, self.h, host.ctypes.data_as(C.c_void_p), nsites), "tmhip_field_upload32")
            return self
        _ck(self.lat.lib.tmhip_field_upload(self.lat.h, self.h, _hp(host), nsites), "tmhip_field_upload")
        return self

    def download(self, nsites=None, out=None):
        """Returns the field as a host AoS array; `out`: an existing fp64 array of the right shape to fill instead (a host
        program's own, already touched, buffer)."""
        nsites = nsites if nsites is not None else (self.lat.V if self.kind == FIELD_FULL else self.lat.Vh)
        if out is not None:
            if self.prec == 32 or out.dtype != np.float64 or out.shape != (nsites, 4, 3, 2) or not out.flags.c_contiguous:
                raise TmHipError("download(out=...): needs a C-contiguous float64 [%d][4][3][2] array and an fp64 field" % nsites)
            _ck(self.lat.lib.tmhip_field_download(self.lat.h, self.h, _hp(out), nsites), "tmhip_field_download")
            return out
        if self.prec == 32:
            out = np.empty((nsites, 4, 3, 2), dtype=np.float32)
            _ck(self.lat.lib.tmhip_field_download32(self.lat.h, self.h, out.ctypes.data_as(C.c_void_p), nsites), "tmhip_field_download32")
            return out
        out = np.empty((nsites, 4, 3, 2), dtype=np.float64)
        _ck(self.lat.lib.tmhip_field_download(self.lat.h, self.h, _hp(out), nsites), "tmhip_field_download")
        return out

    def zero(self):
        _ck(self.lat.lib.tmhip_field_zero(self.lat.h, self.h), "tmhip_field_zero")
        return self

    def raw(self, planes=None):
        """The planes of an fp64 one-parity field as they lie in HBM, float64 [12][stride][2] with the padding entries [Vh, stride):
        returned, or -- `planes` given -- written to the device."""
        ns = C.c_int()
        _ck(self.lat.lib.tmhip_field_raw(self.lat.h, self.h, None, 0, C.byref(ns)), "tmhip_field_raw")
        if planes is not None:
            if planes.shape != (12, ns.value, 2):
                raise TmHipError("raw(planes): needs a float64 [12][%d][2] array" % ns.value)
            _ck(self.lat.lib.tmhip_field_raw(self.lat.h, self.h, _hp(planes), 1, None), "tmhip_field_raw")
            return self
        out = np.empty((12, ns.value, 2))
        _ck(self.lat.lib.tmhip_field_raw(self.lat.h, self.h, _hp(out), 0, None), "tmhip_field_raw")
        return out

    def even(self):
        return Field(self.lat, FIELD_EO, C.c_void_p(self.lat.lib.tmhip_field_even(self.h)), owner=False)

    def odd(self):
        return Field(self.lat, FIELD_EO, C.c_void_p(self.lat.lib.tmhip_field_odd(self.h)), owner=False)

    def free(self):
        if self.owner and self.h is not None and self.lat.h is not None:
            self.lat.lib.tmhip_field_free(self.lat.h, self.h)
        self.h = None


class CvField:
    """A device-resident colour-vector field (opaque handle): T x LX LY LZ sites of three complex doubles, the reference's
    su3_vector [T][SPACEVOLUME]; host arrays are float64 [T][SPACEVOLUME][3][2]."""

    def __init__(self, lat):
        self.lat = lat
        h = C.c_void_p()
        _ck(lat.lib.tmhip_cvfield_alloc(lat.h, C.byref(h)), "tmhip_cvfield_alloc")
        self.h = h

    def _shape(self):
        return (self.lat.T, self.lat.V // self.lat.T, 3, 2)

    def upload(self, host):
        if host.shape != self._shape():
            raise TmHipError("colour-vector fields take float64 [T][SPACEVOLUME][3][2] arrays, got %s" % (host.shape,))
        _ck(self.lat.lib.tmhip_cvfield_upload(self.lat.h, self.h, _hp(host)), "tmhip_cvfield_upload")
        return self

    def download(self):
        out = np.empty(self._shape(), dtype=np.float64)
        _ck(self.lat.lib.tmhip_cvfield_download(self.lat.h, self.h, _hp(out)), "tmhip_cvfield_download")
        return out

    def zero(self):
        _ck(self.lat.lib.tmhip_cvfield_zero(self.lat.h, self.h), "tmhip_cvfield_zero")
        return self

    def free(self):
        if self.h is not None and self.lat.h is not None:
            self.lat.lib.tmhip_cvfield_free(self.lat.h, self.h)
        self.h = None


class Lattice:
    """One rank's lattice on one MI355X: context + operators, mirroring the reference's names."""

    def __init__(self, T, LX, LY, LZ, kappa=0.125, mu=0.0, theta=(0, 0, 0, 0), nproc_t=1, proc_t=0, device=0):
        self.lib = load_library()
        self.T, self.LX, self.LY, self.LZ = T, LX, LY, LZ
        self.nproc_t, self.proc_t = nproc_t, proc_t
        self.V = T * LX * LY * LZ
        self.Vh = self.V // 2
        self.VPR = self.V + (2 * LX * LY * LZ if nproc_t > 1 else 0)
        g = _Geom(T, LX, LY, LZ, nproc_t, proc_t)
        h = C.c_void_p()
        self.h = None
        _ck(self.lib.tmhip_create(C.byref(g), device, C.byref(h)), "tmhip_create")
        self.h = h
        self.set_boundary(kappa, theta)
        self.set_mu(mu)

    def close(self):
        if self.h is not None:
            self.lib.tmhip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- parameters -------------------------------------------------------
    def set_boundary(self, kappa, theta=(0, 0, 0, 0)):
        th = (C.c_double * 4)(*theta)
        _ck(self.lib.tmhip_set_boundary(self.h, kappa, th), "tmhip_set_boundary")

    def set_mu(self, mu):
        self.mu = mu
        _ck(self.lib.tmhip_set_mu(self.h, mu), "tmhip_set_mu")

    def set_mu3(self, mu3):
        _ck(self.lib.tmhip_set_mu3(self.h, mu3), "tmhip_set_mu3")

    def set_gauge(self, g):
        if g.shape != (self.VPR, 4, 3, 3, 2):
            raise TmHipError("gauge field must be [VPR=%d][4][3][3][2], got %s" % (self.VPR, g.shape))
        _ck(self.lib.tmhip_set_gauge(self.h, _hp(g)), "tmhip_set_gauge")

    def set_option(self, name, value):
        _ck(self.lib.tmhip_set_option(self.h, name.encode(), int(value)), "tmhip_set_option")

    def get_option(self, name):
        """the value an option has now (the eigensolvers' options: "eig_basis", "eig_cheb", "eig_fused", "eig_restarts", "laph_basis",
        "laph_cheb", "laph_fused")"""
        out = C.c_int()
        _ck(self.lib.tmhip_get_option(self.h, name.encode(), C.byref(out)), "tmhip_get_option")
        return out.value

    def gauge_su3_deviation(self):
        """max |row2 - conj(row0 x row1)| over the resident links (what the gauge_recon=12 guard looks at)."""
        out = C.c_double()
        _ck(self.lib.tmhip_gauge_su3_deviation(self.h, C.byref(out)), "tmhip_gauge_su3_deviation")
        return out.value

    def gauge_pack_stats(self):
        """(packed 0/1, links on rotation 0, 1, 2, links without an exact rotation) of the packed twin of the gauge copy
        (option gauge_pack); builds it if it is stale."""
        out = (C.c_longlong * 5)()
        _ck(self.lib.tmhip_gauge_pack_stats(self.h, out), "tmhip_gauge_pack_stats")
        return tuple(int(v) for v in out)

    def gauge_pack_format(self):
        """bytes per link the stencil reads of the packed twin: 104 (compact rows, option gauge_pack_compact), 112, or 0 where the
        field is read in full; builds the twin if it is stale."""
        out = C.c_int()
        _ck(self.lib.tmhip_gauge_pack_format(self.h, C.byref(out)), "tmhip_gauge_pack_format")
        return out.value

    def gauge_pack_launches(self):
        """stencil launches that read the packed copy so far"""
        out = C.c_longlong()
        _ck(self.lib.tmhip_gauge_pack_launches(self.h, C.byref(out)), "tmhip_gauge_pack_launches")
        return out.value

    def gauge_pack_build_ms(self):
        """device time of the last build of the packed twin, in ms"""
        out = C.c_double()
        _ck(self.lib.tmhip_gauge_pack_build_ms(self.h, C.byref(out)), "tmhip_gauge_pack_build_ms")
        return out.value

    def sync(self):
        _ck(self.lib.tmhip_sync(self.h), "tmhip_sync")

    # --- fields -----------------------------------------------------------
    def field(self, host=None, kind=FIELD_EO):
        f = Field(self, kind)
        if host is not None:
            f.upload(host, host.shape[0])
        return f

    def full_field(self, host=None):
        return self.field(host, FIELD_FULL)

    def field32(self, host=None):
        f = Field(self, FIELD_EO, prec=32)
        if host is not None:
            f.upload(host, host.shape[0])
        return f

    # --- clover twisted mass (operator/clovertm_operators.h) ---------------
    def set_clover(self, sw, sw_inv):
        """sw [V][3][2][3][3][2] from sw_term, sw_inv [V][4][2][3][3][2] from sw_invert(EE, mu) (host arrays)."""
        if sw.shape != (self.V, 3, 2, 3, 3, 2) or sw_inv.shape != (self.V, 4, 2, 3, 3, 2):
            raise TmHipError("clover arrays must be [V][3][2][3][3][2] and [V][4][2][3][3][2]")
        _ck(self.lib.tmhip_set_clover(self.h, _hp(sw), _hp(sw_inv)), "tmhip_set_clover")

    # --- fermion force (deriv_Sb.h) ------------------------------------------
    def derivative_zero(self):
        _ck(self.lib.tmhip_derivative_zero(self.h), "tmhip_derivative_zero")

    def deriv_Sb(self, ieo, l, k, factor):
        """deriv_Sb.c:401: accumulate the hopping part of the fermion force into the device-resident derivative field."""
        _ck(self.lib.tmhip_deriv_Sb(self.h, ieo, l.h, k.h, factor), "deriv_Sb")

    def deriv_Sb_batch(self, ieo, ls, ks, factors):
        """sum_j deriv_Sb(ieo, ls[j], ks[j], factors[j]) in one kernel launch (1 <= len <= 64 pairs; unsplit lattices)."""
        n = len(ls)
        if len(ks) != n or len(factors) != n:
            raise TmHipError("deriv_Sb_batch: ls, ks and factors must have the same length")
        m = max(n, 1)
        _ck(self.lib.tmhip_deriv_Sb_batch(self.h, ieo, n, (C.c_void_p * m)(*[f.h for f in ls]), (C.c_void_p * m)(*[f.h for f in ks]),
                                          (C.c_double * m)(*factors)), "deriv_Sb_batch")

    def derivative(self, into=None):
        """The accumulated derivative as su3adj df[V][4][8]; with `into`, added to that host array (accumulate)."""
        if into is None:
            out = np.zeros((self.V, 4, 8))
            _ck(self.lib.tmhip_derivative_download(self.h, _hp(out), 0), "tmhip_derivative_download")
            return out
        _ck(self.lib.tmhip_derivative_download(self.h, _hp(into), 1), "tmhip_derivative_download")
        return into

    # --- clover part of the force (clover_deriv.c, clover_accumulate_deriv.c) ---
    def swpm_zero(self):
        _ck(self.lib.tmhip_swpm_zero(self.h), "tmhip_swpm_zero")

    def sw_spinor_eo(self, ieo, kk, ll, fac):
        _ck(self.lib.tmhip_sw_spinor_eo(self.h, ieo, kk.h, ll.h, fac), "sw_spinor_eo")

    def sw_spinor_eo_batch(self, ieo, kks, lls, facs):
        """sum_j sw_spinor_eo(ieo, kks[j], lls[j], facs[j]) in one kernel launch (1 <= len <= 64 pairs): swm / swp move once."""
        n = len(kks)
        if len(lls) != n or len(facs) != n:
            raise TmHipError("sw_spinor_eo_batch: kks, lls and facs must have the same length")
        m = max(n, 1)
        _ck(self.lib.tmhip_sw_spinor_eo_batch(self.h, ieo, n, (C.c_void_p * m)(*[f.h for f in kks]), (C.c_void_p * m)(*[f.h for f in lls]),
                                              (C.c_double * m)(*facs)), "sw_spinor_eo_batch")

    def sw_deriv(self, ieo, mu):
        _ck(self.lib.tmhip_sw_deriv(self.h, ieo, mu), "sw_deriv")

    # --- tr-log energies on the device's clover term (operator/clover_det.c) ---
    def sw_trace(self, ieo, mu, global_sum=None):
        """clover_det.c:115: sum over the sites of parity ieo and both chiralities of log |det(1 + T + i mu)|^2.  global_sum: add the
        shares of the T-split ranks (default: whenever the lattice is split, as the reference's MPI_Allreduce)."""
        out = C.c_double()
        g = self.nproc_t > 1 if global_sum is None else bool(global_sum)
        _ck(self.lib.tmhip_sw_trace(self.h, ieo, mu, int(g), C.byref(out)), "sw_trace")
        return out.value

    def sw_trace_nd(self, ieo, mu, eps, global_sum=None):
        """clover_det.c:202: sum over the sites of parity ieo of log(Re det_0 Re det_1), det_i = det((1 + T_i)^2 + mu^2 - eps^2)."""
        out = C.c_double()
        g = self.nproc_t > 1 if global_sum is None else bool(global_sum)
        _ck(self.lib.tmhip_sw_trace_nd(self.h, ieo, mu, eps, int(g), C.byref(out)), "sw_trace_nd")
        return out.value

    def sw_trace_failures(self):
        """pivots below the reference's tiny_t met by the last sw_trace / sw_trace_nd (six_det's ifail)"""
        return self.lib.tmhip_sw_trace_failures(self.h)

    def sw_all(self, kappa, c_sw, gauge=None):
        _ck(self.lib.tmhip_sw_all(self.h, _hp(gauge) if gauge is not None else None, kappa, c_sw), "sw_all")

    def get_swpm(self):
        swm, swp = np.zeros((self.V, 4, 3, 3, 2)), np.zeros((self.V, 4, 3, 3, 2))
        _ck(self.lib.tmhip_get_swpm(self.h, _hp(swm), _hp(swp)), "tmhip_get_swpm")
        return swm, swp

    def sw_term(self, gauge, kappa, c_sw):
        """operator/clover_term.c:88 on the device; `gauge` as for set_gauge ([VPR][4][3][3][2]), or None = the links resident
        on the device (after set_gauge / update_gauge)."""
        if gauge is not None and gauge.shape != (self.VPR, 4, 3, 3, 2):
            raise TmHipError("gauge field must be [%d][4][3][3][2]" % self.VPR)
        _ck(self.lib.tmhip_sw_term(self.h, _hp(gauge) if gauge is not None else None, kappa, c_sw), "tmhip_sw_term")

    # --- molecular dynamics with the links resident in HBM (update_gauge.c, update_momenta.c) ---------------
    def momenta_upload(self, mom):
        if mom.shape != (self.V, 4, 8):
            raise TmHipError("momenta must be [V=%d][4][8]" % self.V)
        _ck(self.lib.tmhip_momenta_upload(self.h, _hp(mom)), "tmhip_momenta_upload")

    def momenta_download(self):
        out = np.zeros((self.V, 4, 8))
        _ck(self.lib.tmhip_momenta_download(self.h, _hp(out)), "tmhip_momenta_download")
        return out

    def update_momenta(self, step):
        _ck(self.lib.tmhip_update_momenta(self.h, step), "update_momenta")

    def update_gauge(self, step):
        _ck(self.lib.tmhip_update_gauge(self.h, step), "update_gauge")

    def gauge_download(self):
        out = np.zeros((self.VPR, 4, 3, 3, 2))
        _ck(self.lib.tmhip_gauge_download(self.h, _hp(out)), "tmhip_gauge_download")
        return out

    # --- the frame of a trajectory on the resident fields (update_tm.c, moment_energy.c, monitor_forces.c) ---------------
    def gauge_snapshot(self):
        """gauge_tmp <- links (update_tm.c:109-121), in a device buffer of its own."""
        _ck(self.lib.tmhip_gauge_snapshot(self.h), "gauge_snapshot")

    def gauge_restore(self):
        """links <- gauge_tmp (update_tm.c:329-339, reject); the stencil's copy follows, the clover blocks become stale."""
        _ck(self.lib.tmhip_gauge_restore(self.h), "gauge_restore")

    def gauge_snapshot_free(self):
        _ck(self.lib.tmhip_gauge_snapshot_free(self.h), "gauge_snapshot_free")

    def gauge_reunitarize(self):
        """restoresu3_in_place on every link (update_tm.c:313-328, accept); derived state as after update_gauge."""
        _ck(self.lib.tmhip_gauge_reunitarize(self.h), "gauge_reunitarize")

    def gauge_snapshot_diff(self):
        """sum over the own links of sqrt(|U - U_tmp|_F^2) (update_tm.c:233-272)."""
        out = C.c_double(0.0)
        _ck(self.lib.tmhip_gauge_snapshot_diff(self.h, C.byref(out)), "gauge_snapshot_diff")
        return out.value

    def moment_energy(self):
        """0.5 * sum over the own links of |P|^2 of the resident momenta (moment_energy.c:46-74)."""
        out = C.c_double(0.0)
        _ck(self.lib.tmhip_moment_energy(self.h, C.byref(out)), "moment_energy")
        return out.value

    def derivative_norms(self):
        """(sum, max) over the own links of d1^2 + ... + d8^2 of the resident derivative (monitor_forces.c:64-89)."""
        s, m = C.c_double(0.0), C.c_double(0.0)
        _ck(self.lib.tmhip_derivative_norms(self.h, C.byref(s), C.byref(m)), "derivative_norms")
        return s.value, m.value

    def transfer_counts(self):
        """whole-field copies so far: (set_gauge, gauge_download, momenta_upload, momenta_download)"""
        out = (C.c_longlong * 4)()
        _ck(self.lib.tmhip_transfer_counts(self.h, out), "tmhip_transfer_counts")
        return tuple(int(v) for v in out)

    def bench_trajectory_forms(self, form, reps):
        """device ms per call of one form of the reject / accept pass (tmhip_bench_trajectory_forms)"""
        out = C.c_double(0.0)
        _ck(self.lib.tmhip_bench_trajectory_forms(self.h, form, reps, C.byref(out)), "tmhip_bench_trajectory_forms")
        return out.value

    def derivative_upload(self, df):
        """su3adj df[V][4][8] (host) replaces the device derivative field."""
        if df.shape != (self.V, 4, 8):
            raise TmHipError("derivative must be [V=%d][4][8]" % self.V)
        _ck(self.lib.tmhip_derivative_upload(self.h, _hp(df)), "tmhip_derivative_upload")

    # --- gauge monomial on the resident links (monomial/gauge_monomial.c, measure_gauge_action.c, measure_rectangles.c) ---
    def gauge_derivative(self, beta, c0=1.0, c1=0.0, use_rectangles=False, glambda=0.0):
        """gauge_derivative / gauge_EMderivative (glambda != 0): added to the device-resident derivative field."""
        _ck(self.lib.tmhip_gauge_derivative(self.h, beta, c0, c1, 1 if use_rectangles else 0, glambda), "gauge_derivative")

    def measure_plaquette(self):
        out = C.c_double(0.0)
        _ck(self.lib.tmhip_measure_plaquette(self.h, C.byref(out)), "measure_plaquette")
        return out.value

    def measure_gauge_action(self, glambda=0.0):
        out = C.c_double(0.0)
        _ck(self.lib.tmhip_measure_gauge_action(self.h, glambda, C.byref(out)), "measure_gauge_action")
        return out.value

    def measure_rectangles(self):
        out = C.c_double(0.0)
        _ck(self.lib.tmhip_measure_rectangles(self.h, C.byref(out)), "measure_rectangles")
        return out.value

    # --- Wilson gradient flow and clover field strength on the resident links (meas/gradient_flow.c; flow.hip) ---
    def measure_field_strength(self):
        """(E, Q) of measure_clover_field_strength_observables on the resident links."""
        e, q = C.c_double(0.0), C.c_double(0.0)
        _ck(self.lib.tmhip_measure_field_strength(self.h, C.byref(e), C.byref(q)), "measure_field_strength")
        return e.value, q.value

    def flow_begin(self):
        """Copy the resident links into the flow buffers (t = 0); the resident links are never modified by the flow."""
        _ck(self.lib.tmhip_flow_begin(self.h), "flow_begin")

    def flow_step(self, eps):
        """One step_gradient_flow."""
        _ck(self.lib.tmhip_flow_step(self.h, eps), "flow_step")

    def flow_observables(self):
        """(P, E, Q) of the flowed links, P = measure_plaquette / (6 VOLUME)."""
        p, e, q = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        _ck(self.lib.tmhip_flow_observables(self.h, C.byref(p), C.byref(e), C.byref(q)), "flow_observables")
        return p.value, e.value, q.value

    def flow_links(self):
        """The flowed links, [V][4][3][3][2]."""
        out = np.zeros((self.V, 4, 3, 3, 2))
        _ck(self.lib.tmhip_flow_download(self.h, _hp(out)), "flow_download")
        return out

    def flow_end(self):
        _ck(self.lib.tmhip_flow_end(self.h), "flow_end")

    def gradient_flow(self, eps, tmax, max_rows=None):
        """The loop of gradient_flow_measurement: an [n][8] array of rows t, P, Eplaq, Esym, tsqEplaq, tsqEsym, Wsym, Qsym."""
        if max_rows is None:
            max_rows = int(tmax / (2.0 * eps)) + 2 if eps > 0.0 else 0
        rows = np.zeros((max(max_rows, 1), 8))
        n = C.c_int(0)
        _ck(self.lib.tmhip_gradient_flow(self.h, eps, tmax, max_rows, rows.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)), "gradient_flow")
        return rows[:n.value].copy()

    # --- the other online measurements (meas/correlators.c, pion_norm.c, polyakov_loop.c, oriented_plaquettes.c; meas.hip) ---
    def slice_correlators(self, even, odd, dir=0, pa_p4=True):
        """Raw per-slice sums of a propagator given as its two one-parity fields: (pp, pa, p4), or pp alone with pa_p4=False.
        dir 0: T time-slices (correlators.c:159-170), dir 3: LZ z-slices (pion_norm.c:98-107)."""
        n = self.LZ if dir == 3 else self.T
        pd = C.POINTER(C.c_double)
        pp = np.zeros(n)
        if not pa_p4:
            _ck(self.lib.tmhip_slice_correlators(self.h, even.h, odd.h, dir, pp.ctypes.data_as(pd), None, None), "slice_correlators")
            return pp
        pa, p4 = np.zeros(n), np.zeros(n)
        _ck(self.lib.tmhip_slice_correlators(self.h, even.h, odd.h, dir, pp.ctypes.data_as(pd), pa.ctypes.data_as(pd), p4.ctypes.data_as(pd)),
            "slice_correlators")
        return pp, pa, p4

    def polyakov_loop(self, dir):
        """The Polyakov loop along dir = 0 .. 3 on the resident links (polyakov_loop.c), a complex number."""
        re, im = C.c_double(0.0), C.c_double(0.0)
        _ck(self.lib.tmhip_polyakov_loop(self.h, dir, C.byref(re), C.byref(im)), "polyakov_loop")
        return complex(re.value, im.value)

    def measure_oriented_plaquettes(self):
        """The six plane averages of measure_oriented_plaquettes, planes (0,1), (0,2), (0,3), (1,2), (1,3), (2,3)."""
        out = np.zeros(6)
        _ck(self.lib.tmhip_measure_oriented_plaquettes(self.h, out.ctypes.data_as(C.POINTER(C.c_double))), "measure_oriented_plaquettes")
        return [float(x) for x in out]

    # ---- ILDG gauge configurations (io/gauge_read.c, io/gauge_write.c; ildg.hip)
    def gauge_unpack_ildg(self, file_bytes, prec):
        """This rank's part of an "ildg-binary-data" record (bytes / uint8 array) -> resident links; returns (suma, sumb)."""
        buf = np.frombuffer(file_bytes, dtype=np.uint8) if not isinstance(file_bytes, np.ndarray) else file_bytes
        want = self.V * 4 * 9 * (16 if prec == 64 else 8)
        if buf.size != want:
            raise TmHipError("gauge_unpack_ildg: %d bytes, expected %d" % (buf.size, want))
        buf = np.ascontiguousarray(buf)
        sums = (C.c_uint * 2)()
        _ck(self.lib.tmhip_gauge_unpack_ildg(self.h, buf.ctypes.data_as(C.c_void_p), prec, sums), "tmhip_gauge_unpack_ildg")
        return int(sums[0]), int(sums[1])

    def gauge_pack_ildg(self, prec, out=None):
        """The resident links as the bytes of this rank's part of the record; returns (uint8 array, (suma, sumb)).  `out`: a buffer
        of the record's size to fill (a fresh numpy array is 600 MB of pages the kernel has never mapped: the copy into it
        runs at the page-fault rate, 52 ms instead of 12 at 32^4)."""
        n = self.V * 4 * 9 * (16 if prec == 64 else 8)
        if out is None:
            out = np.zeros(n, dtype=np.uint8)
        elif out.dtype != np.uint8 or out.size != n or not out.flags["C_CONTIGUOUS"]:
            raise TmHipError("gauge_pack_ildg: out must be a contiguous uint8 array of %d bytes" % n)
        sums = (C.c_uint * 2)()
        _ck(self.lib.tmhip_gauge_pack_ildg(self.h, out.ctypes.data_as(C.c_void_p), prec, sums), "tmhip_gauge_pack_ildg")
        return out, (int(sums[0]), int(sums[1]))

    def read_gauge_field(self, filename, prec=64, io_checks=True, want_host=True):
        """read_gauge_field(filename, gf) (io/gauge_read.c:28): returns (status 0 | -1, host field or None, GaugeInfo)."""
        info = GaugeInfo()
        out = np.zeros((self.VPR, 4, 3, 3, 2)) if want_host else None
        rc = self.lib.tmhip_read_gauge_field(self.h, str(filename).encode(), prec, 1 if io_checks else 0, _hp(out) if want_host else None, C.byref(info))
        if rc not in (0, -1):
            raise TmHipError("tmhip_read_gauge_field failed (rc=%d)" % rc)
        return rc, out, info

    def write_gauge_field(self, filename, prec=64, xlf_info=None):
        """write_gauge_field(filename, prec, xlfInfo) (io/gauge_write.c:22) from the resident links; returns (suma, sumb)."""
        sums = (C.c_uint * 2)()
        _ck(self.lib.tmhip_write_gauge_field(self.h, str(filename).encode(), prec, xlf_info.encode() if xlf_info else None, sums), "tmhip_write_gauge_field")
        return int(sums[0]), int(sums[1])

    # ---- propagators and sources (io/spinor_read.c, io/spinor_write.c, start.c; spinor_io.hip)
    def spinor_pack(self, even, odd, prec, out=None):
        """Two fp64 EO fields (or the two views of a FULL field) as the bytes of this rank's part of a "scidac-binary-data" record;
        returns (uint8 array, (suma, sumb)).  `out`: a contiguous uint8 buffer of the record's size to fill."""
        n = self.V * (192 if prec == 64 else 96)
        if out is None:
            out = np.zeros(n, dtype=np.uint8)
        elif out.dtype != np.uint8 or out.size != n or not out.flags["C_CONTIGUOUS"]:
            raise TmHipError("spinor_pack: out must be a contiguous uint8 array of %d bytes" % n)
        sums = (C.c_uint * 2)()
        _ck(self.lib.tmhip_spinor_pack(self.h, even.h, odd.h, out.ctypes.data_as(C.c_void_p), prec, sums), "tmhip_spinor_pack")
        return out, (int(sums[0]), int(sums[1]))

    def spinor_unpack(self, even, odd, file_bytes, prec):
        """This rank's part of a "scidac-binary-data" record (bytes / uint8 array) -> the two fields; returns (suma, sumb)."""
        buf = np.frombuffer(file_bytes, dtype=np.uint8) if not isinstance(file_bytes, np.ndarray) else file_bytes
        want = self.V * (192 if prec == 64 else 96)
        if buf.size != want:
            raise TmHipError("spinor_unpack: %d bytes, expected %d" % (buf.size, want))
        buf = np.ascontiguousarray(buf)
        sums = (C.c_uint * 2)()
        _ck(self.lib.tmhip_spinor_unpack(self.h, even.h, odd.h, buf.ctypes.data_as(C.c_void_p), prec, sums), "tmhip_spinor_unpack")
        return int(sums[0]), int(sums[1])

    def read_spinor(self, even, odd, filename, position=0, io_checks=True):
        """read_spinor(s, r, filename, position) (io/spinor_read.c:27): returns (status 0 | -1 | -2 | -3 | -5 | -6 | -7, SpinorInfo)."""
        info = SpinorInfo()
        rc = self.lib.tmhip_read_spinor(self.h, even.h, odd.h, str(filename).encode(), position, 1 if io_checks else 0, C.byref(info))
        if rc > 0:
            raise TmHipError("tmhip_read_spinor failed (rc=%d)" % rc)
        return rc, info

    def write_spinor(self, filename, even, odd, prec=64, append=False):
        """write_spinor(writer, s, r, flavours, prec) (io/spinor_write.c:23): `even`, `odd` a field each or equally long lists of
        them (one entry per flavour); returns the list of (suma, sumb), one per flavour."""
        ev = list(even) if isinstance(even, (list, tuple)) else [even]
        od = list(odd) if isinstance(odd, (list, tuple)) else [odd]
        if len(ev) != len(od) or not ev:
            raise TmHipError("write_spinor: as many even as odd fields, at least one")
        n = len(ev)
        sums = (C.c_uint * (2 * n))()
        _ck(self.lib.tmhip_write_spinor(self.h, str(filename).encode(), 1 if append else 0, (C.c_void_p * n)(*[f.h.value for f in ev]),
                                        (C.c_void_p * n)(*[f.h.value for f in od]), n, prec, sums), "tmhip_write_spinor")
        return [(int(sums[2 * k]), int(sums[2 * k + 1])) for k in range(n)]

    def bench_spinor_io(self, even, odd, prec, pack, reps):
        """Milliseconds of `reps` launches of the pack / unpack kernel alone (HIP events)."""
        ms = C.c_double()
        _ck(self.lib.tmhip_bench_spinor_io(self.h, even.h, odd.h, prec, 1 if pack else 0, reps, C.byref(ms)), "tmhip_bench_spinor_io")
        return ms.value

    def source_point(self, even, odd, is_, ic, global_site=0):
        """source_spinor_field (start.c:707, site 0) / source_spinor_field_point_from_file (start.c:743) on the device."""
        _ck(self.lib.tmhip_source_point(self.h, even.h, odd.h, is_, ic, global_site), "tmhip_source_point")

    def sw_invert(self, ieo, mu):
        """operator/clover_invert.c:170 on the device (needs sw_term or set_clover first)."""
        _ck(self.lib.tmhip_sw_invert(self.h, ieo, mu), "tmhip_sw_invert")

    def get_clover(self, want_sw=True, want_sw_inv=True):
        """Device-resident clover blocks in the reference's host layouts: (sw [V][3][2][3][3][2], sw_inv [V][4][2][3][3][2])."""
        sw = np.zeros((self.V, 3, 2, 3, 3, 2)) if want_sw else None
        swi = np.zeros((self.V, 4, 2, 3, 3, 2)) if want_sw_inv else None
        _ck(self.lib.tmhip_get_clover(self.h, _hp(sw) if want_sw else None, _hp(swi) if want_sw_inv else None), "tmhip_get_clover")
        return sw, swi

    def assign_mul_one_sw_pm_imu(self, ieo, k, l, mu):
        _ck(self.lib.tmhip_assign_mul_one_sw_pm_imu(self.h, ieo, k.h, l.h, mu), "assign_mul_one_sw_pm_imu")

    def assign_mul_one_sw_pm_imu_inv(self, ieo, k, l, mu):
        _ck(self.lib.tmhip_assign_mul_one_sw_pm_imu_inv(self.h, ieo, k.h, l.h, mu), "assign_mul_one_sw_pm_imu_inv")

    def Msw_full(self, en, on, e, o):
        _ck(self.lib.tmhip_Msw_full(self.h, en.h, on.h, e.h, o.h), "Msw_full")

    def clover_inv(self, l, tau3sign, mu):
        _ck(self.lib.tmhip_clover_inv(self.h, l.h, tau3sign, mu), "clover_inv")

    def clover_gamma5(self, ieo, l, k, j, mu):
        _ck(self.lib.tmhip_clover_gamma5(self.h, ieo, l.h, k.h, j.h, mu), "clover_gamma5")

    def clover(self, ieo, l, k, j, mu):
        _ck(self.lib.tmhip_clover(self.h, ieo, l.h, k.h, j.h, mu), "clover")

    def H_eo_sw_inv_psi(self, l, k, ieo, tau3sign, mu):
        _ck(self.lib.tmhip_H_eo_sw_inv_psi(self.h, l.h, k.h, ieo, tau3sign, mu), "H_eo_sw_inv_psi")

    def Qsw_pm_psi_32(self, l, k):
        _ck(self.lib.tmhip_Qsw_pm_psi_32(self.h, l.h, k.h), "Qsw_pm_psi_32")

    # --- mixed precision (reference names with the _32 suffix) -------------
    def assign_to_32(self, r32, s64, N):
        _ck(self.lib.tmhip_assign_to_32(self.h, r32.h, s64.h, N), "assign_to_32")

    def assign_to_64(self, r64, s32, N):
        _ck(self.lib.tmhip_assign_to_64(self.h, r64.h, s32.h, N), "assign_to_64")

    def Hopping_Matrix_32(self, ieo, l, k):
        _ck(self.lib.tmhip_hopping_matrix_32(self.h, ieo, l.h, k.h), "Hopping_Matrix_32")

    def Qtm_pm_psi_32(self, l, k):
        _ck(self.lib.tmhip_Qtm_pm_psi_32(self.h, l.h, k.h), "Qtm_pm_psi_32")

    def square_norm_32(self, P, N, parallel=0):
        out = C.c_double()
        _ck(self.lib.tmhip_square_norm_32(self.h, P.h, N, parallel, C.byref(out)), "square_norm_32")
        return out.value

    def scalar_prod_r_32(self, S, R, N, parallel=0):
        out = C.c_double()
        _ck(self.lib.tmhip_scalar_prod_r_32(self.h, S.h, R.h, N, parallel, C.byref(out)), "scalar_prod_r_32")
        return out.value

    def assign_add_mul_r_32(self, P, Q, c, N):
        _ck(self.lib.tmhip_assign_add_mul_r_32(self.h, P.h, Q.h, c, N), "assign_add_mul_r_32")

    def assign_mul_add_r_32(self, R, c, S, N):
        _ck(self.lib.tmhip_assign_mul_add_r_32(self.h, R.h, c, S.h, N), "assign_mul_add_r_32")

    def mixed_cg_her(self, P, Q, max_iter, eps_sq, rel_prec, N, innereps=5.0e-5, max_inner_it=5000, op="Qtm_pm_psi"):
        """solver/mixed_cg_her.c with (f, f32) = (Qtm_pm_psi, Qtm_pm_psi_32) or (Qsw_pm_psi, Qsw_pm_psi_32);
        returns (iterations, outer iterations)."""
        it, outer = C.c_int(), C.c_int()
        _ck(self.lib.tmhip_mixed_cg_her(self.h, P.h, Q.h, max_iter, eps_sq, rel_prec, N, OPS[op], innereps,
                                        max_inner_it, C.byref(it), C.byref(outer)), "mixed_cg_her")
        return it.value, outer.value

    def mixed_cg_restarts(self):
        """Inner iteration count (the reference's j, mixed_cg_her.c:152) of every outer iteration of the last mixed_cg_her."""
        buf, n = (C.c_int * 256)(), C.c_int()
        _ck(self.lib.tmhip_mixed_cg_restarts(self.h, buf, 256, C.byref(n)), "tmhip_mixed_cg_restarts")
        return list(buf[:min(n.value, 256)])

    def rg_mixed_cg_her(self, P, Q, max_iter, eps_sq, rel_prec, N, delta=5.0e-5, op="Qtm_pm_psi"):
        """solver/rg_mixed_cg_her.c:180 (reliable updates, fp64 fail-safe); delta = solver_params.mcg_delta.
        Returns (iterations as the reference counts them, (iter_out, iter_in_sp, iter_in_dp))."""
        it, a, b, c = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _ck(self.lib.tmhip_rg_mixed_cg_her(self.h, P.h, Q.h, max_iter, eps_sq, rel_prec, N, OPS[op], delta, C.byref(it),
                                           C.byref(a), C.byref(b), C.byref(c)), "rg_mixed_cg_her")
        return it.value, (a.value, b.value, c.value)

    # --- stencil ----------------------------------------------------------
    def Hopping_Matrix(self, ieo, l, k):
        _ck(self.lib.tmhip_hopping_matrix(self.h, ieo, l.h, k.h), "Hopping_Matrix")

    def Hopping_Matrix_nocom(self, ieo, l, k):
        _ck(self.lib.tmhip_hopping_matrix_nocom(self.h, ieo, l.h, k.h), "Hopping_Matrix_nocom")

    def tm_times_Hopping_Matrix(self, ieo, l, k, c):
        _ck(self.lib.tmhip_tm_times_hopping_matrix(self.h, ieo, l.h, k.h, c.real, c.imag), "tm_times_Hopping_Matrix")

    def tm_sub_Hopping_Matrix(self, ieo, l, p, k, c):
        _ck(self.lib.tmhip_tm_sub_hopping_matrix(self.h, ieo, l.h, p.h, k.h, c.real, c.imag), "tm_sub_Hopping_Matrix")

    def D_psi(self, P, Q):
        _ck(self.lib.tmhip_D_psi(self.h, P.h, Q.h), "D_psi")

    # --- site-diagonal ----------------------------------------------------
    def mul_one_pm_imu_inv(self, l, sign, N):
        _ck(self.lib.tmhip_mul_one_pm_imu_inv(self.h, l.h, sign, N), "mul_one_pm_imu_inv")

    def assign_mul_one_pm_imu_inv(self, l, k, sign, N):
        _ck(self.lib.tmhip_assign_mul_one_pm_imu_inv(self.h, l.h, k.h, sign, N), "assign_mul_one_pm_imu_inv")

    def assign_mul_one_pm_imu(self, l, k, sign, N):
        _ck(self.lib.tmhip_assign_mul_one_pm_imu(self.h, l.h, k.h, sign, N), "assign_mul_one_pm_imu")

    def mul_one_pm_imu(self, l, sign):
        _ck(self.lib.tmhip_mul_one_pm_imu(self.h, l.h, sign), "mul_one_pm_imu")

    def mul_one_pm_imu_sub_mul(self, l, k, j, sign, N):
        _ck(self.lib.tmhip_mul_one_pm_imu_sub_mul(self.h, l.h, k.h, j.h, sign, N), "mul_one_pm_imu_sub_mul")

    def mul_one_pm_imu_sub_mul_gamma5(self, l, k, j, sign):
        _ck(self.lib.tmhip_mul_one_pm_imu_sub_mul_gamma5(self.h, l.h, k.h, j.h, sign), "mul_one_pm_imu_sub_mul_gamma5")

    def mul_one_sub_mul_gamma5(self, l, k, j):
        _ck(self.lib.tmhip_mul_one_sub_mul_gamma5(self.h, l.h, k.h, j.h), "mul_one_sub_mul_gamma5")

    def gamma5(self, l, k, N):
        _ck(self.lib.tmhip_gamma5(self.h, l.h, k.h, N), "gamma5")

    # --- compositions -----------------------------------------------------
    def H_eo_tm_inv_psi(self, l, k, ieo, sign):
        _ck(self.lib.tmhip_H_eo_tm_inv_psi(self.h, l.h, k.h, ieo, sign), "H_eo_tm_inv_psi")

    def op(self, name, l, k):
        _ck(getattr(self.lib, "tmhip_" + name)(self.h, l.h, k.h), name)

    def Qtm_pm_psi(self, l, k):
        self.op("Qtm_pm_psi", l, k)

    def M_full(self, en, on, e, o):
        _ck(self.lib.tmhip_M_full(self.h, en.h, on.h, e.h, o.h), "M_full")

    # --- linalg -----------------------------------------------------------
    def square_norm(self, P, N, parallel=0):
        out = C.c_double()
        _ck(self.lib.tmhip_square_norm(self.h, P.h, N, parallel, C.byref(out)), "square_norm")
        return out.value

    def scalar_prod_r(self, S, R, N, parallel=0):
        out = C.c_double()
        _ck(self.lib.tmhip_scalar_prod_r(self.h, S.h, R.h, N, parallel, C.byref(out)), "scalar_prod_r")
        return out.value

    def assign_add_mul_r(self, P, Q, c, N):
        _ck(self.lib.tmhip_assign_add_mul_r(self.h, P.h, Q.h, c, N), "assign_add_mul_r")

    def assign_add_mul(self, P, Q, c, N):
        """linalg/assign_add_mul.c: P += c Q with complex c"""
        c = complex(c)
        _ck(self.lib.tmhip_assign_add_mul(self.h, P.h, Q.h, c.real, c.imag, N), "assign_add_mul")

    def assign_mul_add_r(self, R, c, S, N):
        _ck(self.lib.tmhip_assign_mul_add_r(self.h, R.h, c, S.h, N), "assign_mul_add_r")

    def assign_mul_add_r_and_square(self, R, c, S, N, parallel=0):
        out = C.c_double()
        _ck(self.lib.tmhip_assign_mul_add_r_and_square(self.h, R.h, c, S.h, N, parallel, C.byref(out)),
            "assign_mul_add_r_and_square")
        return out.value

    def diff(self, Q, R, S, N):
        _ck(self.lib.tmhip_diff(self.h, Q.h, R.h, S.h, N), "diff")

    def add(self, Q, R, S, N):
        _ck(self.lib.tmhip_add(self.h, Q.h, R.h, S.h, N), "add")

    def mul_r(self, R, c, S, N):
        _ck(self.lib.tmhip_mul_r(self.h, R.h, c, S.h, N), "mul_r")

    def assign(self, R, S, N):
        _ck(self.lib.tmhip_assign(self.h, R.h, S.h, N), "assign")

    # --- complex linalg and its batched forms (linalg/scalar_prod.c, assign_diff_mul.c, mul.c) ---
    @staticmethod
    def _handles(fs):
        return (C.c_void_p * max(len(fs), 1))(*[f.h for f in fs])

    @staticmethod
    def _pairs(cs):
        a = np.ascontiguousarray(np.asarray(cs, dtype=np.complex128).reshape(-1))
        return a, a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))

    def scalar_prod(self, S, R, N, parallel=0):
        """sum conj(S) R"""
        out = (C.c_double * 2)()
        _ck(self.lib.tmhip_scalar_prod(self.h, S.h, R.h, N, parallel, out), "scalar_prod")
        return complex(out[0], out[1])

    def assign_diff_mul(self, R, S, c, N):
        """R -= c S"""
        c = complex(c)
        _ck(self.lib.tmhip_assign_diff_mul(self.h, R.h, S.h, c.real, c.imag, N), "assign_diff_mul")

    def mul(self, R, c, S, N):
        """R = c S (R may be S)"""
        c = complex(c)
        _ck(self.lib.tmhip_mul(self.h, R.h, c.real, c.imag, S.h, N), "mul")

    def multi_scalar_prod(self, Ss, R, N):
        """[<S_i, R>] as a complex128 array, one pass over R per group of fields and one host synchronisation"""
        n = len(Ss)
        out = np.zeros(max(n, 1), dtype=np.complex128)
        _ck(self.lib.tmhip_multi_scalar_prod(self.h, n, self._handles(Ss), R.h, N, out.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))),
            "multi_scalar_prod")
        return out[:n]

    def multi_assign_diff_mul(self, Rs, S, cs, N):
        """R_i -= c_i S for all i"""
        if len(cs) != len(Rs):
            raise TmHipError("multi_assign_diff_mul: one coefficient per field")
        keep, pc = self._pairs(cs)
        _ck(self.lib.tmhip_multi_assign_diff_mul(self.h, len(Rs), self._handles(Rs), S.h, pc, N), "multi_assign_diff_mul")

    def lincomb(self, P, Vs, cs, N):
        """P = sum_i c_i V_i, added from the last field down to the first"""
        if len(cs) != len(Vs):
            raise TmHipError("lincomb: one coefficient per field")
        keep, pc = self._pairs(cs)
        _ck(self.lib.tmhip_lincomb(self.h, P.h, len(Vs), self._handles(Vs), pc, N), "lincomb")

    # --- chronological solver guess (solver/chrono_guess.c) -----------------
    def chrono_guess(self, trial, phi, vs, op="Qtm_pm_psi", N=None):
        """trial = the guess for op x = phi from the stored solutions vs (oldest first; all but the last are orthogonalised against
        the last in place).  Returns (G, bn): the projected operator [n][n] and the projected right-hand side [n], complex128."""
        n = len(vs)
        N = self.Vh if N is None else N
        G = np.zeros((n, n), dtype=np.complex128)
        bn = np.zeros(max(n, 1), dtype=np.complex128)
        pd = C.POINTER(C.c_double)
        _ck(self.lib.tmhip_chrono_guess(self.h, trial.h, phi.h, self._handles(vs), n, OPS[op], N,
                                        G.view(np.float64).ctypes.data_as(pd) if n else None, bn.view(np.float64).ctypes.data_as(pd)), "chrono_guess")
        return G, bn[:n]

    def chrono_add_solution(self, slot, trial, N=None):
        """slot = trial / |trial|"""
        _ck(self.lib.tmhip_chrono_add_solution(self.h, slot.h, trial.h, self.Vh if N is None else N), "chrono_add_solution")

    # --- solver -----------------------------------------------------------
    def cg_her(self, P, Q, max_iter, eps_sq, rel_prec, N, op="Qtm_pm_psi"):
        it = C.c_int()
        hist = np.zeros(max(max_iter, 1), dtype=np.float64)
        _ck(self.lib.tmhip_cg_her(self.h, P.h, Q.h, max_iter, eps_sq, rel_prec, N, OPS[op], C.byref(it),
                                  hist.ctypes.data_as(C.POINTER(C.c_double)), hist.size), "cg_her")
        n = it.value if it.value > 0 else max_iter
        return it.value, hist[:n]

    # --- BiCGstab (solver/bicgstab_complex.c) -------------------------------
    @staticmethod
    def _c2(z):
        z = complex(z)
        return (C.c_double * 2)(z.real, z.imag)

    def assign_add_mul_add_mul(self, R, S, U, c1, c2, N):
        """R += c1 S + c2 U (EO fields, or FULL fields with N = VOLUME)"""
        c1, c2 = complex(c1), complex(c2)
        _ck(self.lib.tmhip_assign_add_mul_add_mul(self.h, R.h, S.h, U.h, c1.real, c1.imag, c2.real, c2.imag, N), "assign_add_mul_add_mul")

    def assign_mul_bra_add_mul_ket_add(self, R, S, U, c1, c2, N):
        """R = c2 (R + c1 S) + U"""
        c1, c2 = complex(c1), complex(c2)
        _ck(self.lib.tmhip_assign_mul_bra_add_mul_ket_add(self.h, R.h, S.h, U.h, c1.real, c1.imag, c2.real, c2.imag, N),
            "assign_mul_bra_add_mul_ket_add")

    def bicg_update(self, P, r, p, s, t, hatr, alpha, omega, N):
        """K4 of the fused iteration: P += alpha p + omega s; r = s - omega t.  Returns (<hatr, r>, <r, r>)."""
        out = (C.c_double * 3)()
        _ck(self.lib.tmhip_bicg_update(self.h, P.h, r.h, p.h, s.h, t.h, hatr.h, self._c2(alpha), self._c2(omega), N, out), "bicg_update")
        return complex(out[0], out[1]), out[2]

    def bicg_pair_dot(self, t, s, N):
        """K3: (<t, s>, <t, t>) from one pass over t"""
        out = (C.c_double * 3)()
        _ck(self.lib.tmhip_bicg_pair_dot(self.h, t.h, s.h, N, out), "bicg_pair_dot")
        return complex(out[0], out[1]), out[2]

    def bicg_sub(self, s, r, v, alpha, N):
        """K2: s = r - alpha v"""
        _ck(self.lib.tmhip_bicg_sub(self.h, s.h, r.h, v.h, self._c2(alpha), N), "bicg_sub")

    def bicg_dir(self, p, v, r, omega, beta, N):
        """K5: p = beta (p - omega v) + r"""
        _ck(self.lib.tmhip_bicg_dir(self.h, p.h, v.h, r.h, self._c2(omega), self._c2(beta), N), "bicg_dir")

    def bicgstab_complex(self, P, Q, max_iter, eps_sq, rel_prec, N, op="Mtm_plus_sym_psi"):
        """Returns (the reference's return value, |r|^2 at the top of every iteration run, the starting residual first)."""
        it = C.c_int(-2)
        hist = np.zeros(max(max_iter, 0) + 1, dtype=np.float64)
        _ck(self.lib.tmhip_bicgstab_complex(self.h, P.h, Q.h, max_iter, eps_sq, rel_prec, N, BICG_OPS[op], C.byref(it),
                                            hist.ctypes.data_as(C.POINTER(C.c_double)), hist.size), "bicgstab_complex")
        n = it.value + 1 if it.value > 0 else hist.size
        return it.value, hist[:n]

    # --- eigenvalue measurement (solver/eigenvalues.c, eigenvalues_bi.c; eig.hip) ---
    @staticmethod
    def _flavours(vs):
        """a list of fields or of (up, dn) pairs -> (up handles, dn handles or None)"""
        if len(vs) and isinstance(vs[0], (tuple, list)):
            return Lattice._handles([v[0] for v in vs]), Lattice._handles([v[1] for v in vs])
        return Lattice._handles(vs), None

    def eig_dots(self, vs, w, N=None):
        """[<v_i, w>] as a complex128 array from one launch; vs: fields, or (up, dn) pairs with w = (w_up, w_dn)"""
        up, dn = self._flavours(vs)
        wu, wd = (w[0].h, w[1].h) if dn is not None else (w.h, None)
        out = np.zeros(len(vs), dtype=np.complex128)
        _ck(self.lib.tmhip_eig_dots(self.h, len(vs), up, dn, wu, wd, self.Vh if N is None else N,
                                    out.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))), "eig_dots")
        return out

    def eig_project(self, vs, w, h, N=None):
        """w -= sum_i h_i v_i, ascending i; returns |w|^2 of the result"""
        up, dn = self._flavours(vs)
        wu, wd = (w[0].h, w[1].h) if dn is not None else (w.h, None)
        if len(h) != len(vs):
            raise TmHipError("eig_project: one coefficient per vector")
        keep, pc = self._pairs(h)
        out = C.c_double()
        _ck(self.lib.tmhip_eig_project(self.h, len(vs), up, dn, wu, wd, pc, self.Vh if N is None else N, C.byref(out)), "eig_project")
        return out.value

    def basis_rotate(self, vs, Y, N=None):
        """V[:, 0:k] = V[:, 0:n] Y in place; Y real [n][k]"""
        up, dn = self._flavours(vs)
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[0] != len(vs):
            raise TmHipError("basis_rotate: Y must be [n = %d][k]" % len(vs))
        _ck(self.lib.tmhip_basis_rotate(self.h, Y.shape[0], Y.shape[1], up, dn, Y.ctypes.data_as(C.POINTER(C.c_double)),
                                        self.Vh if N is None else N), "basis_rotate")

    def eig_set_interval(self, lo=0.0, hi=0.0):
        """the interval of the Chebyshev filter ("eig_cheb"); 0, 0 = from one unfiltered cycle"""
        _ck(self.lib.tmhip_eig_set_interval(self.h, lo, hi), "eig_set_interval")

    def _eig(self, nd, op, N, nev, which, prec, max_apps, vectors, start, cheb):
        w = {"lowest": 0, "highest": 1}.get(which, which)
        kind = FIELD_FULL if (not nd and op == "Q_pm_psi") else FIELD_EO
        fields = None
        old_cheb = None
        if cheb is not None:                 # for this call only: the context's option is back when it returns
            old_cheb = self.get_option("eig_cheb")
            self.set_option("eig_cheb", cheb)
        try:
            return self._eig_call(nd, op, N, nev, w, kind, prec, max_apps, vectors, start)
        finally:
            if old_cheb is not None:
                self.set_option("eig_cheb", old_cheb)

    def _eig_call(self, nd, op, N, nev, w, kind, prec, max_apps, vectors, start):
        fields = None
        if vectors or start is not None:
            fields = [((self.field(), self.field()) if nd else self.field(kind=kind)) for _ in range(nev)]
            for f in fields:
                for g in (f if nd else (f,)):
                    g.zero()
            if start is not None:
                for g, s in zip(fields[0] if nd else (fields[0],), start if nd else (start,)):
                    g.upload(s)
        up, dn = self._flavours(fields) if fields else (None, None)
        ev, rs = np.zeros(nev), np.zeros(nev)
        conv, apps = C.c_int(), C.c_int()
        pd = C.POINTER(C.c_double)
        if nd:
            rc = self.lib.tmhip_eigenvalues_nd(self.h, ND_OPS[op], nev, w, prec, max_apps, up, dn, ev.ctypes.data_as(pd), rs.ctypes.data_as(pd),
                                               C.byref(conv), C.byref(apps))
        else:
            rc = self.lib.tmhip_eigenvalues(self.h, ALL_OPS[op], (self.V if kind == FIELD_FULL else self.Vh) if N is None else N, nev, w, prec,
                                            max_apps, up, ev.ctypes.data_as(pd), rs.ctypes.data_as(pd), C.byref(conv), C.byref(apps))
        if rc != 0 and fields:
            for f in fields:
                for g in (f if nd else (f,)):
                    g.free()
        _ck(rc, "eigenvalues_nd" if nd else "eigenvalues")
        out = {"evals": ev, "resid": rs, "converged": conv.value, "apps": apps.value}
        if vectors:
            out["vectors"] = fields
        elif fields:
            for f in fields:
                for g in (f if nd else (f,)):
                    g.free()
        return out

    def eigenvalues(self, nev, which="lowest", prec=1e-7, max_apps=5000, op="Qtm_pm_psi", N=None, vectors=False, start=None, cheb=None):
        """The nev lowest / highest eigenpairs of a Hermitian positive single-flavour operator (Qtm_pm_psi, Qsw_pm_psi, Q_pm_psi on FULL
        fields) -> {"evals", "resid", "converged", "apps"[, "vectors": nev device fields, the caller's to free]}.  start: a host
        spinor array as the start vector; cheb: the degree of the filter of the lowest end for THIS call (the option "eig_cheb" otherwise)."""
        return self._eig(False, op, N, nev, which, prec, max_apps, vectors, start, cheb)

    def eigenvalues_nd(self, nev, which="lowest", prec=1e-7, max_apps=5000, op="Qtm_pm_ndpsi", vectors=False, start=None, cheb=None):
        """The same for the doublet operators; vectors and start are (up, dn) pairs."""
        return self._eig(True, op, None, nev, which, prec, max_apps, vectors, start, cheb)

    # --- LapH eigensystem: the 3D Laplacian of jacobi.c on all time-slices (LapH_ev.c, solver/eigenvalues_Jacobi.c; laph.hip) ---
    def cvfield(self, host=None):
        f = CvField(self)
        if host is not None:
            f.upload(host)
        return f

    def _slices(self, t0, nt):
        return t0, (self.T - t0 if nt is None else nt)

    @staticmethod
    def _flags(active, nt):
        """None, or nt flags -> (keep-alive, pointer)"""
        if active is None:
            return None, None
        a = np.ascontiguousarray(active, dtype=np.int32)
        if a.shape != (nt,):
            raise TmHipError("active: one flag per time-slice of the range")
        return a, a.ctypes.data_as(C.POINTER(C.c_int))

    def laph_apply(self, out, inp, t0=0, nt=None, dot=False, coef=None, prev=None):
        """out[t] = Jacobi(in[t], t) for t0 <= t < t0 + nt in one launch.  dot: returns the complex <in, out> of every slice from the
        same pass.  coef [nt][3]: out = c1 (A in) + c2 in + c3 prev instead, the Chebyshev step (prev None: c3 is not read)."""
        t0, nt = self._slices(t0, nt)
        pd = C.POINTER(C.c_double)
        if coef is not None:
            cf = np.ascontiguousarray(coef, dtype=np.float64)
            if cf.shape != (nt, 3):
                raise TmHipError("laph_apply: coef must be [nt = %d][3]" % nt)
            _ck(self.lib.tmhip_laph_apply_filter(self.h, out.h, inp.h, prev.h if prev is not None else None, t0, nt, cf.ctypes.data_as(pd)), "laph_apply_filter")
            return None
        if dot:
            d = np.zeros(nt, dtype=np.complex128)
            _ck(self.lib.tmhip_laph_apply_dot(self.h, out.h, inp.h, t0, nt, d.view(np.float64).ctypes.data_as(pd)), "laph_apply_dot")
            return d
        _ck(self.lib.tmhip_laph_apply(self.h, out.h, inp.h, t0, nt), "laph_apply")
        return None

    def laph_dots(self, vs, w, t0=0, nt=None, active=None, out=None):
        """<v_i, w> per slice as a complex128 [nt][nv] array (`out`: filled in place; the rows of frozen slices are left alone)"""
        t0, nt = self._slices(t0, nt)
        keep, pa = self._flags(active, nt)
        if out is None:
            out = np.zeros((nt, len(vs)), dtype=np.complex128)
        if out.shape != (nt, len(vs)) or out.dtype != np.complex128 or not out.flags.c_contiguous:
            raise TmHipError("laph_dots: out must be a C-contiguous complex128 [nt][nv] array")
        _ck(self.lib.tmhip_laph_dots(self.h, len(vs), self._handles(vs), w.h, t0, nt, pa, out.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))), "laph_dots")
        return out

    def laph_project(self, vs, w, h, t0=0, nt=None, active=None, out=None):
        """w[t] -= sum_i h[t][i] v_i[t], ascending i; returns |w[t]|^2 of the result, float64 [nt]"""
        t0, nt = self._slices(t0, nt)
        keep, pa = self._flags(active, nt)
        hc = np.ascontiguousarray(h, dtype=np.complex128)
        if hc.shape != (nt, len(vs)):
            raise TmHipError("laph_project: h must be [nt][nv]")
        if out is None:
            out = np.zeros(nt)
        pd = C.POINTER(C.c_double)
        _ck(self.lib.tmhip_laph_project(self.h, len(vs), self._handles(vs) if len(vs) else None, w.h, hc.view(np.float64).ctypes.data_as(pd), t0, nt, pa,
                                        out.ctypes.data_as(pd)), "laph_project")
        return out

    def laph_normalise(self, out, inp, t0=0, nt=None, active=None, sqnorm=None):
        """out[t] = in[t] / |in[t]|; returns |in[t]|^2, float64 [nt]"""
        t0, nt = self._slices(t0, nt)
        keep, pa = self._flags(active, nt)
        if sqnorm is None:
            sqnorm = np.zeros(nt)
        _ck(self.lib.tmhip_laph_normalise(self.h, out.h, inp.h, t0, nt, pa, sqnorm.ctypes.data_as(C.POINTER(C.c_double))), "laph_normalise")
        return sqnorm

    def laph_rotate(self, vs, Y, t0=0, nt=None, active=None):
        """V[t][:, 0:k] = V[t][:, 0:n] Y[t] in place; Y real [nt][n][k]"""
        t0, nt = self._slices(t0, nt)
        keep, pa = self._flags(active, nt)
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 3 or Y.shape[0] != nt or Y.shape[1] != len(vs):
            raise TmHipError("laph_rotate: Y must be [nt = %d][n = %d][k]" % (nt, len(vs)))
        _ck(self.lib.tmhip_laph_rotate(self.h, Y.shape[1], Y.shape[2], self._handles(vs), Y.ctypes.data_as(C.POINTER(C.c_double)), t0, nt, pa), "laph_rotate")

    def laph_set_interval(self, lo=0.0, hi=0.0):
        """the interval of the Chebyshev filter ("laph_cheb") of every slice; 0, 0 = per slice from one unfiltered cycle"""
        _ck(self.lib.tmhip_laph_set_interval(self.h, lo, hi), "laph_set_interval")

    def laph_timing(self):
        """(host seconds in the small eigenproblems, host seconds in all) of the last laph_eigensystem"""
        out = (C.c_double * 2)()
        _ck(self.lib.tmhip_laph_timing(self.h, out), "laph_timing")
        return out[0], out[1]

    def laph_eigensystem(self, nev, prec=1e-8, max_apps=5000, t0=0, nt=None, vectors=False, start=None):
        """The nev lowest eigenpairs of the 3D Laplacian on every slice of the range -> {"evals" [nt][nev], "resid" [nt][nev],
        "converged" [nt], "apps" [nt][, "vectors": nev colour-vector fields, the caller's to free]}.  start: a host colour-vector
        array, the start vector of every slice where its norm is non-zero."""
        t0, nt = self._slices(t0, nt)
        fields = None
        if vectors or start is not None:
            fields = [self.cvfield() for _ in range(nev)]
            if start is not None:
                fields[0].upload(start)
        ev, rs = np.zeros((nt, nev)), np.zeros((nt, nev))
        conv, apps = np.zeros(nt, dtype=np.int32), np.zeros(nt, dtype=np.int32)
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int)
        rc = self.lib.tmhip_laph_eigensystem(self.h, t0, nt, nev, prec, max_apps, self._handles(fields) if fields else None, ev.ctypes.data_as(pd),
                                             rs.ctypes.data_as(pd), conv.ctypes.data_as(pi), apps.ctypes.data_as(pi))
        if fields and (rc != 0 or not vectors):
            for f in fields:
                f.free()
        _ck(rc, "laph_eigensystem")
        out = {"evals": ev, "resid": rs, "converged": conv, "apps": apps}
        if vectors:
            out["vectors"] = fields
        return out

    def laph_write(self, directory, nstore, vectors, evals, t0=0, nt=None):
        """eigenvalues.TTT.NNNN and eigenvector.EEE.TTT.NNNN of eigenvalues_Jacobi.c:176-209 into `directory`"""
        t0, nt = self._slices(t0, nt)
        ev = np.ascontiguousarray(evals, dtype=np.float64)
        if ev.shape != (nt, len(vectors)):
            raise TmHipError("laph_write: evals must be [nt][nev]")
        _ck(self.lib.tmhip_laph_write(self.h, str(directory).encode(), nstore, t0, nt, len(vectors), self._handles(vectors),
                                      ev.ctypes.data_as(C.POINTER(C.c_double))), "laph_write")

    # --- non-degenerate doublet (operator/tm_operators_nd.c; strange = up = first field of a pair) ---
    def set_nd(self, mubar, epsbar, invmaxev=1.0):
        """g_mubar, g_epsbar (global.h:202) and phmc_invmaxev (phmc.h:31)."""
        _ck(self.lib.tmhip_set_nd(self.h, mubar, epsbar, invmaxev), "tmhip_set_nd")

    def M_ee_inv_ndpsi(self, l_s, l_c, k_s, k_c, mu, eps):
        _ck(self.lib.tmhip_M_ee_inv_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h, mu, eps), "M_ee_inv_ndpsi")

    def M_oo_sub_g5_ndpsi(self, l_s, l_c, k_s, k_c, j_s, j_c, mu, eps):
        _ck(self.lib.tmhip_M_oo_sub_g5_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h, j_s.h, j_c.h, mu, eps), "M_oo_sub_g5_ndpsi")

    def Qtm_ndpsi(self, l_s, l_c, k_s, k_c):
        _ck(self.lib.tmhip_Qtm_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "Qtm_ndpsi")

    def Qtm_dagger_ndpsi(self, l_s, l_c, k_s, k_c):
        _ck(self.lib.tmhip_Qtm_dagger_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "Qtm_dagger_ndpsi")

    def Qtm_pm_ndpsi(self, l_s, l_c, k_s, k_c):
        _ck(self.lib.tmhip_Qtm_pm_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "Qtm_pm_ndpsi")

    def H_eo_tm_ndpsi(self, l_s, l_c, k_s, k_c, ieo):
        _ck(self.lib.tmhip_H_eo_tm_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h, ieo), "H_eo_tm_ndpsi")

    def Q_tau1_sub_const_ndpsi(self, l_s, l_c, k_s, k_c, z, Cpol, invev):
        """tm_operators_nd.c:311-380: l = Cpol invev Qhat tau^1 k - Cpol z k (complex z)"""
        z = complex(z)
        _ck(self.lib.tmhip_Q_tau1_sub_const_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h, z.real, z.imag, Cpol, invev), "Q_tau1_sub_const_ndpsi")

    def cg_her_nd(self, P_up, P_dn, Q_up, Q_dn, max_iter, eps_sq, rel_prec, N, op=None):
        """solver/cg_her_nd.c with f = Qtm_pm_ndpsi (op None: the un-suffixed call; "Qtm_pm_ndpsi" / "Qsw_pm_ndpsi": tmhip_cg_her_nd_op);
        returns the reference's return value (iterations or -1)."""
        it = C.c_int()
        if op is None:
            _ck(self.lib.tmhip_cg_her_nd(self.h, P_up.h, P_dn.h, Q_up.h, Q_dn.h, max_iter, eps_sq, rel_prec, N, C.byref(it)), "cg_her_nd")
        else:
            _ck(self.lib.tmhip_cg_her_nd_op(self.h, P_up.h, P_dn.h, Q_up.h, Q_dn.h, max_iter, eps_sq, rel_prec, N, ND_OPS[op], C.byref(it)), "cg_her_nd_op")
        return it.value

    # --- fp32 doublet and the mixed-precision doublet solve (operator/tm_operators_nd_32.c, solver/rg_mixed_cg_her_nd.c) ---
    def M_ee_inv_ndpsi_32(self, l_s, l_c, k_s, k_c, mu, eps):
        _ck(self.lib.tmhip_M_ee_inv_ndpsi_32(self.h, l_s.h, l_c.h, k_s.h, k_c.h, mu, eps), "M_ee_inv_ndpsi_32")

    def M_oo_sub_g5_ndpsi_32(self, l_s, l_c, k_s, k_c, j_s, j_c, mu, eps):
        _ck(self.lib.tmhip_M_oo_sub_g5_ndpsi_32(self.h, l_s.h, l_c.h, k_s.h, k_c.h, j_s.h, j_c.h, mu, eps), "M_oo_sub_g5_ndpsi_32")

    def Qtm_pm_ndpsi_32(self, l_s, l_c, k_s, k_c):
        """tm_operators_nd_32.c:215-263 on fp32 fields (field32), with mubar, epsbar, invmaxev of set_nd; l may be k."""
        _ck(self.lib.tmhip_Qtm_pm_ndpsi_32(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "Qtm_pm_ndpsi_32")

    def rg_mixed_cg_her_nd(self, P_up, P_dn, Q_up, Q_dn, max_iter, eps_sq, rel_prec, N, delta=5.0e-5, op="Qtm_pm_ndpsi"):
        """solver/rg_mixed_cg_her_nd.c:189 with f = Qtm_pm_ndpsi, f32 = Qtm_pm_ndpsi_32; delta = solver_params.mcg_delta.
        Returns (iterations as the reference counts them or -1, (iter_out, iter_in_sp, iter_in_dp))."""
        it, a, b, c = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _ck(self.lib.tmhip_rg_mixed_cg_her_nd(self.h, P_up.h, P_dn.h, Q_up.h, Q_dn.h, max_iter, eps_sq, rel_prec, N, ND_OPS[op], delta,
                                              C.byref(it), C.byref(a), C.byref(b), C.byref(c)), "rg_mixed_cg_her_nd")
        return it.value, (a.value, b.value, c.value)

    def cg_mms_tm_nd(self, Q_up, Q_dn, shifts, max_iter, eps_sq, rel_prec, P=None, op=None):
        """solver/cg_mms_tm_nd.c with M_ndpsi = Qtm_pm_ndpsi: (iterations, [(Pup_i, Pdn_i) ...]), one pair per shift; P: pairs to
        reuse as the solution fields (allocated otherwise).  Shifts still active at the end: nd_active_shifts().
        op None: the un-suffixed call; "Qtm_pm_ndpsi" / "Qsw_pm_ndpsi": tmhip_cg_mms_tm_nd_op."""
        n = len(shifts)
        if P is None:
            P = [(self.field(), self.field()) for _ in range(n)]
        vp = C.c_void_p
        up = (vp * n)(*[p[0].h for p in P])
        dn = (vp * n)(*[p[1].h for p in P])
        sh = (C.c_double * n)(*shifts)
        it = C.c_int()
        if op is None:
            _ck(self.lib.tmhip_cg_mms_tm_nd(self.h, up, dn, Q_up.h, Q_dn.h, sh, n, max_iter, eps_sq, rel_prec, C.byref(it)), "cg_mms_tm_nd")
        else:
            _ck(self.lib.tmhip_cg_mms_tm_nd_op(self.h, up, dn, Q_up.h, Q_dn.h, sh, n, max_iter, eps_sq, rel_prec, ND_OPS[op], C.byref(it)), "cg_mms_tm_nd_op")
        return it.value, P

    def mixed_cg_mms_tm_nd(self, Q_up, Q_dn, shifts, max_iter, eps_sq, rel_prec, P=None, op="Qtm_pm_ndpsi"):
        """solver/mixed_cg_mms_tm_nd.c with M_ndpsi = Qtm_pm_ndpsi, M_ndpsi32 = Qtm_pm_ndpsi_32: the fp32 multi-shift CG with reliable
        updates.  Returns (iterations or -1, (reliable updates, shifts removed), [(Pup_i, Pdn_i) ...]); P as in cg_mms_tm_nd.
        Shifts still active at the end: nd_active_shifts().  Options "mms32_fused" and "cg_batch" change the launches, not the result."""
        n = len(shifts)
        if P is None:
            P = [(self.field(), self.field()) for _ in range(n)]
        vp = C.c_void_p
        up = (vp * n)(*[p[0].h for p in P])
        dn = (vp * n)(*[p[1].h for p in P])
        sh = (C.c_double * n)(*shifts)
        it, nrel, nrem = C.c_int(), C.c_int(), C.c_int()
        _ck(self.lib.tmhip_mixed_cg_mms_tm_nd(self.h, up, dn, Q_up.h, Q_dn.h, sh, n, max_iter, eps_sq, rel_prec, ND_OPS[op], C.byref(it),
                                              C.byref(nrel), C.byref(nrem)), "mixed_cg_mms_tm_nd")
        return it.value, (nrel.value, nrem.value), P

    def nd_active_shifts(self):
        return self.lib.tmhip_nd_active_shifts(self.h)

    # --- the clover doublet (Qsw_*_ndpsi, operator/tm_operators_nd.c; the _nd functions of operator/clovertm_operators.c) ---
    def sw_invert_nd(self, mshift):
        """operator/clover_invert.c:440: ((1+T)^2 + mshift)^-1 on the even sites, into sw_inv_nd (needs sw_term or set_clover first)."""
        _ck(self.lib.tmhip_sw_invert_nd(self.h, mshift), "tmhip_sw_invert_nd")

    def sw_invert_failures(self):
        """near-singular pivots met by the last sw_invert / sw_invert_nd"""
        n = C.c_int()
        _ck(self.lib.tmhip_sw_invert_failures(self.h, C.byref(n)), "tmhip_sw_invert_failures")
        return n.value

    def get_clover_nd(self):
        """sw_inv_nd in the reference's host layout sw_inv[icx][0..3][i]: [V/2][4][2][3][3][2]"""
        swi = np.zeros((self.Vh, 4, 2, 3, 3, 2))
        _ck(self.lib.tmhip_get_clover_nd(self.h, _hp(swi)), "tmhip_get_clover_nd")
        return swi

    def assign_mul_one_sw_pm_imu_eps(self, ieo, k_s, k_c, l_s, l_c, mu, eps):
        _ck(self.lib.tmhip_assign_mul_one_sw_pm_imu_eps(self.h, ieo, k_s.h, k_c.h, l_s.h, l_c.h, mu, eps), "assign_mul_one_sw_pm_imu_eps")

    def clover_inv_nd(self, ieo, l_c, l_s):
        _ck(self.lib.tmhip_clover_inv_nd(self.h, ieo, l_c.h, l_s.h), "clover_inv_nd")

    def clover_gamma5_nd(self, ieo, l_c, l_s, k_c, k_s, j_c, j_s, mubar, epsbar):
        _ck(self.lib.tmhip_clover_gamma5_nd(self.h, ieo, l_c.h, l_s.h, k_c.h, k_s.h, j_c.h, j_s.h, mubar, epsbar), "clover_gamma5_nd")

    def Qsw_ndpsi(self, l_s, l_c, k_s, k_c):
        _ck(self.lib.tmhip_Qsw_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "Qsw_ndpsi")

    def Qsw_dagger_ndpsi(self, l_s, l_c, k_s, k_c):
        _ck(self.lib.tmhip_Qsw_dagger_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "Qsw_dagger_ndpsi")

    def Qsw_pm_ndpsi(self, l_s, l_c, k_s, k_c):
        _ck(self.lib.tmhip_Qsw_pm_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "Qsw_pm_ndpsi")

    def Qsw_tau1_sub_const_ndpsi(self, l_s, l_c, k_s, k_c, z, Cpol, invev):
        """tm_operators_nd.c:378-444 (complex z)"""
        z = complex(z)
        _ck(self.lib.tmhip_Qsw_tau1_sub_const_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h, z.real, z.imag, Cpol, invev), "Qsw_tau1_sub_const_ndpsi")

    def H_eo_sw_ndpsi(self, l_s, l_c, k_s, k_c):
        _ck(self.lib.tmhip_H_eo_sw_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "H_eo_sw_ndpsi")

    def Msw_ee_inv_ndpsi(self, l_s, l_c, k_s, k_c):
        _ck(self.lib.tmhip_Msw_ee_inv_ndpsi(self.h, l_s.h, l_c.h, k_s.h, k_c.h), "Msw_ee_inv_ndpsi")

    def sw_deriv_nd(self, ieo):
        _ck(self.lib.tmhip_sw_deriv_nd(self.h, ieo), "sw_deriv_nd")

    # --- single-flavour multi-shift CG (solver/cg_mms_tm.c) ---------------------------------------------------------------
    def cg_mms_tm(self, Q, shifts, max_iter, eps_sq, rel_prec, op="Qtm_pm_psi", P=None):
        """solver/cg_mms_tm.c: (iterations, reached_prec, [P_0, P_1, ...]), one solution per shift; op Qtm_pm_psi / Qsw_pm_psi
        (one-parity fields, N = VOLUME/2) or Q_pm_psi (FULL fields, N = VOLUME).  P: fields to reuse as the solutions (allocated
        otherwise).  Shifts still active at the end: mms_active_shifts()."""
        full = op == "Q_pm_psi"
        n = len(shifts)
        if P is None:
            P = [self.field(kind=FIELD_FULL if full else FIELD_EO) for _ in range(n)]
        arr = (C.c_void_p * max(n, 1))(*[p.h for p in P])
        sh = (C.c_double * max(n, 1))(*shifts)
        it, prec = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_cg_mms_tm(self.h, arr, Q.h, sh, n, max_iter, eps_sq, rel_prec, self.V if full else self.Vh, MMS_OPS[op],
                                     C.byref(it), C.byref(prec)), "cg_mms_tm")
        return it.value, prec.value, P

    def mms_active_shifts(self):
        return self.lib.tmhip_mms_active_shifts(self.h)

    def mms_form(self):
        """0: fused e/o stencils, 1: unfused e/o form, 2: FULL composite (the last cg_mms_tm)"""
        return self.lib.tmhip_mms_form(self.h)

    # --- rational monomials (monomial/ndrat_monomial.c NDRAT, monomial/rat_monomial.c RAT; rational.hip) -----------------
    @staticmethod
    def _da(x):
        x = [float(v) for v in x]
        return (C.c_double * max(len(x), 1))(*x), len(x)

    def ndrat_force(self, chi, mu, rmu, invmaxev):
        """ndrat_monomial.c:114-160 given the solutions chi = [(up_j, dn_j) ...]; added to the derivative accumulator."""
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        vp = C.c_void_p * max(n, 1)
        _ck(self.lib.tmhip_ndrat_force(self.h, vp(*[p[0].h for p in chi]), vp(*[p[1].h for p in chi]), m, r, n, invmaxev), "ndrat_force")

    def ndrat_derivative(self, pf_up, pf_dn, mu, rmu, invmaxev, max_iter, eps_sq, rel_prec):
        """ndrat_monomial.c:96-160 (solve + force); returns the solver's iteration count."""
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it = C.c_int()
        _ck(self.lib.tmhip_ndrat_derivative(self.h, pf_up.h, pf_dn.h, m, r, n, invmaxev, max_iter, eps_sq, rel_prec, C.byref(it)), "ndrat_derivative")
        return it.value

    def ndrat_heatbath(self, pf_up, pf_dn, nu, rnu, invmaxev, max_iter, eps_sq, rel_prec):
        """ndrat_monomial.c:212-254: pf holds eta on entry, C eta on exit; returns (energy0, iterations)."""
        (m, n), (r, _) = self._da(nu), self._da(rnu)
        it, e = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_ndrat_heatbath(self.h, pf_up.h, pf_dn.h, m, r, n, invmaxev, max_iter, eps_sq, rel_prec, C.byref(e), C.byref(it)), "ndrat_heatbath")
        return e.value, it.value

    def ndrat_acc(self, pf_up, pf_dn, mu, rmu, max_iter, eps_sq, rel_prec):
        """ndrat_monomial.c:281-309; returns (energy1, iterations)."""
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it, e = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_ndrat_acc(self.h, pf_up.h, pf_dn.h, m, r, n, max_iter, eps_sq, rel_prec, C.byref(e), C.byref(it)), "ndrat_acc")
        return e.value, it.value

    # --- polynomial monomial (monomial/ndpoly_monomial.c NDPOLY, Ptilde_nd.c; poly.hip) ----------------------------------
    @staticmethod
    def _ca(z):
        """complex numbers as (re, im) pairs of doubles"""
        z = np.ascontiguousarray(np.asarray(z, dtype=np.complex128))
        return z.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)), len(z), z

    def assign_mul_add_mul_add_mul_add_mul_r(self, R, S, U, V, c1, c2, c3, c4):
        """linalg/assign_mul_add_mul_add_mul_add_mul_r.c with N = VOLUME/2: R = c1 R + c2 S + c3 U + c4 V"""
        _ck(self.lib.tmhip_assign_mul_add_mul_add_mul_add_mul_r(self.h, R.h, S.h, U.h, V.h, c1, c2, c3, c4), "assign_mul_add_mul_add_mul_add_mul_r")

    def comb4_ndpsi(self, out, A, B, Cc, D, c1, c2, c3, c4):
        """out = c1 A + c2 B + c3 C + c4 D for both flavours of a doublet (pairs of fields) in one launch; out may be an input pair"""
        h = [f.h for p in (out, A, B, Cc, D) for f in p]
        _ck(self.lib.tmhip_comb4_ndpsi(self.h, *h, c1, c2, c3, c4), "comb4_ndpsi")

    def Ptilde_ndpsi(self, R_s, R_c, coefs, S_s, S_c, evmin, evmax, op="Qtm_pm_ndpsi"):
        """Ptilde_nd.c:102-203 with Qsq = op and phmc_cheb_evmin / evmax = evmin / evmax; R may be S"""
        c, n = self._da(coefs)
        _ck(self.lib.tmhip_Ptilde_ndpsi(self.h, R_s.h, R_c.h, c, n, S_s.h, S_c.h, evmin, evmax, ND_OPS[op]), "Ptilde_ndpsi")

    def ndpoly_derivative(self, pf_up, pf_dn, roots, Cpol, invmaxev, n=None):
        """ndpoly_monomial.c:79-117, added to the derivative accumulator; roots: the 2n - 2 complex MDPolyRoots (n = MDPolyDegree)."""
        r, nr, _keep = self._ca(roots)
        n = nr // 2 + 1 if n is None else n
        _ck(self.lib.tmhip_ndpoly_derivative(self.h, pf_up.h, pf_dn.h, r, n, Cpol, invmaxev), "ndpoly_derivative")

    def ndpoly_heatbath(self, pf_up, pf_dn, roots, Cpol, invmaxev, ptilde_coefs, evmin, evmax):
        """ndpoly_monomial.c:179-209, 255-256: pf holds eta on entry, Ptilde B^dagger Q eta on exit; returns energy0."""
        r, nr, _keep = self._ca(roots)
        c, nc = self._da(ptilde_coefs)
        e = C.c_double()
        _ck(self.lib.tmhip_ndpoly_heatbath(self.h, pf_up.h, pf_dn.h, r, nr // 2 + 1, Cpol, invmaxev, c, nc, evmin, evmax, C.byref(e)), "ndpoly_heatbath")
        return e.value

    def ndpoly_acc(self, pf_up, pf_dn, roots, Cpol, invmaxev, md_coefs, ptilde_coefs, evmin, evmax, precision_hfinal):
        """ndpoly_monomial.c:282-368; returns (energy1, corrections, Ener[0 .. 7])."""
        r, nr, _keep = self._ca(roots)
        (m, nm), (c, nc) = self._da(md_coefs), self._da(ptilde_coefs)
        if nm != nr // 2 + 1:
            raise TmHipError("ndpoly_acc: %d MDPolyCoefs for %d roots" % (nm, nr))
        e, k, ener = C.c_double(), C.c_int(), (C.c_double * 8)()
        _ck(self.lib.tmhip_ndpoly_acc(self.h, pf_up.h, pf_dn.h, r, nm, Cpol, invmaxev, m, c, nc, evmin, evmax, precision_hfinal, C.byref(e), C.byref(k), ener),
            "ndpoly_acc")
        return e.value, k.value, list(ener)

    def ndcloverrat_force(self, chi, mu, rmu, invmaxev, kappa, c_sw, trlog):
        """ndrat_monomial.c:80-86, :114-184 for NDCLOVERRAT given the solutions; needs sw_term + sw_invert_nd on the current links."""
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        vp = C.c_void_p * max(n, 1)
        _ck(self.lib.tmhip_ndcloverrat_force(self.h, vp(*[p[0].h for p in chi]), vp(*[p[1].h for p in chi]), m, r, n, invmaxev, kappa, c_sw, int(trlog)),
            "ndcloverrat_force")

    def ndcloverrat_derivative(self, pf_up, pf_dn, mu, rmu, invmaxev, kappa, c_sw, trlog, max_iter, eps_sq, rel_prec):
        """solve with Qsw_pm_ndpsi + force; returns the solver's iteration count."""
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it = C.c_int()
        _ck(self.lib.tmhip_ndcloverrat_derivative(self.h, pf_up.h, pf_dn.h, m, r, n, invmaxev, kappa, c_sw, int(trlog), max_iter, eps_sq, rel_prec, C.byref(it)),
            "ndcloverrat_derivative")
        return it.value

    def ndcloverrat_heatbath(self, pf_up, pf_dn, nu, rnu, invmaxev, max_iter, eps_sq, rel_prec):
        (m, n), (r, _) = self._da(nu), self._da(rnu)
        it, e = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_ndcloverrat_heatbath(self.h, pf_up.h, pf_dn.h, m, r, n, invmaxev, max_iter, eps_sq, rel_prec, C.byref(e), C.byref(it)), "ndcloverrat_heatbath")
        return e.value, it.value

    def ndcloverrat_acc(self, pf_up, pf_dn, mu, rmu, max_iter, eps_sq, rel_prec):
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it, e = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_ndcloverrat_acc(self.h, pf_up.h, pf_dn.h, m, r, n, max_iter, eps_sq, rel_prec, C.byref(e), C.byref(it)), "ndcloverrat_acc")
        return e.value, it.value

    def rat_force(self, chi, rmu):
        """rat_monomial.c:95-132 (type RAT) given the solutions chi = [chi_j ...]; runs at twisted mass 0."""
        r, n = self._da(rmu)
        _ck(self.lib.tmhip_rat_force(self.h, (C.c_void_p * max(n, 1))(*[f.h for f in chi]), r, n), "rat_force")

    def rat_derivative(self, pf, mu, rmu, max_iter, eps_sq, rel_prec):
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it = C.c_int()
        _ck(self.lib.tmhip_rat_derivative(self.h, pf.h, m, r, n, max_iter, eps_sq, rel_prec, C.byref(it)), "rat_derivative")
        return it.value

    def rat_heatbath(self, pf, nu, rnu, max_iter, eps_sq, rel_prec):
        (m, n), (r, _) = self._da(nu), self._da(rnu)
        it, e = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_rat_heatbath(self.h, pf.h, m, r, n, max_iter, eps_sq, rel_prec, C.byref(e), C.byref(it)), "rat_heatbath")
        return e.value, it.value

    def rat_acc(self, pf, mu, rmu, max_iter, eps_sq, rel_prec):
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it, e = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_rat_acc(self.h, pf.h, m, r, n, max_iter, eps_sq, rel_prec, C.byref(e), C.byref(it)), "rat_acc")
        return e.value, it.value

    def cloverrat_force(self, chi, rmu, kappa, c_sw, trlog):
        """rat_monomial.c:66-73, :95-139 for CLOVERRAT given the solutions chi = [chi_j ...]; needs sw_term + sw_invert(EE, 0.) on the
        current links; runs at twisted mass 0."""
        r, n = self._da(rmu)
        _ck(self.lib.tmhip_cloverrat_force(self.h, (C.c_void_p * max(n, 1))(*[f.h for f in chi]), r, n, kappa, c_sw, int(trlog)), "cloverrat_force")

    def cloverrat_derivative(self, pf, mu, rmu, kappa, c_sw, trlog, max_iter, eps_sq, rel_prec):
        """solve with Qsw_pm_psi + force; returns the solver's iteration count."""
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it = C.c_int()
        _ck(self.lib.tmhip_cloverrat_derivative(self.h, pf.h, m, r, n, kappa, c_sw, int(trlog), max_iter, eps_sq, rel_prec, C.byref(it)), "cloverrat_derivative")
        return it.value

    def cloverrat_heatbath(self, pf, nu, rnu, max_iter, eps_sq, rel_prec):
        (m, n), (r, _) = self._da(nu), self._da(rnu)
        it, e = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_cloverrat_heatbath(self.h, pf.h, m, r, n, max_iter, eps_sq, rel_prec, C.byref(e), C.byref(it)), "cloverrat_heatbath")
        return e.value, it.value

    def cloverrat_acc(self, pf, mu, rmu, max_iter, eps_sq, rel_prec):
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it, e = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_cloverrat_acc(self.h, pf.h, m, r, n, max_iter, eps_sq, rel_prec, C.byref(e), C.byref(it)), "cloverrat_acc")
        return e.value, it.value

    # --- correction monomials (monomial/ratcor_monomial.c, monomial/ndratcor_monomial.c; rational.hip, linalg.hip) -------
    def rat_sum(self, out, inp, chi, rmu, c=1.0):
        """out = c (in + sum_j rmu_j chi_j), added from j = np - 1 down to 0, in one launch; out may be in."""
        r, n = self._da(rmu)
        _ck(self.lib.tmhip_rat_sum(self.h, out.h, inp.h, self._handles(chi), r, n, c), "rat_sum")

    def rat_sum_nd(self, out, inp, chi, rmu, c=1.0):
        """rat_sum for both flavours in one launch: out, inp = (up, dn) pairs, chi = [(up_j, dn_j) ...]."""
        r, n = self._da(rmu)
        _ck(self.lib.tmhip_rat_sum_nd(self.h, out[0].h, out[1].h, inp[0].h, inp[1].h, self._handles([p[0] for p in chi]),
                                      self._handles([p[1] for p in chi]), r, n, c), "rat_sum_nd")

    def diff_sqnorm(self, k, l):
        """k = k - l; returns |k|^2 (one launch, one synchronisation)."""
        out = C.c_double()
        _ck(self.lib.tmhip_diff_sqnorm(self.h, k.h, l.h, C.byref(out)), "diff_sqnorm")
        return out.value

    def diff_sqnorm_nd(self, k, l):
        """diff_sqnorm for both flavours, k, l = (up, dn) pairs; returns |k_up|^2 + |k_dn|^2."""
        out = C.c_double()
        _ck(self.lib.tmhip_diff_sqnorm_nd(self.h, k[0].h, k[1].h, l[0].h, l[1].h, C.byref(out)), "diff_sqnorm_nd")
        return out.value

    def apply_Z(self, k, l, mu, rmu, A, max_iter, eps_sq, rel_prec, op="Qtm_pm_psi"):
        """ratcor_monomial.c:183-218: k = (Q^2 (A R)^2 - 1) l; returns (delta, the first solve's return value)."""
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it, dl = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_apply_Z(self.h, k.h, l.h, m, r, A, n, max_iter, eps_sq, rel_prec, MMS_OPS[op], C.byref(dl), C.byref(it)), "apply_Z")
        return dl.value, it.value

    def apply_Z_nd(self, k, l, mu, rmu, A, max_iter, eps_sq, rel_prec, op="Qtm_pm_ndpsi"):
        """ndratcor_monomial.c:202-245 on (up, dn) pairs k, l; returns (delta, the first solve's return value)."""
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it, dl = C.c_int(), C.c_double()
        _ck(self.lib.tmhip_apply_Z_nd(self.h, k[0].h, k[1].h, l[0].h, l[1].h, m, r, A, n, max_iter, eps_sq, rel_prec, ND_OPS[op], C.byref(dl), C.byref(it)),
            "apply_Z_nd")
        return dl.value, it.value

    def _ratcor(self, fn, what, pfs, mu, rmu, A, max_iter, accprec, rel_prec, op):
        (m, n), (r, _) = self._da(mu), self._da(rmu)
        it, na, e = C.c_int(), C.c_int(), C.c_double()
        _ck(fn(self.h, *[f.h for f in pfs], m, r, A, n, max_iter, accprec, rel_prec, op, C.byref(e), C.byref(na), C.byref(it)), what)
        return e.value, na.value, it.value

    def ratcor_heatbath(self, pf, mu, rmu, A, max_iter, accprec, rel_prec, op="Qtm_pm_psi"):
        """ratcor_monomial.c:85-110 (op Qsw_pm_psi: CLOVERRATCOR): pf holds eta on entry, B eta on exit; returns (energy0, applications
        of Z, summed first-solve iterations)."""
        return self._ratcor(self.lib.tmhip_ratcor_heatbath, "ratcor_heatbath", [pf], mu, rmu, A, max_iter, accprec, rel_prec, MMS_OPS[op])

    def ratcor_acc(self, pf, mu, rmu, A, max_iter, accprec, rel_prec, op="Qtm_pm_psi"):
        """ratcor_monomial.c:151-168; returns (energy1, applications of Z, summed first-solve iterations)."""
        return self._ratcor(self.lib.tmhip_ratcor_acc, "ratcor_acc", [pf], mu, rmu, A, max_iter, accprec, rel_prec, MMS_OPS[op])

    def ndratcor_heatbath(self, pf_up, pf_dn, mu, rmu, A, max_iter, accprec, rel_prec, op="Qtm_pm_ndpsi"):
        """ndratcor_monomial.c:88-123 (op Qsw_pm_ndpsi: NDCLOVERRATCOR); returns (energy0, applications of Z, iterations)."""
        return self._ratcor(self.lib.tmhip_ndratcor_heatbath, "ndratcor_heatbath", [pf_up, pf_dn], mu, rmu, A, max_iter, accprec, rel_prec, ND_OPS[op])

    def ndratcor_acc(self, pf_up, pf_dn, mu, rmu, A, max_iter, accprec, rel_prec, op="Qtm_pm_ndpsi"):
        """ndratcor_monomial.c:166-187; returns (energy1, applications of Z, iterations)."""
        return self._ratcor(self.lib.tmhip_ndratcor_acc, "ndratcor_acc", [pf_up, pf_dn], mu, rmu, A, max_iter, accprec, rel_prec, ND_OPS[op])

    # --- multi-GPU --------------------------------------------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        _ck(self.lib.tmhip_comm_get_unique_id(buf), "tmhip_comm_get_unique_id")
        return buf.raw

    def comm_init(self, uid):
        _ck(self.lib.tmhip_comm_init(self.h, uid), "tmhip_comm_init")

    def comm_init_shm(self, job):
        """the ring over the host-staged shared-memory transport (ranks of one node, no RCCL; `job`: the same string on every rank)"""
        _ck(self.lib.tmhip_comm_init_shm(self.h, job.encode()), "tmhip_comm_init_shm")

    def comm_init_ipc(self):
        """the direct face carrier on top of the ring (collective, after comm_init / comm_init_shm): faces are stored by the producing
        waves straight into the ring neighbours' IPC-mapped receive buffers"""
        _ck(self.lib.tmhip_comm_init_ipc(self.h), "tmhip_comm_init_ipc")

    def comm_faces_direct(self):
        """(True when the faces travel as direct stores, ranks of the job on this rank's GPU)"""
        n = C.c_int()
        v = self.lib.tmhip_comm_faces_direct(self.h, C.byref(n))
        return bool(v), n.value

    def comm_sums_direct(self):
        """True when the scalar sums over the ranks travel as direct stores into every rank's block (no communicator involved)"""
        return bool(self.lib.tmhip_comm_sums_direct(self.h))

    def comm_count(self):
        """(ranks of the face communicator, ranks of the reduction communicator) as RCCL reports them; (0, 0) without one."""
        a, b = C.c_int(), C.c_int()
        _ck(self.lib.tmhip_comm_count(self.h, C.byref(a), C.byref(b)), "tmhip_comm_count")
        return a.value, b.value

    def comm_is_split(self):
        """True: reductions on their own communicator; False: they share the face communicator; None: no communicator."""
        v = self.lib.tmhip_comm_is_split(self.h)
        return None if v < 0 else bool(v)

    def set_loopback(self, on):
        _ck(self.lib.tmhip_comm_set_loopback(self.h, int(on)), "tmhip_comm_set_loopback")

    def comm_stream_delay_ms(self, ms):
        """Test hook: hold the comm stream back for `ms` milliseconds in front of the next halo exchange (a late neighbour)."""
        _ck(self.lib.tmhip_comm_stream_delay_ms(self.h, int(ms)), "tmhip_comm_stream_delay_ms")

    # --- measurement ------------------------------------------------------
    def bench_hopping(self, f0, f1, f2, iters):
        ms = C.c_double()
        _ck(self.lib.tmhip_bench_hopping(self.h, f0.h, f1.h, f2.h, iters, C.byref(ms)), "tmhip_bench_hopping")
        return ms.value

    def event_record(self, slot):
        _ck(self.lib.tmhip_event_record(self.h, slot), "tmhip_event_record")

    def event_elapsed_ms(self, a, b):
        ms = C.c_double()
        _ck(self.lib.tmhip_event_elapsed_ms(self.h, a, b, C.byref(ms)), "tmhip_event_elapsed_ms")
        return ms.value


def multi_Hopping_Matrix(lats, ieo, ls, ks):
    """Hopping_Matrix on a T-split lattice held by several contexts of THIS process (peer-copy ring)."""
    n = len(lats)
    arr = C.c_void_p * n
    _ck(lats[0].lib.tmhip_multi_hopping_matrix(n, arr(*[l.h for l in lats]), ieo, arr(*[f.h for f in ls]),
                                               arr(*[f.h for f in ks])), "tmhip_multi_hopping_matrix")


def multi_deriv_Sb(lats, ieo, ls, ks, factor):
    """deriv_Sb on a T-split lattice held by several contexts of THIS process (peer-copy ring)."""
    n = len(lats)
    arr = C.c_void_p * n
    _ck(lats[0].lib.tmhip_multi_deriv_Sb(n, arr(*[l.h for l in lats]), ieo, arr(*[f.h for f in ls]), arr(*[f.h for f in ks]),
                                         factor), "tmhip_multi_deriv_Sb")


def multi_sw_all(lats, kappa, c_sw):
    """sw_all on a T-split lattice held by several contexts of THIS process (two-sided derivative halo by peer copies)."""
    n = len(lats)
    arr = C.c_void_p * n
    _ck(lats[0].lib.tmhip_multi_sw_all(n, arr(*[l.h for l in lats]), kappa, c_sw), "tmhip_multi_sw_all")


def multi_update_gauge(lats, step):
    """update_gauge on a T-split lattice held by several contexts of THIS process: links updated, halo slabs by peer copies, stencil copies re-sorted."""
    n = len(lats)
    arr = C.c_void_p * n
    _ck(lats[0].lib.tmhip_multi_update_gauge(n, arr(*[l.h for l in lats]), step), "tmhip_multi_update_gauge")
