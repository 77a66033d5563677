"""ctypes binding of the C ABI in include/mhh_hip.h (libmhh_hip.so, hand-written HIP for gfx950).

This is the ONLY compute path of the package: if the shared library is missing the import of a symbol
fails loudly -- there is no CPU or PyTorch fallback. (tests/ can bind the same signatures onto other
libraries -- the CPU emulation build of the kernels -- through ``bind``.)
"""
import ctypes as C
import os

from .grid import MhhGrid, MAX_SCALARS

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmhh_hip.so")

vp, ci, cd = C.c_void_p, C.c_int, C.c_double
GP = C.POINTER(MhhGrid)


class MhhFields(C.Structure):
    _fields_ = [("u", vp), ("v", vp), ("w", vp), ("ut", vp), ("vt", vp), ("wt", vp),
                ("nscalars", ci),
                ("s", vp * MAX_SCALARS), ("st", vp * MAX_SCALARS), ("svisc", cd * MAX_SCALARS),
                ("evisc", vp), ("p", vp), ("rhoref", vp), ("rhorefh", vp), ("visc", cd),
                ("u_fluxbot", vp), ("u_fluxtop", vp), ("v_fluxbot", vp), ("v_fluxtop", vp),
                ("s_fluxbot", vp * MAX_SCALARS), ("s_fluxtop", vp * MAX_SCALARS),
                ("dudz", vp), ("dvdz", vp), ("dbdz", vp), ("z0m", vp),
                ("s_fluxlimit", ci * MAX_SCALARS)]


class MhhDiffParams(C.Structure):
    _fields_ = [("cs", cd), ("tPr", cd), ("surface_model", ci), ("neutral", ci), ("N2", vp),
                ("th_for_N2", ci), ("thref", vp), ("grav", cd), ("mlen0", vp),
                ("buoyancy", ci), ("threfh", vp), ("evisc_ghost_rows", ci), ("mlen2", vp),
                ("buoyancy_kind", ci), ("bg_n2", cd), ("alpha", cd), ("utrans", cd)]


class MhhBufferParams(C.Structure):
    _fields_ = [("swbuffer", ci), ("bufferkstart", ci), ("bufferkstarth", ci), ("sigma", vp), ("sigmah", vp),
                ("abuf_u", vp), ("abuf_v", vp), ("abuf_w", vp), ("abuf_s", vp * MAX_SCALARS)]


class MhhForceParams(C.Structure):
    _fields_ = [("swlspres", ci), ("order", ci), ("dpdx", cd), ("uflux", cd), ("dt", cd), ("uflux_sums", vp),
                ("fc", cd), ("utrans", cd), ("vtrans", cd), ("ug", vp), ("vg", vp),
                ("swls", ci), ("ls_u", vp), ("ls_v", vp), ("ls_s", vp * MAX_SCALARS),
                ("swwls", ci), ("swwls_mom", ci), ("wls", vp),
                ("mean_u", vp), ("mean_v", vp), ("mean_s", vp * MAX_SCALARS),
                ("swnudge", ci), ("nudge_factor", vp), ("nudge_u", vp), ("nudge_v", vp), ("nudge_s", vp * MAX_SCALARS)]


class MhhSurfaceParams(C.Structure):
    _fields_ = [("mbcbot", ci), ("thermobc", ci), ("thermo_kind", ci), ("thermo_index", ci), ("swconstantz0", ci), ("swcharnock", ci),
                ("thref_kstart", cd), ("threfh_kstart", cd), ("grav", cd), ("bg_n2", cd),
                ("zL", vp), ("f", vp), ("z0m", vp), ("z0h", vp), ("ustar", vp), ("obuk", vp), ("nobuk", vp),
                ("ubot", vp), ("vbot", vp), ("ugradbot", vp), ("vgradbot", vp),
                ("sbot", vp * MAX_SCALARS), ("sgradbot", vp * MAX_SCALARS), ("sbcbot", ci * MAX_SCALARS),
                ("qt_index", ci), ("thvref", vp), ("thvrefh", vp)]


class MhhMicroParams(C.Structure):
    _fields_ = [("Nc0", cd), ("dt", cd), ("processes", ci)]


class MhhRadiationGcssParams(C.Structure):
    _fields_ = [("xka", cd), ("fr0", cd), ("fr1", cd), ("div", cd), ("mu", cd), ("parts", ci)]


class MhhStatsJob(C.Structure):
    _fields_ = [("fld", vp), ("mean", vp), ("loc", ci), ("op", ci), ("offset", cd), ("threshold", cd),
                ("kind", ci), ("scheme", ci), ("limit", ci), ("surface_model", ci), ("w", vp), ("wmean", vp), ("evisc", vp),
                ("flux_bot", vp), ("flux_top", vp), ("visc", cd), ("tPr", cd), ("a", ci), ("b", ci)]


class MhhCrossJob(C.Structure):
    _fields_ = [("fld", vp), ("kind", ci), ("index", ci), ("k0", ci), ("k1", ci), ("offset", cd), ("out", vp)]


IP = C.POINTER(C.c_int)


class MhhIbGhostLists(C.Structure):
    _fields_ = [("i", IP), ("j", IP), ("k", IP), ("xb", vp), ("yb", vp), ("zb", vp), ("xi", vp), ("yi", vp), ("zi", vp), ("di", vp),
                ("ip_i", IP), ("ip_j", IP), ("ip_k", IP), ("ip_d", vp), ("c_idw", vp), ("c_idw_sum", vp)]


class MhhIbJob(C.Structure):
    _fields_ = [("fld", vp), ("boundary_value", vp), ("bc", ci), ("nghost", ci), ("visc", cd), ("cell", vp), ("ip", vp),
                ("c_idw", vp), ("c_idw_sum", vp), ("di", vp)]


class MhhBudget2Desc(C.Structure):
    _fields_ = [("u", vp), ("v", vp), ("w", vp), ("p", vp), ("evisc", vp), ("b", vp), ("u_fluxbot", vp), ("v_fluxbot", vp),
                ("umodel", vp), ("vmodel", vp), ("wmodel", vp), ("bmean", vp), ("pmean", vp),
                ("utrans", cd), ("vtrans", cd), ("fc", cd), ("order", ci), ("diff_scheme", ci), ("groups", C.c_uint)]


class MhhSourceDesc(C.Structure):
    _fields_ = [("scalar", ci), ("swvmr", ci), ("profile_index", ci), ("reserved", ci)] + \
               [(n, cd) for n in ("x0", "y0", "z0", "sigma_x", "sigma_y", "sigma_z", "line_x", "line_y", "line_z", "strength")]


class MhhDecayParams(C.Structure):
    _fields_ = [("exponential", ci * MAX_SCALARS), ("timescale", cd * MAX_SCALARS)]


FP = C.POINTER(MhhFields)
SP = C.POINTER(MhhSurfaceParams)
DP = C.POINTER(MhhDiffParams)
BP = C.POINTER(MhhBufferParams)
FRP = C.POINTER(MhhForceParams)
MP = C.POINTER(MhhMicroParams)
RP = C.POINTER(MhhRadiationGcssParams)
SJP = C.POINTER(MhhStatsJob)
BDP = C.POINTER(MhhBudget2Desc)
CJP = C.POINTER(MhhCrossJob)
IGP = C.POINTER(MhhIbGhostLists)
IJP = C.POINTER(MhhIbJob)
SDP = C.POINTER(MhhSourceDesc)
DCP = C.POINTER(MhhDecayParams)
CDP = C.POINTER(cd)
PLAN = vp

SIGNATURES = {
    "mhh_synchronize": (ci, [vp]),
    "mhh_version": (ci, []),
    "mhh_last_error": (C.c_char_p, []),
    "mhh_reduce_work_bytes": (C.c_ulonglong, []),
    "mhh_boundary_cyclic": (ci, [GP, vp, ci, vp]),
    "mhh_boundary_cyclic_2d": (ci, [GP, vp, vp]),
    "mhh_boundary_cyclic_u32": (ci, [GP, vp, ci, vp]),
    "mhh_boundary_cyclic_2d_u32": (ci, [GP, vp, vp]),
    "mhh_boundary_cyclic_n": (ci, [GP, C.POINTER(vp), ci, ci, vp]),
    "mhh_advec_u": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_advec_v": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_advec_w": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_advec_s": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_advec_s_lim": (ci, [GP, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_advec_exec": (ci, [GP, ci, FP, vp]),
    "mhh_stat_visc_march_launches": (C.c_ulonglong, []),
    "mhh_selftest_sqrt_in_range": (ci, [C.c_ulonglong, C.c_ulonglong, C.POINTER(C.c_ulonglong), vp]),
    "mhh_diff_exec_viscosity_rows": (ci, [GP, ci, FP, DP, ci, ci, vp]),
    "mhh_diff_exec_viscosity_rows2": (ci, [GP, ci, FP, DP, ci, ci, ci, ci, vp]),
    "mhh_rhs_exec_rows": (ci, [GP, ci, ci, FP, DP, ci, ci, vp]),
    "mhh_rhs_exec_rows2": (ci, [GP, ci, ci, FP, DP, ci, ci, ci, ci, vp]),
    "mhh_stat_rhs44_march_launches": (C.c_ulonglong, []),
    "mhh_stat_scalar_march_launches": (C.c_ulonglong, []),
    "mhh_stat_scalar4_march_launches": (C.c_ulonglong, []),
    "mhh_stat_march_form": (ci, [ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]),
    "mhh_thermo_dry_buoyancy_tend": (ci, [GP, ci, vp, vp, vp, cd, vp]),
    "mhh_thermo_buoy_tend": (ci, [GP, ci, FP, ci, cd, cd, cd, vp]),
    "mhh_thermo_buoy_N2": (ci, [GP, vp, vp, cd, vp]),
    "mhh_advec_cfl": (ci, [GP, ci, vp, vp, vp, cd, vp, C.POINTER(cd), vp]),
    "mhh_diff_c": (ci, [GP, ci, vp, vp, cd, vp]),
    "mhh_diff_w": (ci, [GP, ci, vp, vp, cd, vp]),
    "mhh_smag2_strain2": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_smag2_mlen0_host": (ci, [GP, cd, vp]),
    "mhh_smag2_mlen2_host": (ci, [GP, ci, ci, vp, cd, vp]),
    "mhh_smag2_evisc": (ci, [GP, ci, vp, vp, vp, vp, vp, cd, vp]),
    "mhh_smag2_evisc_neutral": (ci, [GP, ci, vp, vp, vp, vp, vp, cd, vp]),
    "mhh_smag2_diff_u": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, cd, vp]),
    "mhh_smag2_diff_v": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, cd, vp]),
    "mhh_smag2_diff_w": (ci, [GP, vp, vp, vp, vp, vp, vp, vp, cd, vp]),
    "mhh_smag2_diff_c": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp, cd, cd, vp]),
    "mhh_smag2_dnmul": (ci, [GP, vp, cd, vp, C.POINTER(cd), vp]),
    "mhh_calc_N2": (ci, [GP, vp, vp, vp, cd, vp]),
    "mhh_diff_exec_viscosity": (ci, [GP, ci, FP, DP, vp]),
    "mhh_diff_exec": (ci, [GP, ci, FP, DP, vp]),
    "mhh_rhs_exec": (ci, [GP, ci, ci, FP, DP, vp]),
    "mhh_pres_plan_create": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, C.POINTER(PLAN)]),
    "mhh_pres_plan_destroy": (None, [PLAN]),
    "mhh_pres_exec": (ci, [PLAN, GP, FP, cd, vp]),
    "mhh_pres_lds_stage": (ci, [PLAN, GP, FP, cd, ci, vp]),
    "mhh_pres_plan_has_lds_form": (ci, [PLAN]),
    "mhh_pres_exec_form": (ci, [PLAN]),
    "mhh_pres_plan_spectral": (vp, [PLAN]),
    "mhh_pres_input": (ci, [PLAN, GP, FP, cd, vp, vp]),
    "mhh_pres_solve": (ci, [PLAN, GP, FP, vp, vp]),
    "mhh_pres_output": (ci, [PLAN, GP, FP, vp]),
    "mhh_pres_check_divergence": (ci, [GP, ci, FP, vp, C.POINTER(cd), vp]),
    "mhh_rk_substep": (ci, [GP, ci, ci, cd, vp, vp, vp]),
    "mhh_pres_exec_rk": (ci, [PLAN, GP, FP, C.c_double, ci, ci, C.c_double, vp]),
    "mhh_boundary_ghost_cells": (ci, [GP, ci, vp, ci, ci, vp, vp, vp, vp, vp]),
    "mhh_boundary_ghost_cells_w": (ci, [GP, vp, ci, vp]),
    "mhh_pres_input_packed": (ci, [GP, ci, FP, cd, vp, vp]),
    "mhh_pres_output_order": (ci, [GP, ci, FP, vp]),
    "mhh_halo_buffer_elems": (C.c_ulonglong, [GP, ci]),
    "mhh_halo_pack_ns": (ci, [GP, C.POINTER(vp), ci, vp, vp, vp]),
    "mhh_halo_unpack_ns": (ci, [GP, C.POINTER(vp), ci, vp, vp, vp]),
    "mhh_halo_pack_rows": (ci, [GP, C.POINTER(vp), ci, ci, ci, vp, vp, vp]),
    "mhh_halo_unpack_rows": (ci, [GP, C.POINTER(vp), ci, ci, ci, vp, vp, vp]),
    "mhh_pres_slab_plan_create": (ci, [GP, vp, vp, vp, vp, C.POINTER(PLAN)]),
    "mhh_pres_slab_plan_destroy": (None, [PLAN]),
    "mhh_pres_slab_xbuf_elems": (C.c_ulonglong, [PLAN]),
    "mhh_pres_slab_packed": (vp, [PLAN]),
    "mhh_pres_fwd_x_pack": (ci, [PLAN, GP, vp, vp, vp]),
    "mhh_pres_fwd_y_solve_bwd_y": (ci, [PLAN, GP, vp, vp, vp]),
    "mhh_pres_bwd_x_unpack": (ci, [PLAN, GP, vp, FP, vp]),
    "mhh_pres_bwd_x_unpack_output": (ci, [PLAN, GP, vp, FP, vp]),
    "mhh_pres_output_south_row": (ci, [GP, FP, vp]),
    "mhh_pres_slab_set_chunks": (ci, [PLAN, ci]),
    "mhh_pres_slab_chunks": (ci, [PLAN]),
    "mhh_pres_fwd_x_pack_chunk": (ci, [PLAN, GP, vp, vp, ci, vp]),
    "mhh_pres_fwd_y_chunk": (ci, [PLAN, GP, vp, ci, vp]),
    "mhh_pres_solve_y": (ci, [PLAN, GP, vp]),
    "mhh_pres_bwd_y_chunk": (ci, [PLAN, GP, vp, ci, vp]),
    "mhh_pres_bwd_x_chunk": (ci, [PLAN, GP, vp, ci, vp]),
    "mhh_pres_unpack_output_slab": (ci, [PLAN, GP, FP, vp]),
    "mhh_pres_slab_has_lds": (ci, [PLAN]),
    "mhh_pres_slab_lds_fwd": (ci, [PLAN, GP, FP, C.c_double, vp, ci, vp]),
    "mhh_pres_slab_lds_bwd": (ci, [PLAN, GP, vp, FP, ci, vp]),
    "mhh_pres_slab_lds_fwd_y": (ci, [PLAN, GP, vp, ci, vp]),
    "mhh_pres_slab_lds_bwd_y": (ci, [PLAN, GP, vp, ci, vp]),
    "mhh_pres_slab_plan_create_order": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, C.POINTER(PLAN)]),
    "mhh_pres_slab_order": (ci, [PLAN]),
    "mhh_pres_unpack_slab": (ci, [PLAN, GP, FP, vp]),
    "mhh_field_mean_scratch_elems": (C.c_ulonglong, [GP, ci]),
    "mhh_field_mean_chunk_rows": (ci, []),
    "mhh_field_mean_profile": (ci, [GP, C.POINTER(vp), ci, C.POINTER(vp), vp, vp]),
    "mhh_field_mean_sum": (ci, [GP, C.POINTER(vp), ci, vp, vp, vp]),
    "mhh_buffer_sigma_host": (ci, [GP, cd, cd, cd, ci, vp]),
    "mhh_buffer_exec": (ci, [GP, FP, BP, vp]),
    "mhh_force_exec": (ci, [GP, FP, FRP, vp]),
    "mhh_buffer_force_exec": (ci, [GP, FP, BP, FRP, vp]),
    "mhh_surface_lut_host": (ci, [cd, cd, cd, ci, ci, ci, vp, vp]),
    "mhh_surface_dutot": (ci, [GP, FP, SP, vp, vp]),
    "mhh_surface_stability": (ci, [GP, FP, SP, vp, vp]),
    "mhh_surface_momentum": (ci, [GP, FP, SP, vp]),
    "mhh_surface_scalar": (ci, [GP, FP, SP, ci, vp]),
    "mhh_surface_mo_gradients": (ci, [GP, FP, SP, vp]),
    "mhh_boundary_surface_exec": (ci, [GP, FP, SP, vp, vp]),
    "mhh_thermo_moist_sat_adjust": (ci, [ci, C.c_longlong, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_thermo_moist_buoyancy_tend": (ci, [GP, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_thermo_moist_buoyancy_tend_impl": (ci, [GP, ci, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_thermo_moist_fields": (ci, [GP, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_thermo_moist_base_state_host": (ci, [GP, vp, vp, cd, ci, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_thermo_moist_base_state": (ci, [GP, vp, vp, cd, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_micro_2mom_warm_exec": (ci, [GP, MP] + [vp]*15),
    "mhh_micro_2mom_warm_exec_impl": (ci, [GP, ci, MP] + [vp]*15),
    "mhh_micro_2mom_warm_cfl": (ci, [GP, vp, vp, vp, cd, vp, C.POINTER(cd), vp]),
    "mhh_limiter_exec": (ci, [GP, vp, vp, cd, vp]),
    "mhh_micro_nsw6_exec": (ci, [GP, MP] + [vp]*21),
    "mhh_micro_nsw6_exec_impl": (ci, [GP, ci, MP] + [vp]*21),
    "mhh_micro_nsw6_cfl": (ci, [GP, vp, vp, vp, vp, cd, vp, C.POINTER(cd), vp]),
    "mhh_micro_nsw6_cfl_impl": (ci, [GP, ci, vp, vp, vp, vp, cd, vp, C.POINTER(cd), vp]),
    "mhh_radiation_gcss_zenith_host": (ci, [ci, cd, cd, cd, C.POINTER(cd)]),
    "mhh_radiation_gcss_exec": (ci, [GP, RP] + [vp]*12),
    "mhh_radiation_gcss_exec_impl": (ci, [GP, ci, RP] + [vp]*12),
    "mhh_thermo_moist_ql_h": (ci, [GP, vp, vp, vp, vp, vp, vp, vp]),
    "mhh_stats_interpolate_w": (ci, [GP, vp, vp, vp]),
    "mhh_stats_scratch_elems": (C.c_ulonglong, [GP, ci, ci]),
    "mhh_stats_chunk_rows": (ci, []),
    "mhh_stats_mask_init": (ci, [GP, vp, vp, ci, vp]),
    "mhh_stats_mask_thres": (ci, [GP, vp, vp, ci, vp, vp, vp, cd, ci, vp]),
    "mhh_stats_mask_count": (ci, [GP, vp, vp, ci, vp, vp, vp]),
    "mhh_stats_mask_finish": (ci, [GP, ci, vp, vp, vp, vp, vp, vp]),
    "mhh_stats_sums": (ci, [GP, vp, ci, SJP, ci, vp, vp, vp]),
    "mhh_stats_finish": (ci, [GP, ci, SJP, ci, vp, vp, vp, vp]),
    "mhh_stats_columns": (ci, [GP, vp, ci, vp, ci, cd, cd, vp, vp, vp, vp]),
    "mhh_stats_columns_finish": (ci, [GP, ci, vp, vp, vp]),
    "mhh_budget_2_nprofs": (ci, [C.c_uint]),
    "mhh_budget_2_prof_name": (C.c_char_p, [C.c_uint, ci, C.POINTER(ci)]),
    "mhh_budget_2_scratch_elems": (C.c_ulonglong, [GP, ci]),
    "mhh_budget_2_model_sums": (ci, [GP, vp, ci, vp, vp, vp, vp, vp, vp]),
    "mhh_budget_2_model_finish": (ci, [GP, ci, vp, vp, vp, vp]),
    "mhh_budget_2_sums": (ci, [GP, vp, ci, BDP, vp, vp, vp]),
    "mhh_budget_2_finish": (ci, [GP, ci, BDP, vp, vp, vp, vp]),
    "mhh_thermo_dry_buoyancy": (ci, [GP, vp, vp, vp, cd, vp]),
    "mhh_cross_gather": (ci, [GP, CJP, ci, vp]),
    "mhh_cross_lngrad": (ci, [GP, ci, CJP, ci, vp]),
    "mhh_cross_path": (ci, [GP, vp, vp, vp, vp]),
    "mhh_cross_height_threshold": (ci, [GP, vp, cd, ci, vp, vp]),
    "mhh_cross_indices_host": (ci, [GP, ci, C.POINTER(cd), ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]),
    "mhh_ib_ghost_cells_host": (ci, [GP, vp, vp, vp, vp, vp, ci, ci, ci, ci, C.POINTER(ci), IGP]),
    "mhh_ib_k_dem_host": (ci, [GP, vp, vp, vp]),
    "mhh_ib_interp_dem_host": (ci, [GP, vp, vp, vp, vp, vp, ci, ci, ci, vp]),
    "mhh_ib_set_ghost_cells": (ci, [GP, ci, IJP, ci, vp]),
    "mhh_ib_mask": (ci, [GP, vp, vp, vp, vp]),
    "mhh_ib_fluxbot": (ci, [GP, vp, vp, vp, cd, vp]),
    "mhh_source_create": (ci, [GP, SDP, ci, vp, ci, vp, vp, C.POINTER(vp)]),
    "mhh_source_destroy": (None, [vp]),
    "mhh_source_update": (ci, [vp, ci, CDP, CDP, CDP, CDP, vp]),
    "mhh_source_count": (ci, [vp]),
    "mhh_source_tiles": (ci, [vp]),
    "mhh_source_ranges": (ci, [vp, ci, C.POINTER(ci)]),
    "mhh_source_norm": (ci, [vp, ci, CDP]),
    "mhh_source_exec": (ci, [vp, GP, FP, vp]),
    "mhh_decay_exec": (ci, [GP, FP, DCP, cd, vp]),
    "mhh_decay_couvreux_scratch_elems": (C.c_ulonglong, [GP]),
    "mhh_decay_couvreux_sums": (ci, [GP, vp, vp, vp, vp]),
    "mhh_decay_couvreux_field": (ci, [GP, vp, vp, cd, vp, vp, vp]),
    "mhh_boundary_outflow_profile_host": (ci, [GP, vp, vp]),
    "mhh_boundary_outflow_exec": (ci, [GP, ci, C.POINTER(vp), ci, C.POINTER(vp), C.POINTER(ci), ci, vp]),
    "mhh_boundary_outflow_last_launches": (ci, []),
}


class MhhError(RuntimeError):
    """Non-zero status from the C ABI (the C++ adaptor throws std::runtime_error in the same place)."""


def bind(lib, required=True):
    """Attach argtypes/restype for every declared entry point; missing symbols raise."""
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if required:
                raise
            continue
        fn.restype = res
        fn.argtypes = args
    return lib


_lib = None


def lib():
    """The HIP library. Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        path = os.environ.get("MHH_LIB") or LIB_PATH      # tuning sweeps point this at a variant build of the SAME sources
        if path != LIB_PATH:
            _lib = bind(C.CDLL(path))
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not found: build it with `python -m microhh_amd.build` (needs hipcc); "
                              "microhh_amd has no CPU fallback" % LIB_PATH)
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def check(rc, library=None):
    if rc != 0:
        msg = (library or lib()).mhh_last_error()
        raise MhhError("mhh status %d: %s" % (rc, msg.decode() if msg else "?"))
