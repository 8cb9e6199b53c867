"""ctypes binding of the C-ABI shared library (include/fastmpc.h).

The library is built in-tree (`mpc-sensorlessao_amd/lib/libfastmpc.so`, see csrc/Makefile).  If it
is missing this module raises: there is no Python or CPU fallback for the solve path.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMPC_LIB") or os.path.join(_HERE, "lib", "libfastmpc.so")

FMPC_OK = 0
FMPC_W_LINESEARCH = 1
FMPC_E_NULL = -1
FMPC_E_DIM = -2
FMPC_E_UNSUPPORTED = -3
FMPC_E_NOT_PD_PHI = -4
FMPC_E_NOT_PD_SCHUR = -5
FMPC_E_HIP = -6
FMPC_E_ALLOC = -7
FMPC_E_NO_DEVICE = -8
# fmpc_last_dispatch paths
FMPC_PATH_GENERIC = 0
FMPC_PATH_WAVE = 1
FMPC_PATH_SHARED = 2
FMPC_PATH_PANEL = 3
FMPC_PATH_RAMP = 4
FMPC_PATH_TILED = 5
FMPC_PATH_TILED_F32 = 6
FMPC_PATH_RAMP_WS = 7
FMPC_PREC_F64 = 0
FMPC_PREC_F32_MIXED = 1
FMPC_MAX_REFINEMENT = 3
# fmpc_kkt_report*: fields of a report row, flag bits
FMPC_KKT_FIELDS = 6
FMPC_KKT_RD, FMPC_KKT_RP, FMPC_KKT_NR, FMPC_KKT_COST, FMPC_KKT_BARRIER, FMPC_KKT_MIN_SLACK = range(6)
FMPC_KKT_FIELD_NAMES = ("rd", "rp", "nr", "cost", "barrier", "min_slack")
FMPC_KKT_CONVERGED = 1
FMPC_KKT_INFEASIBLE = 2

# fmpc_est_refine_device: fields of an info row, status bits
FMPC_REFINE_FIELDS = 4
FMPC_REFINE_COST0, FMPC_REFINE_COST, FMPC_REFINE_STEP, FMPC_REFINE_ITERS = range(4)
FMPC_REFINE_FIELD_NAMES = ("cost0", "cost", "step", "iters")
FMPC_REFINE_CONVERGED = 1
FMPC_REFINE_FACTOR_FAILED = 2
FMPC_REFINE_BAD_INPUT = 4

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

# fmpc_noise: the noise block of fmpc_est_apply_noisy_device / fmpc_noise_normal_*
FMPC_NOISE_SIGMA = 0
FMPC_NOISE_SNR_MEASURED = 1


class Noise(C.Structure):
    _fields_ = [("mode", C.c_int), ("value", C.c_double), ("sigma_dev", _vp), ("seed", C.c_ulonglong), ("step", C.c_ulonglong),
                ("step_dev", _vp), ("first", C.c_longlong)]


# fmpc_detector: the block of fmpc_est_apply_detector_device / fmpc_detector_read_*
class Detector(C.Structure):
    _fields_ = [("gain", C.c_double), ("gain_dev", _vp), ("qe", C.c_double), ("background", C.c_double), ("read_noise", C.c_double),
                ("photon_noise", C.c_int), ("seed", C.c_ulonglong), ("step", C.c_ulonglong), ("step_dev", _vp), ("first", C.c_longlong)]


# name -> (restype, argtypes); every symbol include/fastmpc.h declares
SIGNATURES = {
    "fmpc_version": (C.c_int, []),
    "fmpc_strerror": (C.c_char_p, [C.c_int]),
    "fmpc_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 14 + [C.c_int]),
    "fmpc_destroy": (C.c_int, [_vp]),
    "fmpc_dims": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip]),
    "fmpc_solve": (C.c_int, [_vp, C.c_int] + [_vp] * 5 + [C.c_int, C.c_double] + [_vp] * 5),
    "fmpc_step_ld": (C.c_int, [C.c_int]),
    "fmpc_solve_device": (C.c_int, [_vp, C.c_int] + [_vp] * 5 + [C.c_int, C.c_double] + [_vp] * 5 + [_vp]),
    "fmpc_unpack": (C.c_int, [_vp, C.c_int] + [_vp] * 4),
    "fmpc_unpack_device": (C.c_int, [_vp, C.c_int] + [_vp] * 4 + [_vp]),
    "fmpc_solve_once": (C.c_int, [C.c_int] * 4 + [_vp] * 23 + [C.c_int, C.c_double, C.c_int, _vp, _vp]),
    "fmpc_solve_once_cache_clear": (C.c_int, []),
    "fmpc_last_dispatch": (C.c_int, [_vp, _ip, _ip]),
    "fmpc_set_dense_form": (C.c_int, [_vp, C.c_int, C.c_int]),
    "fmpc_last_dual_form": (C.c_int, [_vp]),
    "fmpc_last_tiled_wavefronts": (C.c_int, [_vp]),
    "fmpc_set_small_batch_kernel": (C.c_int, [_vp, C.c_int]),
    "fmpc_set_z_ld": (C.c_int, [_vp, C.c_int]),
    "fmpc_alloc_generation": (C.c_ulonglong, []),
    "fmpc_stretch_begin": (C.c_int, [_vp]),
    "fmpc_stretch_end": (C.c_int, [_vp]),
    "fmpc_last_stretch": (C.c_int, [_vp, _ip, _ip]),
    "fmpc_loop_inputs_device": (C.c_int, [_vp, C.c_int] + [_vp] * 7 + [_vp]),
    "fmpc_loop_step_device": (C.c_int, [_vp, C.c_int] + [_vp] * 8 + [C.c_int, C.c_double] + [_vp] * 6 + [_vp]),
    "fmpc_ao_step_device": (C.c_int, [_vp, C.c_int] + [_vp] * 6 + [C.c_int, C.c_double] + [_vp] * 6 + [_vp]),
    "fmpc_loop_run_device": (C.c_int, [_vp, C.c_int, C.c_int] + [_vp] * 4 + [C.c_int, C.c_int, C.c_double] + [_vp] * 7 + [_vp]),
    "fmpc_loop_records_device": (C.c_int, [_vp, C.c_int, C.c_int] + [_vp] * 4 + [C.c_longlong, C.c_int, _vp] + [C.c_double] * 3 + [_vp] * 5 + [_vp]),
    "fmpc_loop_records_run_device": (C.c_int, [_vp, C.c_int, C.c_int] + [_vp] * 5 + [C.c_double] * 3 + [_vp] * 4 + [_vp]),
    "fmpc_solve_u0_device": (C.c_int, [_vp, C.c_int] + [_vp] * 5 + [C.c_int, C.c_double] + [_vp] * 6 + [_vp]),
    "fmpc_solve_u0_device_ld": (C.c_int, [_vp, C.c_int] + [_vp] * 5 + [C.c_int, C.c_double] + [_vp] * 6 + [C.c_int, _vp]),
    "fmpc_solve_u0": (C.c_int, [_vp, C.c_int] + [_vp] * 5 + [C.c_int, C.c_double] + [_vp] * 4),
    "fmpc_set_ramp": (C.c_int, [_vp, _vp, _vp]),
    "fmpc_set_ramp_workspace": (C.c_int, [_vp, C.c_int]),
    "fmpc_set_precision": (C.c_int, [_vp, C.c_int]),
    "fmpc_set_refinement": (C.c_int, [_vp, C.c_int]),
    "fmpc_last_refinement": (C.c_int, [_vp]),
    "fmpc_var_identify_device": (C.c_int, [C.c_int] * 4 + [_vp] * 5),
    "fmpc_var_fit_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "fmpc_var_fit_device": (C.c_int, [C.c_int] * 5 + [_vp] * 5 + [C.c_size_t, _vp]),
    "fmpc_var_validate_device": (C.c_int, [C.c_int] * 6 + [_vp] * 6),
    "fmpc_solve_ramp": (C.c_int, [_vp, C.c_int] + [_vp] * 6 + [C.c_int, C.c_double] + [_vp] * 5),
    "fmpc_solve_ramp_device": (C.c_int, [_vp, C.c_int] + [_vp] * 6 + [C.c_int, C.c_double] + [_vp] * 5 + [_vp]),
    "fmpc_solve_ramp_u0_device": (C.c_int, [_vp, C.c_int] + [_vp] * 6 + [C.c_int, C.c_double] + [_vp] * 6 + [_vp]),
    "fmpc_bank_set_device": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    "fmpc_bank_count": (C.c_int, [_vp]),
    "fmpc_bank_release": (C.c_int, [_vp]),
    "fmpc_solve_bank_device": (C.c_int, [_vp, C.c_int, _vp] + [_vp] * 5 + [C.c_int, C.c_double] + [_vp] * 6 + [_vp]),
    "fmpc_loop_inputs_bank_device": (C.c_int, [_vp, C.c_int, _vp] + [_vp] * 7 + [_vp]),
    "fmpc_loop_records_bank_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int] + [_vp] * 4 + [C.c_longlong, C.c_int, _vp] + [C.c_double] * 3 + [_vp] * 5 + [_vp]),
    "fmpc_kkt_report_device": (C.c_int, [_vp, C.c_int] + [_vp] * 5 + [C.c_longlong, _vp, C.c_double, _vp, C.c_int, _vp, _vp]),
    "fmpc_kkt_report_bank_device": (C.c_int, [_vp, C.c_int, _vp] + [_vp] * 5 + [C.c_longlong, _vp, C.c_double, _vp, C.c_int, _vp, _vp]),
    "fmpc_kkt_report": (C.c_int, [_vp, C.c_int] + [_vp] * 5 + [C.c_longlong, _vp, C.c_double, _vp, C.c_int, _vp]),
    "fmpc_loop_records_run_bank_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp] + [_vp] * 5 + [C.c_double] * 3 + [_vp] * 4 + [_vp]),
    "fmpc_bank_prefactor_device": (C.c_int, [_vp, C.c_double, _vp]),
    "fmpc_bank_prefactor_count": (C.c_int, [_vp]),
    "fmpc_bank_prefactor_release": (C.c_int, [_vp]),
    "fmpc_last_bank_stored_factor": (C.c_int, [_vp]),
    "fmpc_bank_first_move_device": (C.c_int, [_vp, C.c_double, _vp]),
    "fmpc_bank_first_move_count": (C.c_int, [_vp]),
    "fmpc_bank_first_move_release": (C.c_int, [_vp]),
    "fmpc_last_bank_first_move": (C.c_int, [_vp]),
    "fmpc_loop_step_bank_device": (C.c_int, [_vp, C.c_int, _vp] + [_vp] * 8 + [C.c_int, C.c_double] + [_vp] * 6 + [_vp]),
    "fmpc_loop_run_bank_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp] + [_vp] * 4 + [C.c_int, C.c_int, C.c_double] + [_vp] * 7 + [_vp]),
    "fmpc_phase_residual_device": (C.c_int, [_vp, C.c_int, C.c_longlong] + [_vp] * 4 + [_vp]),
    "fmpc_est_create": (C.c_int, [C.POINTER(_vp)] + [C.c_int] * 4 + [_vp, _vp, C.c_double, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "fmpc_est_destroy": (C.c_int, [_vp]),
    "fmpc_est_dims": (C.c_int, [_vp] + [_ip] * 6),
    "fmpc_est_apply": (C.c_int, [_vp, C.c_int] + [_vp] * 4),
    "fmpc_est_apply_device": (C.c_int, [_vp, C.c_int] + [_vp] * 4 + [_vp]),
    "fmpc_est_apply_noisy_device": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(Noise), _vp, _vp, _vp, _vp]),
    "fmpc_noise_normal_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_longlong, C.POINTER(Noise), _vp]),
    "fmpc_noise_normal_host": (C.c_int, [_vp, C.c_int, C.c_int, C.c_longlong, C.POINTER(Noise)]),
    "fmpc_est_snr_sigma": (C.c_int, [_vp, C.c_double, _dp]),
    "fmpc_philox4x32_10": (C.c_int, [C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "fmpc_est_apply_detector_device": (C.c_int, [_vp, C.c_int, _vp, C.POINTER(Detector), _vp, _vp, _vp]),
    "fmpc_detector_read_device": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_longlong, C.POINTER(Detector), _vp]),
    "fmpc_detector_read_host": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_longlong, C.POINTER(Detector)]),
    "fmpc_est_photon_gain": (C.c_int, [_vp, C.c_double, _dp]),
    "fmpc_modal_workspace_bytes": (C.c_size_t, [C.c_int, C.c_longlong, C.c_int]),
    "fmpc_modal_factor_device": (C.c_int, [C.c_int, C.c_longlong, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "fmpc_modal_fit_device": (C.c_int, [C.c_int, C.c_longlong, C.c_int, _vp, _vp, _vp, C.c_longlong, C.c_int, _vp, C.c_int, _vp, C.c_size_t, _vp]),
    "fmpc_zernike_modes": (C.c_int, [C.c_int, _ip, _ip]),
    "fmpc_zernike_device": (C.c_int, [C.c_int, _ip, _ip, C.c_longlong, _vp, _vp, C.c_int, _vp, C.c_longlong, _vp]),
    "fmpc_zernike_grid_device": (C.c_int, [C.c_int, _ip, _ip, C.c_int, C.c_int, _vp, _vp]),
    "fmpc_est_optics_create": (C.c_int, [C.POINTER(_vp)] + [C.c_int] * 4 + [_vp, _vp, C.c_double, C.c_int]),
    "fmpc_est_optics_destroy": (C.c_int, [_vp]),
    "fmpc_est_model_workspace_bytes": (C.c_size_t, [_vp, C.c_int]),
    "fmpc_est_model_device": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "fmpc_est_create_from_model": (C.c_int, [C.POINTER(_vp), _vp, C.c_int, C.c_int, _vp, _vp]),
    "fmpc_est_refine_workspace_bytes": (C.c_size_t, [_vp, C.c_int, C.c_int]),
    "fmpc_est_refine_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_longlong, _vp, C.c_int, C.c_double, C.c_double, _vp, _vp, _vp,
                                         C.c_size_t, _vp]),
    "fmpc_est_refine_hold_workspace_bytes": (C.c_size_t, [_vp, C.c_int, C.c_int, C.c_int]),
    "fmpc_est_refine_hold_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_longlong, _vp, C.c_int, C.c_int, _vp, C.c_longlong,
                                              C.c_double, C.c_double, _vp, _vp, _vp, C.c_size_t, _vp]),
    "fmpc_est_refine_weighted_workspace_bytes": (C.c_size_t, [_vp, C.c_int, C.c_int, C.c_int]),
    "fmpc_est_refine_weighted_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_longlong, _vp, C.c_int, C.c_int, C.POINTER(Detector),
                                                  C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "fmpc_dm_influence_device": (C.c_int, [C.c_int] * 3 + [_vp] * 4 + [C.c_double] * 2 + [C.c_int] * 2 + [_vp, C.c_longlong, _vp]),
    "fmpc_dm_matrix_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "fmpc_dm_matrix_device": (C.c_int, [C.c_int] * 4 + [_vp] * 6 + [C.c_double] * 2 + [C.c_int, _vp, C.c_int, _vp, C.c_size_t, _vp]),
    "fmpc_dm_surface_device": (C.c_int, [C.c_int] * 4 + [_vp] * 4 + [C.c_double] * 2 + [_vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong, _vp]),
    "fmpc_dm_profile_oomao_host": (C.c_int, [C.c_double, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _ip]),
    "fmpc_dm_profile_eval_host": (C.c_int, [C.c_int, _vp, _vp, C.c_longlong, _vp, _vp]),
    "fmpc_dm_spline_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "fmpc_dm_spline_prepare_device": (C.c_int, [C.c_int] * 3 + [_vp] * 4 + [C.c_double, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp]),
    "fmpc_dm_spline_influence_device": (C.c_int, [C.c_int] * 3 + [_vp, C.c_int, C.c_int, _vp, C.c_longlong, _vp]),
    "fmpc_dm_spline_matrix_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "fmpc_dm_spline_matrix_device": (C.c_int, [C.c_int] * 4 + [_vp] * 3 + [C.c_int, _vp, C.c_int, _vp, C.c_size_t, _vp]),
    "fmpc_dm_spline_surface_device": (C.c_int, [C.c_int] * 4 + [_vp, _vp, C.c_longlong, _vp, C.c_longlong, _vp, C.c_longlong, C.c_uint, _vp]),
    "fmpc_atm_covariance_host": (C.c_int, [C.c_int, _vp, C.c_double, C.c_double, _vp]),
    "fmpc_atm_extruder_host": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp]),
    "fmpc_atm_displacement_host": (C.c_int, [C.c_longlong, C.c_double, C.POINTER(C.c_longlong), _dp]),
    "fmpc_atm_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, C.c_double, C.c_int, _vp,
                                  C.c_int, C.c_ulonglong, C.c_longlong, C.c_int]),
    "fmpc_atm_destroy": (C.c_int, [_vp]),
    "fmpc_atm_dims": (C.c_int, [_vp, _ip, _ip, _ip, _ip, C.POINTER(C.c_longlong)]),
    "fmpc_atm_reset_device": (C.c_int, [_vp, _vp]),
    "fmpc_atm_advance_device": (C.c_int, [_vp, C.c_longlong, _vp]),
    "fmpc_atm_screen_device": (C.c_int, [_vp, C.c_int, _vp, C.c_double, _vp, _vp]),
    "fmpc_atm_get_state": (C.c_int, [_vp, _vp, C.POINTER(C.c_longlong), _vp, _vp]),
    "fmpc_atm_set_state": (C.c_int, [_vp, _vp, C.c_longlong, _vp, _vp]),
    "fmpc_sci_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_double, _vp, C.c_double, C.c_int]),
    "fmpc_sci_destroy": (C.c_int, [_vp]),
    "fmpc_sci_dims": (C.c_int, [_vp, _ip, _ip, _dp, _dp, _dp, _dp]),
    "fmpc_sci_workspace_bytes": (C.c_size_t, [_vp, C.c_int]),
    "fmpc_sci_expose_device": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_longlong, _vp, C.c_size_t, _vp]),
    "fmpc_sci_last_form": (C.c_int, [_vp]),
    "fmpc_sci_summary_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
    "fmpc_sci_tables_host": (C.c_int, [C.c_int, C.c_int, C.c_double, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    "fmpc_sh_valid_host": (C.c_int, [C.c_int, C.c_int, _vp, C.c_double, _vp, _ip]),
    "fmpc_sh_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_double, C.c_double, C.c_int]),
    "fmpc_sh_destroy": (C.c_int, [_vp]),
    "fmpc_sh_dims": (C.c_int, [_vp] + [_ip] * 7),
    "fmpc_sh_set_threshold": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double]),
    "fmpc_sh_set_reference_device": (C.c_int, [_vp, _vp, C.c_double, _vp]),
    "fmpc_sh_set_reconstructor_device": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "fmpc_sh_measure_device": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "fmpc_sh_slopes_device": (C.c_int, [_vp, C.c_int, _vp, C.c_longlong, _vp, _vp, _vp, _vp]),
}

_lib = None


class FastMPCError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = int(code)
        msg = strerror(code)
        super().__init__(f"{where}: [{self.code}] {msg}" if where else f"[{self.code}] {msg}")


def load():
    """Load the shared library once; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(`python -c 'import __graft_entry__ as g; g.build()'` or `make -C mpc-sensorlessao_amd/csrc`). "
            "This package has no CPU fallback.")
    # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so).  Whichever runtime is loaded FIRST serves the
    # process: with this library first (it resolves /opt/rocm's), a later `import torch` brings a second runtime and the
    # library's hipGetDeviceCount then finds no device.  Let torch, when installed, go first; plain C / ctypes clients
    # without torch are unaffected.
    # FMPC_NO_TORCH_PRELOAD=1 opts out (a plain ctypes / numpy client that never imports torch saves its import time and
    # keeps /opt/rocm's runtime); a torch that fails to import is reported, not hidden.
    if "torch" not in sys.modules and os.environ.get("FMPC_NO_TORCH_PRELOAD", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass                                           # no torch installed: nothing to order
        except Exception as e:                             # a broken install: say so, the library may then see no device
            import warnings
            warnings.warn(f"mpc-sensorlessao_amd: `import torch` failed ({e!r}); loading {LIB_PATH} with the system HIP runtime. "
                          "If a later torch import brings its own runtime the library will report FMPC_E_NO_DEVICE.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def strerror(code):
    try:
        return load().fmpc_strerror(int(code)).decode()
    except Exception:   # library absent: still give the number
        return f"fastmpc status {code}"
