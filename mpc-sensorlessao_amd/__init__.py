"""MI355X-native fastMPC inner solver behind the `Fast_MPC2` interface of
jinsungkim96/MPC-SensorlessAO (Fast_MPC/VAR_2/Fast_MPC2.m).  The compute path is the HIP library
behind include/fastmpc.h; nothing here solves on the CPU."""
from ._lib import (FastMPCError, FMPC_OK, FMPC_W_LINESEARCH, FMPC_E_NULL, FMPC_E_DIM,
                   FMPC_E_UNSUPPORTED, FMPC_E_NOT_PD_PHI, FMPC_E_NOT_PD_SCHUR, FMPC_E_HIP,
                   FMPC_E_ALLOC, FMPC_E_NO_DEVICE, FMPC_PATH_GENERIC, FMPC_PATH_WAVE, FMPC_PATH_SHARED,
                   FMPC_PATH_PANEL, FMPC_PATH_RAMP, FMPC_PATH_RAMP_WS, LIB_PATH, load,
                   FMPC_KKT_FIELDS, FMPC_KKT_RD, FMPC_KKT_RP, FMPC_KKT_NR, FMPC_KKT_COST, FMPC_KKT_BARRIER,
                   FMPC_KKT_MIN_SLACK, FMPC_KKT_FIELD_NAMES, FMPC_KKT_CONVERGED, FMPC_KKT_INFEASIBLE)
from .handle import FastMPCHandle
from .fast_mpc2 import Fast_MPC2, Fast_MPC2_VAR1, deinterleave
from . import synthetic
from .sharded import ShardedFastMPC, shard_range
from .closed_loop import ClosedLoop, AOLoop
from .lanes import SolveLanes
from .records import LoopRecords
from .recorded import RecordedSolves
from .var_identify import identify_var2_device, identify_var_device, validate_var_device, var_fit_workspace_bytes
from .estimator import PhaseDiversityEstimator, EstimatorNoise, normal_noise, normal_noise_host, DetectorNoise, detector_read, detector_read_host
from .modal import ModalFit, modal_workspace_bytes
from .dm import GaussianDM, dm_matrix_workspace_bytes, reference_dm_geometry, reference_dm
from .dm_spline import (DMProfile, SplineDM, oomao_profile, oomao_dm_geometry, oomao_dm, dm_spline_matrix_workspace_bytes, FMPC_DM_TILE,
                        FMPC_DM_DENSE)
from .atmosphere import Atmosphere, reference_atmosphere, atm_covariance, atm_extruder, atm_displacement, atm_default_stencil
from . import optics
from .optics import zernike_modes, zernike_basis, zernike_grid, EstimatorOptics, reference_optics, reference_pupil, reference_science_camera
from ._lib import (FMPC_REFINE_FIELDS, FMPC_REFINE_COST0, FMPC_REFINE_COST, FMPC_REFINE_STEP, FMPC_REFINE_ITERS, FMPC_REFINE_FIELD_NAMES,
                   FMPC_REFINE_CONVERGED, FMPC_REFINE_FACTOR_FAILED, FMPC_REFINE_BAD_INPUT)
from . import science
from .science import (ScienceCamera, sci_tables_host, FMPC_SCI_FIELDS, FMPC_SCI_MEAN, FMPC_SCI_RMS, FMPC_SCI_STREHL, FMPC_SCI_MARECHAL,
                      FMPC_SCI_MIN, FMPC_SCI_MAX, FMPC_SCI_FIELD_NAMES, FMPC_SCI_FORM_STANDARD, FMPC_SCI_FORM_FEW)
from . import shwfs
from .shwfs import ShackHartmann, sh_valid_host, FMPC_SH_THRESHOLD_NONE, FMPC_SH_THRESHOLD_FLOOR, FMPC_SH_THRESHOLD_FRACTION
from . import _lib

__all__ = ["optics", "zernike_modes", "zernike_basis", "zernike_grid", "EstimatorOptics", "reference_optics","FastMPCHandle", "Fast_MPC2", "Fast_MPC2_VAR1", "deinterleave", "FastMPCError",
           "ShardedFastMPC", "shard_range", "ClosedLoop", "AOLoop", "SolveLanes", "RecordedSolves", "PhaseDiversityEstimator", "synthetic", "load", "LIB_PATH",
           "identify_var2_device", "identify_var_device", "validate_var_device", "var_fit_workspace_bytes", "LoopRecords",
           "FMPC_KKT_FIELDS", "FMPC_KKT_RD", "FMPC_KKT_RP", "FMPC_KKT_NR", "FMPC_KKT_COST", "FMPC_KKT_BARRIER", "FMPC_KKT_MIN_SLACK",
           "FMPC_KKT_FIELD_NAMES", "FMPC_KKT_CONVERGED", "FMPC_KKT_INFEASIBLE", "ModalFit", "modal_workspace_bytes",
           "EstimatorNoise", "normal_noise", "normal_noise_host", "DetectorNoise", "detector_read", "detector_read_host", "GaussianDM", "dm_matrix_workspace_bytes", "reference_dm_geometry",
           "reference_dm", "science", "ScienceCamera", "sci_tables_host", "reference_pupil", "reference_science_camera", "FMPC_SCI_FIELDS", "FMPC_SCI_MEAN",
           "FMPC_SCI_RMS", "FMPC_SCI_STREHL", "FMPC_SCI_MARECHAL", "FMPC_SCI_MIN", "FMPC_SCI_MAX", "FMPC_SCI_FIELD_NAMES", "FMPC_SCI_FORM_STANDARD",
           "FMPC_SCI_FORM_FEW", "Atmosphere", "reference_atmosphere", "atm_covariance", "atm_extruder", "atm_displacement", "atm_default_stencil",
           "shwfs", "ShackHartmann", "sh_valid_host", "FMPC_SH_THRESHOLD_NONE", "FMPC_SH_THRESHOLD_FLOOR", "FMPC_SH_THRESHOLD_FRACTION",
           "DMProfile", "SplineDM", "oomao_profile", "oomao_dm_geometry", "oomao_dm", "dm_spline_matrix_workspace_bytes", "FMPC_DM_TILE",
           "FMPC_DM_DENSE", "FMPC_REFINE_FIELDS", "FMPC_REFINE_COST0", "FMPC_REFINE_COST", "FMPC_REFINE_STEP", "FMPC_REFINE_ITERS",
           "FMPC_REFINE_FIELD_NAMES", "FMPC_REFINE_CONVERGED", "FMPC_REFINE_FACTOR_FAILED", "FMPC_REFINE_BAD_INPUT"]
