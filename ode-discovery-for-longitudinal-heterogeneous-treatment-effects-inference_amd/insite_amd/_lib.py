"""ctypes binding of ``libinsite_hip.so`` (the C ABI declared in ``include/insite_hip.h``).

The product path has no CPU fallback: if the shared library is missing or cannot be loaded
every op raises ``InsiteLibraryError``.  ``torch`` is imported first so that the library binds
to the HIP runtime torch already loaded (same soname ``libamdhip64.so.7``) and torch stream
handles are valid across the ABI.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must precede the dlopen below: shared HIP runtime)

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(PKG_ROOT, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libinsite_hip.so")
# profiling-only override (ablation builds under tools/); never set in product runs
if os.environ.get("INSITE_LIB_OVERRIDE"):
    LIB_PATH = os.environ["INSITE_LIB_OVERRIDE"]

ABI_VERSION = 9

# status codes / enums (insite_hip.h)
INSITE_OK = 0
INSITE_E_UNSUPPORTED = -2   # include/insite_hip.h
FD_SMOOTHED4, FD_ORDER4, FD_ORDER1, FD_SMOOTHED1 = 0, 1, 2, 3
FD_NONUNIFORM2, FD_NONUNIFORM4 = 4, 5   # include/insite_irregular.h
IRREGULAR_ABI_VERSION = 1
WEAK_ABI_VERSION, WEAK_MAX_K = 1, 1024     # include/insite_weak.h
OPT_SR3, OPT_STLSQ = 0, 1
BOOTSTRAP_ABI_VERSION, BOOT_MAX_REPLICATES = 1, 16384   # include/insite_bootstrap.h
EFFECT_ABI_VERSION, EFFECT_MAX_REPLICATES, EFFECT_MAX_QUANTILES = 1, 512, 16   # include/insite_effect.h
# include/insite_cohort.h
COHORT_ABI_VERSION, COHORT_MAX_REPLICATES, COHORT_MAX_GROUPS, COHORT_MAX_QUANTILES = 1, 4096, 64, 16
COHORT_WEIGHT_NONE, COHORT_WEIGHT_POISSON = 0, 1
# include/insite_regimen.h
REGIMEN_ABI_VERSION, REGIMEN_MAX_REPLICATES, REGIMEN_MAX_QUANTILES, REGIMEN_MAX_PLANS = 1, 512, 16, 16
REGIMEN_MINIMIZE, REGIMEN_MAXIMIZE = 1, -1
# include/insite_policy.h
POLICY_ABI_VERSION, POLICY_MAX_REPLICATES, POLICY_MAX_PLANS, POLICY_MAX_GROUPS, POLICY_MAX_QUANTILES = 1, 4096, 16, 64, 16
# include/insite_feedback.h
FEEDBACK_ABI_VERSION, FEEDBACK_MAX_REPLICATES, FEEDBACK_MAX_QUANTILES, FEEDBACK_MAX_RULES = 1, 512, 16, 16
FEEDBACK_MINIMIZE, FEEDBACK_MAXIMIZE = 1, -1
# include/insite_rulevalue.h
RULEVALUE_ABI_VERSION = 1
RULEVALUE_MAX_REPLICATES, RULEVALUE_MAX_RULES, RULEVALUE_MAX_GROUPS, RULEVALUE_MAX_QUANTILES = 4096, 16, 64, 16
SEGBOOT_ABI_VERSION = 1   # include/insite_segboot.h
# include/insite_score.h
SCORE_ABI_VERSION, SCORE_MAX_REPLICATES, SCORE_MAX_LEVELS, SCORE_MAX_BINS, SCORE_MAX_GROUPS = 1, 512, 8, 32, 64
METHOD_EULER, METHOD_RK4 = 0, 1
LAYOUT_PATIENT_MAJOR, LAYOUT_TIME_MAJOR, LAYOUT_TIME_MAJOR_BITS, LAYOUT_PATIENT_MAJOR_BITS = 0, 1, 2, 3
MAX_TERMS, MAX_STATICS, MAX_ARMS, MAX_STATE_DEGREE = 9, 3, 4, 1
GEN_MAX_TERMS, GEN_MAX_STATE_DEGREE, GEN_MAX_INPUTS = 64, 4, 2   # insite_gen.hip

EXPORTS = (
    "insite_abi_version",
    "insite_strerror",
    "insite_poly_library",
    "insite_gram_workspace_bytes",
    "insite_gram_f64",
    "insite_sindy_fit_f64",
    "insite_fit_rollout_f64",
    "insite_fit_rollout_deferred_workspace_bytes",
    "insite_fit_rollout_deferred_f64",
    "insite_fit_rollout_lagged_f64",
    "insite_gram_segments_workspace_bytes",
    "insite_gram_segments_f64",
    "insite_sindy_fit_segments_f64",
    "insite_per_patient_workspace_bytes",
    "insite_sindy_fit_per_patient_f64",
    "insite_gram_moments_f64",
    "insite_fit_per_patient_moments_f64",
    "insite_stlsq_f64",
    "insite_rollout_f64",
    "insite_rollout_rk45_f64",
    "insite_rk45_order_workspace_bytes",
    "insite_rk45_order_i32",
    "insite_refine_f64",
    "insite_refine_arms_f64",
    "insite_refine_general_f64",
    "insite_refine_rows_f64",
    "insite_refine_prepare_f64",
    "insite_refine_finish_f64",
    "insite_gen_gram_segments_workspace_bytes",
    "insite_gen_gram_segments_f64",
    "insite_masked_sse_workspace_bytes",
    "insite_masked_sse_f64",
    "insite_gram_ms_workspace_bytes",
    "insite_gram_ms_f32",
    "insite_stlsq_wave_f64",
    "insite_rollout_ms_f32",
    "insite_rollout_ms_sparse_f32",
    "insite_gen_gram_workspace_bytes",
    "insite_gen_gram_f64",
    "insite_stlsq_wave64_f64",
    "insite_rollout_poly_f64",
    "insite_threefry2x32_iota_u32",
    "insite_refit_rollout_moments_f64",
)

# the extension header include/insite_irregular.h (same shared library, its own ABI version)
EXT_EXPORTS = (
    "insite_irregular_abi_version",
    "insite_gram_irregular_workspace_bytes",
    "insite_gram_irregular_f64",
    "insite_sindy_fit_irregular_f64",
)

# the extension header include/insite_weak.h (same shared library, its own ABI version; a list of its own:
# EXT_EXPORTS is pinned to insite_irregular.h's functions by tests/test_irregular_oracle.py)
WEAK_EXPORTS = (
    "insite_weak_abi_version",
    "insite_gram_weak_workspace_bytes",
    "insite_gram_weak_f64",
    "insite_sr3_f64",
    "insite_sindy_fit_weak_f64",
)

# the extension header include/insite_bootstrap.h (same shared library, its own ABI version; a list of its own:
# EXT_EXPORTS and WEAK_EXPORTS are pinned by tests/test_irregular_oracle.py and tests/test_weak_abi.py)
BOOT_EXPORTS = (
    "insite_bootstrap_abi_version",
    "insite_bootstrap_workspace_bytes",
    "insite_bootstrap_gram_f64",
    "insite_sindy_bootstrap_f64",
)

# the extension header include/insite_effect.h (same shared library, its own ABI version; a list of its own:
# the four lists above are pinned by tests)
EFFECT_EXPORTS = (
    "insite_effect_abi_version",
    "insite_effect_workspace_bytes",
    "insite_effect_bands_f64",
)

# the extension header include/insite_cohort.h (same shared library, its own ABI version; a list of its own:
# the five lists above are pinned by tests)
COHORT_EXPORTS = (
    "insite_cohort_abi_version",
    "insite_cohort_effect_workspace_bytes",
    "insite_cohort_effect_sums_f64",
    "insite_cohort_effect_finalize_f64",
    "insite_cohort_effect_f64",
)

# the extension header include/insite_regimen.h (same shared library, its own ABI version; a list of its own:
# the six lists above are pinned by tests)
REGIMEN_EXPORTS = (
    "insite_regimen_abi_version",
    "insite_regimen_workspace_bytes",
    "insite_regimen_choice_f64",
)

# the extension header include/insite_policy.h (same shared library, its own ABI version; a list of its own:
# the seven lists above are pinned by tests)
POLICY_EXPORTS = (
    "insite_policy_abi_version",
    "insite_policy_workspace_bytes",
    "insite_policy_sums_f64",
    "insite_policy_finalize_f64",
    "insite_policy_value_f64",
)

# the extension header include/insite_feedback.h (same shared library, its own ABI version).  Not named *_EXPORTS:
# tests/test_workspace_matrix.py pins the set of names with that ending, and this entry point takes no workspace
FEEDBACK_SYMBOLS = (
    "insite_feedback_abi_version",
    "insite_feedback_rules_f64",
)

# the extension header include/insite_rulevalue.h (same shared library, its own ABI version).  Not named *_EXPORTS
# either: tests/test_workspace_matrix.py pins the set of names with that ending.  The sums and the fused call take a
# workspace, but before their outputs (the header says why)
RULEVALUE_SYMBOLS = (
    "insite_rulevalue_abi_version",
    "insite_rulevalue_workspace_bytes",
    "insite_rulevalue_sums_f64",
    "insite_rulevalue_finalize_f64",
    "insite_rulevalue_f64",
)

# the extension header include/insite_segboot.h (same shared library, its own ABI version).  Not named *_EXPORTS
# either; the Gram and the fit take a workspace before their outputs, the moments pass takes none
SEGBOOT_SYMBOLS = (
    "insite_segboot_abi_version",
    "insite_segboot_moments_f64",
    "insite_segboot_workspace_bytes",
    "insite_segboot_gram_f64",
    "insite_segboot_fit_f64",
)

# the extension header include/insite_score.h (same shared library, its own ABI version).  Not named *_EXPORTS
# either; the sums call takes a workspace before its output (the header says why)
SCORE_SYMBOLS = (
    "insite_score_abi_version",
    "insite_score_workspace_bytes",
    "insite_score_sums_f64",
)


class InsiteLibraryError(RuntimeError):
    pass


class InsiteError(RuntimeError):
    def __init__(self, fn, code, msg):
        super().__init__(f"{fn} failed with status {code}: {msg}")
        self.code = code


_lock = threading.Lock()
_lib = None

_c_i32, _c_i64, _c_f64, _c_size, _vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t, ctypes.c_void_p

_SIGNATURES = {
    "insite_abi_version": (_c_i32, []),
    "insite_strerror": (ctypes.c_char_p, [_c_i32]),
    "insite_poly_library": (_c_i32, [_c_i32, _c_i32, _c_i32, _vp, _c_i32, ctypes.POINTER(_c_i32)]),
    "insite_gram_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32]),
    "insite_gram_f64": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _vp, _c_i32,
                                 _c_i32, _c_f64, _vp, _vp, _vp, _c_size, _vp]),
    "insite_sindy_fit_f64": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _vp,
                                      _c_i32, _c_i32,
                                      _c_f64, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp, _vp, _vp, _vp, _c_size,
                                      _vp]),
    "insite_fit_rollout_f64": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _vp, _c_i32,
                                        _c_i32, _c_f64, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i32, _c_f64, _c_i32, _c_i32, _c_f64,
                                        _vp, _c_i64, _c_i32, _vp, _c_size, _vp]),
    "insite_fit_rollout_deferred_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32]),
    "insite_fit_rollout_deferred_f64": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _vp,
                                                 _c_i32, _c_i32, _c_f64, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp,
                                                 _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i32, _c_f64, _c_i32,
                                                 _c_i32, _c_f64, _vp, _c_i64, _c_i32, _c_i32, _c_i32, _vp, _c_size,
                                                 _vp]),
    "insite_fit_rollout_lagged_f64": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _vp,
                                               _c_i32, _c_i32, _c_f64, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i32, _c_f64,
                                               _c_i32, _c_i32, _c_f64, _vp, _c_i64, _c_i32, _c_i32, _c_i32, _vp,
                                               _c_size, _vp]),
    "insite_gram_segments_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32]),
    "insite_gram_segments_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_i64, _c_i32, _c_i32,
                                          _vp, _c_i32, _c_i32, _c_f64, _vp, _vp, _vp, _c_size, _vp]),
    "insite_sindy_fit_segments_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_i64, _c_i32,
                                               _c_i32, _vp, _c_i32, _c_i32, _c_f64, _c_f64, _c_f64, _c_i32, _c_i32,
                                               _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "insite_per_patient_workspace_bytes": (_c_size, [_c_i64]),
    "insite_sindy_fit_per_patient_f64": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32,
                                                  _vp, _c_i32, _c_i32, _c_f64, _vp, _c_f64, _c_f64, _c_i32, _c_i32,
                                                  _vp, _vp, _vp, _vp, _c_size, _vp]),
    "insite_gram_moments_f64": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _vp,
                                         _c_i32, _c_i32, _c_f64, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _c_size, _vp]),
    "insite_fit_per_patient_moments_f64": (_c_i32, [_vp, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _c_i32, _vp, _c_i32,
                                                    _vp, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp, _vp]),
    "insite_stlsq_f64": (_c_i32, [_vp, _vp, _c_i64, _c_i32, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp, _vp]),
    "insite_rollout_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _c_i32, _c_i64, _c_i32, _c_i32,
                                    _c_i32, _c_f64, _c_i32, _c_i32, _c_f64, _vp, _c_i64, _c_i32, _vp]),
    "insite_rollout_rk45_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i64, _vp, _c_i32, _c_i64,
                                         _c_i32, _c_i32, _c_i32, _c_f64, _c_f64, _c_f64, _vp, _c_i64, _vp, _vp,
                                         _c_i32, _vp]),
    "insite_rk45_order_workspace_bytes": (_c_size, [_c_i32]),
    "insite_rk45_order_i32": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _vp, _c_size, _vp]),
    "insite_refine_f64": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _c_i64, _vp, _vp, _c_i64, _c_i32, _vp, _c_i32, _vp,
                                   _c_i32, _c_f64, _c_f64, _c_i32, _c_i32, _c_i32, _vp, _c_i64, _vp, _vp, _vp, _vp,
                                   _vp]),
    "insite_refine_arms_f64": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _c_i64, _vp, _vp, _c_i64, _c_i32, _vp, _c_i32,
                                        _vp, _c_i32, _c_f64, _c_f64, _c_i32, _c_i32, _c_i32, _vp, _c_i64, _vp, _vp, _vp,
                                        _vp, _vp]),
    "insite_refine_general_f64": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i32, _c_i32,
                                           _vp, _vp, _vp, _c_i32, _c_f64, _c_f64, _c_i32, _c_i32, _c_i32, _vp, _c_i64,
                                           _vp, _vp, _vp, _vp, _vp, _vp]),
    "insite_refine_rows_f64": (_c_i32, [_vp, _c_i64, _c_i32, _vp, _c_i64, _vp, _vp, _c_i64, _c_i32, _c_i32, _vp,
                                        _vp, _vp, _c_i32, _c_f64, _c_f64, _c_i32, _c_i32, _c_i32, _vp, _c_i64, _vp,
                                        _vp, _vp, _vp, _vp, _vp]),
    "insite_refine_prepare_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i64, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp,
                                           _c_i64, _vp, _vp, _c_i32, _vp, _vp, _vp, _vp]),
    "insite_refine_finish_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _vp, _c_i64, _vp, _c_i32, _vp, _vp, _vp,
                                          _vp, _vp, _vp]),
    "insite_gen_gram_segments_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32]),
    "insite_gen_gram_segments_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_i32, _c_i64,
                                              _c_i32, _vp, _c_i32, _c_i32, _c_f64, _vp, _vp, _vp, _c_size, _vp]),
    "insite_refit_rollout_moments_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _c_i32, _vp, _c_i32, _vp,
                                                  _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp, _c_i64, _c_i32,
                                                  _c_f64, _c_i32, _c_i32, _c_f64, _vp, _c_i64, _vp, _vp, _vp, _vp]),
    "insite_threefry2x32_iota_u32": (_c_i32, [ctypes.c_uint32, ctypes.c_uint32, _c_i64, _vp, _vp]),
    "insite_masked_sse_workspace_bytes": (_c_size, [_c_i64, _c_i32]),
    "insite_masked_sse_f64": (_c_i32, [_vp, _c_i64, _c_f64, _c_f64, _vp, _vp, _c_i64, _c_i32, _vp, _vp, _vp,
                                       _vp, _c_size, _vp]),
    "insite_gram_ms_workspace_bytes": (_c_size, [_c_i64]),
    "insite_gram_ms_f32": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp, _c_i32, _c_i32,
                                    _c_f64, _vp, _vp, _vp, _c_size, _vp]),
    "insite_stlsq_wave_f64": (_c_i32, [_vp, _vp, _c_i32, _c_i32, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp,
                                       _vp]),
    "insite_rollout_ms_f32": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i32, _c_i32, _c_i64, _c_i32, _c_f64,
                                       _c_i32, _c_i32, _c_f64, _vp, _c_i64, _vp]),
    "insite_rollout_ms_sparse_f32": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _c_i32, _c_i32, _c_i64, _c_i32,
                                              _c_f64, _c_i32, _c_i32, _c_f64, _vp, _c_i64, _vp]),
    "insite_gen_gram_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32]),
    "insite_gen_gram_f64": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _c_i32, _vp, _c_i64, _c_i32, _vp, _c_i32, _vp,
                                     _c_i64, _vp, _c_i32, _c_i32, _c_f64, _vp, _vp, _vp, _c_size, _vp]),
    "insite_stlsq_wave64_f64": (_c_i32, [_vp, _vp, _c_i64, _c_i32, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp,
                                         _vp]),
    "insite_rollout_poly_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _c_i32, _c_i64, _c_i32, _c_i32,
                                         _c_i32, _c_f64, _c_i32, _c_i32, _c_f64, _vp, _c_i64, _c_i32, _vp]),
    # insite_irregular.h
    "insite_irregular_abi_version": (_c_i32, []),
    "insite_gram_irregular_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32]),
    "insite_gram_irregular_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32, _c_i32,
                                           _vp, _c_i32, _c_i32, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "insite_sindy_fit_irregular_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i32, _c_i32,
                                                _c_i32, _vp, _c_i32, _c_i32, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp,
                                                _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    # insite_weak.h
    "insite_weak_abi_version": (_c_i32, []),
    "insite_gram_weak_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32]),
    "insite_gram_weak_f64": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_i64, _c_i32, _vp, _vp, _vp, _c_i64,
                                      _c_i32, _c_i32, _vp, _c_i32, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "insite_sr3_f64": (_c_i32, [_vp, _vp, _c_i64, _c_i32, _c_f64, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _vp, _vp,
                                _vp]),
    "insite_sindy_fit_weak_f64": (_c_i32, [_vp, _c_i64, _c_i32, _c_i32, _vp, _vp, _c_i64, _c_i32, _vp, _vp, _vp,
                                           _c_i64, _c_i32, _c_i32, _vp, _c_i32, _c_i32, _c_f64, _c_f64, _c_f64,
                                           _c_f64, _c_i32, _c_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    # insite_bootstrap.h
    "insite_bootstrap_abi_version": (_c_i32, []),
    "insite_bootstrap_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32]),
    "insite_bootstrap_gram_f64": (_c_i32, [_vp, _vp, _vp, _vp, _c_i32, _c_i64, _c_i64, _c_i32, _c_i32, _vp, _c_i32,
                                           _c_i32, ctypes.c_uint32, _vp, _vp, _vp, _c_size, _vp]),
    "insite_sindy_bootstrap_f64": (_c_i32, [_vp, _vp, _vp, _vp, _c_i32, _c_i64, _c_i64, _c_i32, _c_i32, _vp, _c_i32,
                                            _c_i32, ctypes.c_uint32, _c_i32, _c_f64, _c_f64, _c_f64, _c_f64, _c_i32,
                                            _c_i32, _vp, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    # insite_effect.h
    "insite_effect_abi_version": (_c_i32, []),
    "insite_effect_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32]),
    "insite_effect_bands_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i32, _c_i64, _c_i32, _c_i32,
                                         _c_i32, _c_f64, _c_i32, _c_i32, _c_f64, _c_i32, _vp, _c_i32, _vp, _c_i64,
                                         _vp, _c_size, _vp]),
    # insite_cohort.h
    "insite_cohort_abi_version": (_c_i32, []),
    "insite_cohort_effect_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32]),
    "insite_cohort_effect_sums_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i32, _c_i64, _c_i32,
                                               _c_i32, _c_i32, _c_f64, _c_i32, _c_i32, _c_f64, _c_i32, _vp, _c_i32,
                                               _c_i32, ctypes.c_uint32, _c_i64, _vp, _c_i64, _vp, _vp, _c_size, _vp]),
    "insite_cohort_effect_finalize_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i32, _c_i32, _c_i32, _c_i32, _vp, _c_i32, _vp,
                                                   _c_i64, _vp]),
    "insite_cohort_effect_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _vp, _c_i32, _c_i64, _c_i32, _c_i32,
                                          _c_i32, _c_f64, _c_i32, _c_i32, _c_f64, _c_i32, _vp, _c_i32, _c_i32,
                                          ctypes.c_uint32, _c_i64, _vp, _c_i64, _vp, _vp, _c_i32, _vp, _c_i64, _vp,
                                          _c_size, _vp]),
    # insite_regimen.h
    "insite_regimen_abi_version": (_c_i32, []),
    "insite_regimen_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32]),
    "insite_regimen_choice_f64": (_c_i32, [_vp, _vp, _vp, _c_i32, _c_i64, _c_i64, _vp, _c_i64, _vp, _c_i32, _vp, _vp,
                                           _c_i32, _c_i64, _c_i32, _c_i32, _c_i32, _c_f64, _c_i32, _c_i32, _c_f64,
                                           _c_i32, _vp, _c_i32, _vp, _vp, _vp, _c_i64, _vp, _c_size, _vp]),
    # insite_policy.h
    "insite_policy_abi_version": (_c_i32, []),
    "insite_policy_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32]),
    "insite_policy_sums_f64": (_c_i32, [_vp, _vp, _vp, _c_i32, _c_i64, _c_i64, _vp, _c_i64, _vp, _c_i32, _vp, _vp, _c_i32, _c_i64,
                                        _c_i32, _c_i32, _c_i32, _c_f64, _c_i32, _c_i32, _c_f64, _c_i32, _vp, _c_i32,
                                        _c_i32, ctypes.c_uint32, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_size, _vp]),
    "insite_policy_finalize_f64": (_c_i32, [_vp, _vp, _c_i32, _c_i32, _c_i32, _c_i32, _vp, _c_i32, _vp, _c_i64, _vp,
                                            _vp, _vp]),
    "insite_policy_value_f64": (_c_i32, [_vp, _vp, _vp, _c_i32, _c_i64, _c_i64, _vp, _c_i64, _vp, _c_i32, _vp, _vp, _c_i32, _c_i64,
                                        _c_i32, _c_i32, _c_i32, _c_f64, _c_i32, _c_i32, _c_f64, _c_i32, _vp, _c_i32,
                                        _c_i32, ctypes.c_uint32, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_i32, _vp, _c_i64, _vp, _vp, _vp, _c_size, _vp]),
    # insite_feedback.h
    "insite_feedback_abi_version": (_c_i32, []),
    "insite_feedback_rules_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i32, _vp, _c_i64, _vp, _vp, _c_i32, _vp, _vp,
                                           _c_i32, _c_i64, _c_i32, _c_i32, _c_i32, _c_f64, _c_i32, _c_i32, _c_f64,
                                           _c_i32, _vp, _c_i32, _vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp]),
    # insite_rulevalue.h
    "insite_rulevalue_abi_version": (_c_i32, []),
    "insite_rulevalue_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32]),
    "insite_rulevalue_sums_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i32, _vp, _c_i64, _vp, _vp, _c_i32, _vp, _vp,
                                           _c_i32, _c_i64, _c_i32, _c_i32, _c_i32, _c_f64, _c_i32, _c_i32, _c_f64,
                                           _c_i32, _vp, _c_i32, _c_i32, ctypes.c_uint32, _c_i64, _vp, _vp, _vp, _c_size,
                                           _vp, _vp, _vp]),
    "insite_rulevalue_finalize_f64": (_c_i32, [_vp, _vp, _c_i32, _c_i32, _c_i32, _c_i32, _vp, _c_i32, _vp, _c_i64,
                                               _vp, _vp, _vp]),
    "insite_rulevalue_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _c_i32, _vp, _c_i64, _vp, _vp, _c_i32, _vp, _vp,
                                           _c_i32, _c_i64, _c_i32, _c_i32, _c_i32, _c_f64, _c_i32, _c_i32, _c_f64,
                                           _c_i32, _vp, _c_i32, _c_i32, ctypes.c_uint32, _c_i64, _vp, _vp, _vp, _c_size,
                                           _vp, _vp, _vp, _c_i32, _vp, _c_i64, _vp, _vp, _vp]),
    # insite_segboot.h
    "insite_segboot_abi_version": (_c_i32, []),
    "insite_segboot_moments_f64": (_c_i32, [_vp, _c_i64, _vp, _c_i64, _c_i32, _c_i32, _vp, _c_i64, _c_i32, _c_i32,
                                            _c_f64, _vp, _vp]),
    "insite_segboot_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32]),
    "insite_segboot_gram_f64": (_c_i32, [_vp, _vp, _c_i64, _c_i64, _c_i32, _c_i32, _vp, _c_i32, _c_i32,
                                         ctypes.c_uint32, _vp, _c_size, _vp, _vp, _vp]),
    "insite_segboot_fit_f64": (_c_i32, [_vp, _vp, _c_i64, _c_i64, _c_i32, _c_i32, _vp, _c_i32, _c_i32,
                                        ctypes.c_uint32, _c_f64, _c_f64, _c_i32, _c_i32, _vp, _c_size, _vp, _vp, _vp,
                                        _vp, _vp, _vp]),
    # insite_score.h
    "insite_score_abi_version": (_c_i32, []),
    "insite_score_workspace_bytes": (_c_size, [_c_i64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32]),
    "insite_score_sums_f64": (_c_i32, [_vp, _vp, _vp, _c_i64, _vp, _vp, _c_i32, _c_i64, _c_i32, _c_i32, _c_i32, _c_f64,
                                       _c_i32, _c_i32, _c_f64, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp, _c_i32, _vp,
                                       _c_i32, _c_i32, _vp, _c_size, _vp, _c_i64, _vp]),
}

# (getter, the version these bindings were written for, the label of the mismatch message)
_ABI_VERSIONS = (
    ("insite_abi_version", ABI_VERSION, ""),
    ("insite_irregular_abi_version", IRREGULAR_ABI_VERSION, "irregular "),
    ("insite_weak_abi_version", WEAK_ABI_VERSION, "weak "),
    ("insite_bootstrap_abi_version", BOOTSTRAP_ABI_VERSION, "bootstrap "),
    ("insite_effect_abi_version", EFFECT_ABI_VERSION, "effect "),
    ("insite_cohort_abi_version", COHORT_ABI_VERSION, "cohort "),
    ("insite_regimen_abi_version", REGIMEN_ABI_VERSION, "regimen "),
    ("insite_policy_abi_version", POLICY_ABI_VERSION, "policy "),
    ("insite_feedback_abi_version", FEEDBACK_ABI_VERSION, "feedback "),
    ("insite_rulevalue_abi_version", RULEVALUE_ABI_VERSION, "rulevalue "),
    ("insite_segboot_abi_version", SEGBOOT_ABI_VERSION, "segboot "),
    ("insite_score_abi_version", SCORE_ABI_VERSION, "score "),
)


def load(path: str | None = None):
    """Load (once) and return the ctypes handle; raises InsiteLibraryError if unavailable."""
    global _lib
    if path is None and _lib is not None:   # lock-free fast path once loaded
        return _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise InsiteLibraryError(
                f"{p} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')")
        try:
            lib = ctypes.CDLL(p, mode=ctypes.RTLD_LOCAL)
        except OSError as e:  # pragma: no cover - environment specific
            raise InsiteLibraryError(f"cannot load {p}: {e}") from e
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        for getter, want, label in _ABI_VERSIONS:
            v = getattr(lib, getter)()
            if v != want:
                raise InsiteLibraryError(f"{label}ABI version mismatch: library {v}, bindings {want}")
        if path is None:
            _lib = lib
        return lib


def check(fn_name: str, code: int):
    if code != INSITE_OK:
        msg = load().insite_strerror(code).decode()
        raise InsiteError(fn_name, code, msg)
