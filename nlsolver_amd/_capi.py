"""ctypes binding of libnlsolver_hip.so (include/nlsg_c_api.h).

The library is the product's only compute path. There is no CPU fallback: if
the shared object is missing or no gfx950 device is visible, calls raise.
"""
import ctypes as C
import sys
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# $NLSG_LIBRARY names another build of the library (as for the C++ header): A/B runs of variants
LIB_PATH = os.environ.get("NLSG_LIBRARY") or os.path.join(HERE, "libnlsolver_hip.so")

u64, i32, f64 = C.c_uint64, C.c_int32, C.c_double
pd = C.POINTER(C.c_double)
pu = C.POINTER(C.c_uint64)

OBJECTIVES = {"rosenbrock": 0, "sphere": 1, "styblinski_tang": 2, "rastrigin": 3}
DE_BEST, DE_RANDOM = 0, 1  # enum RecombinationStrategy { best, random }, nlsolver.h:2377


class NlsgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nlsg error {code}: {msg}")
        self.code = code


class Status(C.Structure):
    """nlsg_status == solver_status<T> (nlsolver.h:2054-2097) + engine fields."""
    _fields_ = [("f_value", f64), ("iteration", u64), ("function_calls_used", u64),
                ("gradient_evals_used", u64), ("hessian_evals_used", u64),
                ("best_index", u64), ("val_no_change", u64), ("std_err", f64),
                ("done", i32), ("reserved", i32)]

    def get_summary(self):
        # tuple order of solver_status::get_summary, nlsolver.h:2079-2083
        return (self.function_calls_used, self.iteration, self.f_value,
                self.gradient_evals_used, self.hessian_evals_used)


class DEConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("minimize", i32), ("strategy", i32), ("trace", i32),
                ("pop", u64), ("dim", u64), ("shard_lo", u64), ("shard_n", u64),
                ("CR", f64), ("F", f64), ("eps", f64),
                ("max_iter", u64), ("best_val_no_change", u64), ("seed", u64)]


OBJ_CUSTOM = 64


class DERefConfig(C.Structure):  # nlsg_de_ref_config
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("minimize", i32), ("strategy", i32), ("reserved", i32),
                ("batch", u64), ("pop", u64), ("dim", u64),
                ("CR", f64), ("F", f64), ("eps", f64),
                ("max_iter", u64), ("best_val_no_change", u64), ("log_capacity", u64)]


class DEBatchConfig(C.Structure):  # nlsg_de_batch_config
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("minimize", i32), ("strategy", i32), ("reserved", i32),
                ("batch", u64), ("pop", u64), ("dim", u64),
                ("CR", f64), ("F", f64), ("eps", f64),
                ("max_iter", u64), ("best_val_no_change", u64), ("turns_per_launch", u64)]


class CustomObjectiveC(C.Structure):  # nlsg_custom_objective
    _fields_ = [("term_body", C.c_char_p), ("finish_body", C.c_char_p), ("chain", i32),
                ("n_params", i32)]  # run-time doubles per solve (resident batch engines), 0 = none


PSO_VANILLA, PSO_ACCELERATED = 0, 1  # enum PSOType { Vanilla, Accelerated }, nlsolver.h:2496


class PSOConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("minimize", i32), ("type", i32), ("bounded", i32),
                ("n_particles", u64), ("dim", u64), ("shard_lo", u64), ("shard_n", u64),
                ("inertia", f64), ("cognitive", f64), ("social", f64), ("eps", f64),
                ("max_iter", u64), ("best_val_no_change", u64), ("seed", u64)]


class PSOBatchConfig(C.Structure):  # nlsg_pso_batch_config
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("minimize", i32), ("type", i32), ("bounded", i32),
                ("batch", u64), ("n_particles", u64), ("dim", u64),
                ("inertia", f64), ("cognitive", f64), ("social", f64), ("eps", f64),
                ("max_iter", u64), ("best_val_no_change", u64), ("turns_per_launch", u64)]


OBJ_QUAD_DIAG_RANK1 = 16


class BFGSConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("flags", i32), ("batch", u64), ("dim", u64),
                ("max_iter", u64), ("grad_eps", f64), ("alpha", f64), ("quad_c", f64)]


class BFGSGradientC(C.Structure):  # nlsg_bfgs_gradient
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("grad_body", C.c_char_p)]


BFGS_SYMMETRIC = 1  # NLSG_BFGS_SYMMETRIC
BFGS_REFERENCE_ORDER = 2  # NLSG_BFGS_REFERENCE_ORDER
BFGS_RESIDENT = 4  # NLSG_BFGS_RESIDENT


OBJ_TANH_REGRESSION = 32
OBJ_LINK_REGRESSION = 33  # NLSG_OBJ_LINK_REGRESSION: nlsg_lm_create_link
OBJ_CURVE_MODEL = 34  # NLSG_OBJ_CURVE_MODEL: nlsg_lm_create_curve
LM_CHOLESKY, LM_QR, LM_CHOLESKY_REFERENCE_ORDER = 0, 1, 2
LM_RESIDENT = 256  # NLSG_LM_RESIDENT: a flag OR-ed into the solver (the low byte is the nlsg_lm_solver)
LM_RESIDENT_CUT = 256  # turns per launch of the resident driver (kLmResidentCut)
LM_COV_RESIDUAL, LM_COV_ABSOLUTE = 0, 1  # nlsg_lm_cov_scale: cov = s2 (J^T J)^-1, or (J^T J)^-1


class LMConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("solver", i32), ("batch", u64), ("m", u64), ("n", u64),
                ("lambda_", f64), ("up", f64), ("down", f64), ("max_iter", u64), ("f_delta", f64)]


class LMLinkC(C.Structure):  # nlsg_lm_link
    _fields_ = [("value_body", C.c_char_p), ("slope_body", C.c_char_p)]


class LMCurveC(C.Structure):  # nlsg_lm_curve
    _fields_ = [("body", C.c_char_p), ("k", C.c_uint32)]


NM_REFERENCE_ORDER = 1  # NLSG_NM_REFERENCE_ORDER


class NMConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("minimize", i32), ("bounded", i32), ("flags", i32),
                ("batch", u64), ("dim", u64),
                ("step", f64), ("alpha", f64), ("gamma", f64), ("rho", f64), ("sigma", f64),
                ("eps", f64), ("max_iter", u64), ("no_change_best_tol", u64), ("restarts", u64)]


class SANNConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("minimize", i32), ("batch", u64), ("dim", u64),
                ("chain_lo", u64), ("max_iter", u64), ("temperature_iter", u64),
                ("temperature_max", f64), ("seed", u64)]


class NMPSOConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", i32), ("stream", C.c_void_p),
                ("objective", i32), ("minimize", i32), ("bounded", i32), ("reserved", i32),
                ("batch", u64), ("dim", u64), ("inst_lo", u64),
                ("alpha", f64), ("gamma", f64), ("rho", f64), ("sigma", f64),
                ("inertia", f64), ("cognitive", f64), ("social", f64), ("eps", f64),
                ("max_iter", u64), ("no_change_best_iter", u64), ("seed", u64)]


# every symbol include/nlsg_c_api.h declares: name -> (restype, argtypes)
_H = C.c_void_p
SYMBOLS = {
    "nlsg_last_error": (C.c_char_p, []),
    "nlsg_abi_version": (C.c_int, []),
    "nlsg_device_count": (C.c_int, []),
    "nlsg_call_timing": (C.c_int, [pd]),
    "nlsg_release_cached": (C.c_int, []),
    "nlsg_cached_bytes": (u64, []),
    "nlsg_pool_poison": (C.c_int, []),
    "nlsg_probe_math": (C.c_int, [C.c_int32, pu, pu, u64, C.c_int32]),
    "nlsg_de_create": (C.c_int, [C.POINTER(DEConfig), C.POINTER(_H)]),
    "nlsg_de_destroy": (C.c_int, [_H]),
    "nlsg_de_init": (C.c_int, [_H, pd]),
    "nlsg_de_step": (C.c_int, [_H, u64]),
    "nlsg_de_minimize": (C.c_int, [_H, pd, u64, C.POINTER(Status)]),
    "nlsg_de_status": (C.c_int, [_H, C.POINTER(Status)]),
    "nlsg_de_best": (C.c_int, [_H, pd, pd, pu]),
    "nlsg_de_download": (C.c_int, [_H, pd, pd, pu]),
    "nlsg_de_upload": (C.c_int, [_H, pd, pd]),
    "nlsg_de_time_generation_kernel": (C.c_int, [_H, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_de_time_turns": (C.c_int, [_H, u64, C.POINTER(C.c_float)]),
    "nlsg_de_record_doubles": (u64, [_H]),
    "nlsg_de_turn_begin": (C.c_int, [_H, C.c_void_p]),
    "nlsg_de_turn_end": (C.c_int, [_H, C.c_void_p, i32]),
    "nlsg_de_turn_finalize": (C.c_int, [_H, C.c_void_p, i32]),
    "nlsg_de_turn_generation": (C.c_int, [_H]),
    "nlsg_de_can_speculate": (C.c_int, [_H]),
    "nlsg_rtc_load": (C.c_int, [C.c_char_p]),
    "nlsg_de_create_custom": (C.c_int, [C.POINTER(DEConfig), C.POINTER(CustomObjectiveC),
                                        C.POINTER(C.c_void_p)]),
    "nlsg_pso_create_custom": (C.c_int, [C.POINTER(PSOConfig), C.POINTER(CustomObjectiveC),
                                         C.POINTER(C.c_void_p)]),
    "nlsg_nm_create_custom": (C.c_int, [C.POINTER(NMConfig), C.POINTER(CustomObjectiveC),
                                        C.POINTER(C.c_void_p)]),
    "nlsg_bfgs_create_custom": (C.c_int, [C.POINTER(BFGSConfig), C.POINTER(CustomObjectiveC),
                                          C.POINTER(C.c_void_p)]),
    "nlsg_lm_create_custom": (C.c_int, [C.POINTER(LMConfig), C.POINTER(CustomObjectiveC),
                                        C.POINTER(C.c_void_p)]),
    "nlsg_comm_load": (C.c_int, [C.c_char_p]),
    "nlsg_comm_unique_id": (C.c_int, [C.POINTER(C.c_ubyte)]),
    "nlsg_de_comm_attach": (C.c_int, [_H, C.POINTER(C.c_ubyte), C.c_int32, C.c_int32]),
    "nlsg_de_step_sharded": (C.c_int, [_H, C.c_uint64]),
    "nlsg_de_comm_ranks": (C.c_int, [_H, C.POINTER(i32), C.POINTER(i32)]),
    "nlsg_pso_comm_ranks": (C.c_int, [_H, C.POINTER(i32), C.POINTER(i32)]),
    "nlsg_pso_comm_attach": (C.c_int, [_H, C.POINTER(C.c_ubyte), C.c_int32, C.c_int32]),
    "nlsg_pso_step_sharded": (C.c_int, [_H, C.c_uint64]),
    "nlsg_pso_create": (C.c_int, [C.POINTER(PSOConfig), C.POINTER(_H)]),
    "nlsg_pso_destroy": (C.c_int, [_H]),
    "nlsg_pso_init": (C.c_int, [_H, pd, pd]),
    "nlsg_pso_step": (C.c_int, [_H, u64]),
    "nlsg_pso_minimize": (C.c_int, [_H, pd, pd, pd, u64, C.POINTER(Status)]),
    "nlsg_pso_status": (C.c_int, [_H, C.POINTER(Status)]),
    "nlsg_pso_best": (C.c_int, [_H, pd, pd, pu]),
    "nlsg_pso_download": (C.c_int, [_H, pd, pd, pd, pd]),
    "nlsg_pso_time_move_kernel": (C.c_int, [_H, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_pso_record_doubles": (u64, [_H]),
    "nlsg_pso_turn_begin": (C.c_int, [_H, C.c_void_p]),
    "nlsg_pso_turn_end": (C.c_int, [_H, C.c_void_p, i32]),
    "nlsg_bfgs_create": (C.c_int, [C.POINTER(BFGSConfig), pd, pd, C.POINTER(_H)]),
    "nlsg_bfgs_destroy": (C.c_int, [_H]),
    "nlsg_bfgs_init": (C.c_int, [_H, pd]),
    "nlsg_bfgs_step": (C.c_int, [_H, u64]),
    "nlsg_bfgs_unfinished": (C.c_int, [_H, pu]),
    "nlsg_bfgs_identity_count": (C.c_int, [_H, pu]),
    "nlsg_bfgs_download": (C.c_int, [_H, pd, C.POINTER(Status)]),
    "nlsg_bfgs_download_state": (C.c_int, [_H, pd, pd]),
    "nlsg_bfgs_minimize": (C.c_int, [_H, pd, C.POINTER(Status)]),
    "nlsg_bfgs_time_steps": (C.c_int, [_H, u64, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "nlsg_tinyqr_lm": (C.c_int, [pd, pd, u64, u64, u64, f64, i32, pd, C.POINTER(C.c_float)]),
    "nlsg_tinyqr_lm_device": (C.c_int, [C.c_void_p, C.c_void_p, u64, u64, u64, f64, i32, C.c_void_p,
                                        C.c_void_p]),
    "nlsg_tinyqr_qr": (C.c_int, [pd, pd, u64, u64, u64, f64, i32, pd, pd, pd]),
    "nlsg_lm_create": (C.c_int, [C.POINTER(LMConfig), C.POINTER(_H)]),
    "nlsg_lm_destroy": (C.c_int, [_H]),
    "nlsg_lm_set_data": (C.c_int, [_H, pd, pd]),
    "nlsg_lm_set_solver": (C.c_int, [_H, i32]),
    "nlsg_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), u64]),
    "nlsg_host_free": (C.c_int, [C.c_void_p]),
    "nlsg_lm_minimize": (C.c_int, [_H, pd, C.POINTER(Status), pd]),
    "nlsg_lm_time_solve": (C.c_int, [_H, pd, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_lm_time_eval_kernel": (C.c_int, [_H, pd, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_lm_time_qr_kernel": (C.c_int, [_H, pd, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_nm_create": (C.c_int, [C.POINTER(NMConfig), C.POINTER(_H)]),
    "nlsg_nm_destroy": (C.c_int, [_H]),
    "nlsg_nm_minimize": (C.c_int, [_H, pd, pd, pd, C.POINTER(Status), pd]),
    "nlsg_nm_phase_cycles": (C.c_int, [_H, pd, pu]),
    "nlsg_nm_time_solve": (C.c_int, [_H, pd, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_nmpso_create": (C.c_int, [C.POINTER(NMPSOConfig), C.POINTER(_H)]),
    "nlsg_nmpso_create_custom": (C.c_int, [C.POINTER(NMPSOConfig), C.POINTER(CustomObjectiveC),
                                           C.POINTER(C.c_void_p)]),
    "nlsg_nmpso_destroy": (C.c_int, [_H]),
    "nlsg_nmpso_minimize": (C.c_int, [_H, pd, pd, pd, C.POINTER(Status)]),
    "nlsg_nmpso_time_solve": (C.c_int, [_H, pd, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_sann_create": (C.c_int, [C.POINTER(SANNConfig), C.POINTER(_H)]),
    "nlsg_sann_create_custom": (C.c_int, [C.POINTER(SANNConfig), C.POINTER(CustomObjectiveC),
                                          C.POINTER(C.c_void_p)]),
    "nlsg_sann_destroy": (C.c_int, [_H]),
    "nlsg_sann_minimize": (C.c_int, [_H, pd, C.POINTER(Status)]),
    "nlsg_sann_time_solve": (C.c_int, [_H, pd, C.c_uint32, C.POINTER(C.c_float)]),
}

# Bound when the library has them: a library built without reference-order DE still loads for
# everything else and fails only when that is asked for (require()).
OPTIONAL_SYMBOLS = {
    "nlsg_de_ref_create": (C.c_int, [C.POINTER(DERefConfig), C.POINTER(_H)]),
    "nlsg_de_ref_create_custom": (C.c_int, [C.POINTER(DERefConfig), C.POINTER(CustomObjectiveC),
                                            C.POINTER(_H)]),
    "nlsg_de_ref_destroy": (C.c_int, [_H]),
    "nlsg_de_ref_minimize": (C.c_int, [_H, pd, pu, C.POINTER(Status)]),
    "nlsg_de_ref_log": (C.c_int, [_H, u64, pd, pd, pu]),
    "nlsg_de_ref_time_solve": (C.c_int, [_H, pd, pu, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_de_ref_jump_table": (C.c_int, [pu]),
    "nlsg_de_ref_pick_donors": (C.c_int, [pd, u64, u64, u64, pu, pu, C.POINTER(i32)]),
    "nlsg_de_bound_counts": (C.c_int, [_H, pu]),
    "nlsg_de_bound_state": (C.c_int, [_H, C.POINTER(i32), C.POINTER(C.c_uint32)]),
    "nlsg_de_bound_gate": (C.c_int, [i32, i32, i32, f64, u64]),
    "nlsg_de_screen_counts": (C.c_int, [_H, pu]),
    "nlsg_de_screen_state": (C.c_int, [_H, C.POINTER(i32), C.POINTER(C.c_uint32)]),
    "nlsg_de_screen_gate": (C.c_int, [i32, i32, i32, f64, u64]),
    "nlsg_de_screen_env": (C.c_int, [C.POINTER(i32), C.POINTER(C.c_uint32)]),
    "nlsg_de_screen_rule": (C.c_int, [C.c_uint32, u64, u64, C.c_uint32, C.c_uint32, i32,
                                      C.POINTER(C.c_uint32)]),
    "nlsg_custom_params_lds_bytes": (u64, [i32]),
    "nlsg_de_batch_lds_bytes": (u64, [u64, u64]),
    "nlsg_de_batch_create": (C.c_int, [C.POINTER(DEBatchConfig), C.POINTER(_H)]),
    "nlsg_de_batch_create_custom": (C.c_int, [C.POINTER(DEBatchConfig), C.POINTER(CustomObjectiveC),
                                              C.POINTER(_H)]),
    "nlsg_de_batch_set_params": (C.c_int, [_H, pd]),
    "nlsg_de_batch_destroy": (C.c_int, [_H]),
    "nlsg_de_batch_init": (C.c_int, [_H, pd, pu]),
    "nlsg_de_batch_step": (C.c_int, [_H, u64]),
    "nlsg_de_batch_status": (C.c_int, [_H, C.POINTER(Status)]),
    "nlsg_de_batch_best": (C.c_int, [_H, pd, pd, pu]),
    "nlsg_de_batch_download": (C.c_int, [_H, u64, pd, pd]),
    "nlsg_de_batch_upload": (C.c_int, [_H, pd, pd]),
    "nlsg_de_batch_minimize": (C.c_int, [_H, pd, pu, C.POINTER(Status)]),
    "nlsg_de_batch_time_solve": (C.c_int, [_H, pd, pu, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_pso_batch_lds_bytes": (u64, [u64, u64, i32]),
    "nlsg_pso_batch_create": (C.c_int, [C.POINTER(PSOBatchConfig), C.POINTER(_H)]),
    "nlsg_pso_batch_create_custom": (C.c_int, [C.POINTER(PSOBatchConfig), C.POINTER(CustomObjectiveC),
                                               C.POINTER(_H)]),
    "nlsg_pso_batch_set_params": (C.c_int, [_H, pd]),
    "nlsg_pso_batch_destroy": (C.c_int, [_H]),
    "nlsg_pso_batch_init": (C.c_int, [_H, pd, pd, pu]),
    "nlsg_pso_batch_step": (C.c_int, [_H, u64]),
    "nlsg_pso_batch_status": (C.c_int, [_H, C.POINTER(Status)]),
    "nlsg_pso_batch_best": (C.c_int, [_H, pd, pd, pu]),
    "nlsg_pso_batch_download": (C.c_int, [_H, u64, pd, pd, pd, pd]),
    "nlsg_pso_batch_minimize": (C.c_int, [_H, pd, pd, pd, pu, C.POINTER(Status)]),
    "nlsg_pso_batch_time_solve": (C.c_int, [_H, pd, pd, pu, C.c_uint32, C.POINTER(C.c_float)]),
    "nlsg_nm_create_params": (C.c_int, [C.POINTER(NMConfig), C.POINTER(CustomObjectiveC), C.POINTER(_H)]),
    "nlsg_nm_set_params": (C.c_int, [_H, pd]),
    "nlsg_nm_lds_bytes": (u64, [u64, C.c_uint32]),
    "nlsg_nmpso_create_params": (C.c_int, [C.POINTER(NMPSOConfig), C.POINTER(CustomObjectiveC),
                                           C.POINTER(_H)]),
    "nlsg_nmpso_set_params": (C.c_int, [_H, pd]),
    "nlsg_nmpso_lds_bytes": (u64, [u64]),
    "nlsg_lm_create_params": (C.c_int, [C.POINTER(LMConfig), C.POINTER(CustomObjectiveC), C.POINTER(_H)]),
    "nlsg_lm_set_params": (C.c_int, [_H, pd]),
    "nlsg_lm_lds_bytes": (u64, [u64, C.c_int32]),
    "nlsg_lm_create_link": (C.c_int, [C.POINTER(LMConfig), C.POINTER(LMLinkC), C.POINTER(_H)]),
    "nlsg_lm_create_curve": (C.c_int, [C.POINTER(LMConfig), C.POINTER(LMCurveC), C.POINTER(_H)]),
    "nlsg_lm_set_curve_data": (C.c_int, [_H, pd, pd]),
    "nlsg_lm_covariance": (C.c_int, [_H, pd, i32, pd, pd, C.POINTER(C.c_int32)]),
    "nlsg_bfgs_create_params": (C.c_int, [C.POINTER(BFGSConfig), C.POINTER(CustomObjectiveC), C.POINTER(_H)]),
    "nlsg_bfgs_set_params": (C.c_int, [_H, pd]),
    "nlsg_bfgs_lds_bytes": (u64, [u64, C.c_uint32]),
    "nlsg_bfgs_create_gradient": (C.c_int, [C.POINTER(BFGSConfig), C.POINTER(CustomObjectiveC),
                                            C.POINTER(BFGSGradientC), C.POINTER(_H)]),
    "nlsg_sann_create_params": (C.c_int, [C.POINTER(SANNConfig), C.POINTER(CustomObjectiveC), C.POINTER(_H)]),
    "nlsg_sann_set_params": (C.c_int, [_H, pd]),
    "nlsg_sann_chains_per_wave": (C.c_uint32, [u64, i32]),
    "nlsg_sann_lds_bytes": (u64, [u64, i32]),
}
SYMBOLS.update(OPTIONAL_SYMBOLS)
_PARAMS = "library has no run-time objective parameters"
_CURVE = "library has no curve models for Levenberg-Marquardt"
# what require() says about a missing entry point: the longest prefix of its name that stands here
_MISSING_MESSAGE = {"nlsg_de_ref_": "library has no reference-order DE",
                    "nlsg_de_bound_": "library has no lower-bound rejection in the DE generation",
                    "nlsg_de_screen_": "library has no half-row screen in the DE generation",
                    "nlsg_de_batch_": "library has no resident batch DE",
                    "nlsg_pso_batch_": "library has no resident batch PSO",
                    "nlsg_custom_params_": _PARAMS,
                    "nlsg_de_batch_set_params": _PARAMS,
                    "nlsg_pso_batch_set_params": _PARAMS,
                    "nlsg_nm_": _PARAMS + " for Nelder-Mead",
                    "nlsg_nmpso_": _PARAMS + " for the hybrid",
                    "nlsg_lm_": _PARAMS + " for Levenberg-Marquardt",
                    "nlsg_bfgs_": _PARAMS + " for BFGS",
                    "nlsg_sann_": _PARAMS + " for simulated annealing",
                    "nlsg_lm_create_link": "library has no user-supplied link functions for Levenberg-Marquardt",
                    "nlsg_lm_create_curve": _CURVE,
                    "nlsg_lm_set_curve_data": _CURVE,
                    "nlsg_lm_covariance": "library has no parameter covariance for Levenberg-Marquardt",
                    "nlsg_bfgs_create_gradient": "library has no analytic gradients of compiled objectives for BFGS"}

_lib = None


def lib():
    """Load libnlsolver_hip.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NlsgError(-1, f"{LIB_PATH} is missing: build it with "
                                "`make -C nlsolver_amd/csrc` (no CPU fallback exists)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name, None) if name in OPTIONAL_SYMBOLS else getattr(l, name)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def require(name):
    """The optional entry point `name`; NlsgError if this build of the library lacks it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        prefix = max((p for p in _MISSING_MESSAGE if name.startswith(p)), key=len, default=None)
        msg = _MISSING_MESSAGE.get(prefix, f"library has no {name}")
        raise NlsgError(NLSG_ERR_UNSUPPORTED, msg)
    return fn


NLSG_ERR_INVALID_ARG, NLSG_ERR_UNSUPPORTED = 1, 2
CUSTOM_MAX_PARAMS = 4096  # NLSG_CUSTOM_MAX_PARAMS


def check(rc):
    if rc != 0:
        raise NlsgError(rc, lib().nlsg_last_error().decode(errors="replace"))


class _PinnedBlock:
    """Owner of one nlsg_host_alloc block; numpy arrays made by pinned_empty keep it alive."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        check(lib().nlsg_host_alloc(C.byref(self.ptr), nbytes))

    def __del__(self):
        # at interpreter shutdown the module globals, the ctypes handle or the HIP runtime may be
        # gone already: the process is about to release the memory anyway
        try:
            if sys.is_finalizing():
                return
            if getattr(self, "ptr", None) and self.ptr.value:
                lib().nlsg_host_free(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def pinned_empty(shape, dtype="float64"):
    """numpy array in page-locked host memory (nlsg_host_alloc): what is handed to the engines from
    there crosses PCIe by DMA at the link's rate (e.g. the design matrices of an LM model). The
    memory is released when the array (and every view of it) is gone."""
    import numpy as np
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    nbytes = max(count * dt.itemsize, 8)
    block = _PinnedBlock(nbytes)
    buf = (C.c_char * nbytes).from_address(block.ptr.value)
    buf._nlsg_owner = block  # the array's base is `buf`; `buf` keeps the block alive
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


PROBE_FUNCTIONS = {"log": 0, "cos": 1, "exp": 2, "tanh": 3, "cos_2pi": 4, "u01": 5, "rnorm": 6,
                   "log_unit": 7, "rnorm_cos": 8, "givens_t": 9, "sqrt": 10, "wave_sum": 11}


def probe_math(fn, bits, device=0):
    """nlsg_probe_math: the device's deterministic primitive `fn` ("log", "cos", "exp", "tanh",
    "cos_2pi", "log_unit", "givens_t", "sqrt": argument = a double's bit pattern; "u01", "rnorm",
    "rnorm_cos": argument = a 64-bit draw) on a uint64 array; returns the results' bit patterns.
    "wave_sum": the array's size is a multiple of 64, and element i is the kernels' butterfly sum
    over the 64 doubles of its wave, as lane i % 64 holds it."""
    import numpy as np
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    out = np.empty_like(bits)
    check(lib().nlsg_probe_math(PROBE_FUNCTIONS[fn], bits.ctypes.data_as(pu), out.ctypes.data_as(pu),
                                bits.size, device))
    return out
