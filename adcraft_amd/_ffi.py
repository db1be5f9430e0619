"""ctypes binding of include/adcraft_engine.h (the C ABI of the HIP engine).

No PyTorch, no fallbacks: if the shared library is missing and cannot be built, or if no HIP
device is usable, the error is raised to the caller.  ctypes releases the GIL during calls.
"""
import ctypes as C
import os

from . import build as _build

ADC_OK, ADC_EINVAL, ADC_EHIP, ADC_ENOMEM, ADC_ESTATE, ADC_ETYPE, ADC_ERCCL = 0, -1, -2, -3, -4, -5, -6
MODEL_IMPLICIT, MODEL_EXPLICIT, MODEL_IMPLICIT_GENERAL = 0, 1, 2
P_VOL_MEAN, P_VOL_STD, P_A, P_B, P_BCTR, P_SCTR, P_REV_MEAN, P_REV_STD, P_COUNT = range(9)
(BUF_PARAMS, BUF_BIDS, BUF_BUDGET, BUF_IMPRESSIONS, BUF_CLICKS, BUF_CONVERSIONS, BUF_COST, BUF_REVENUE, BUF_REWARD,
 BUF_CUM_PROFIT, BUF_DAYS, BUF_TERMINATED, BUF_TRUNCATED, BUF_METRIC_PROFIT, BUF_METRIC_SCALARS, BUF_FLAT_OBS,
 BUF_ROLLOUT_ACTION, BUF_ROLLOUT_LOGP, BUF_ROLLOUT_VALUE, BUF_ROLLOUT_REWARD, BUF_ROLLOUT_TERMINATED, BUF_ROLLOUT_TRUNCATED,
 BUF_ROLLOUT_OBS) = range(23)
MLP_TANH, MLP_RELU = 0, 1
ES_CENTERED_RANK, ES_RAW = 0, 1
ES_ADAM, ES_SGD = 0, 1
ROLLOUT_OBS = 1
PG_ADAM, PG_SGD = 0, 1
TD3_ADAM, TD3_SGD = 0, 1
PBT_PG, PBT_TD3 = 0, 1
PBT_SAC = 3        # (2 is unassigned)


class EngineError(RuntimeError):
    pass


class EngineStateError(AssertionError):
    """ADC_ESTATE: the call is not valid in the engine's current state (step before reset, a step whose clicks can no longer be
    replayed ...).  An AssertionError, as the reference raises for step-before-reset (gymnasium_kw_env.py:194-196), but one of its
    own type, so that callers can tell it from a genuine Python `assert` failing."""


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device_id", C.c_int32), ("num_envs", C.c_int32),
                ("num_keywords", C.c_int32), ("model", C.c_int32), ("max_days", C.c_int32),
                ("loss_threshold", C.c_double), ("drift_vol", C.c_float), ("drift_ctr", C.c_float),
                ("drift_cvr", C.c_float), ("drift_enabled", C.c_int32), ("impression_thresh", C.c_float),
                ("auto_reset", C.c_int32), ("env_id_base", C.c_int64), ("seed", C.c_uint64)]


class StepOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("impressions", "buyside_clicks", "sellside_conversions", "cost", "revenue",
                                          "reward", "cumulative_profit", "days_passed", "terminated", "truncated",
                                          "counts_u16", "counts_overflow")]


class Quantiles(C.Structure):
    _fields_ = [("buckets", C.c_int32 * 7), ("mins", C.c_void_p * 7), ("medians", C.c_void_p * 7), ("maxs", C.c_void_p * 7)]


class MLPConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("activation", C.c_int32), ("n_policy_layers", C.c_int32),
                ("policy_widths", C.c_int32 * 4), ("n_value_layers", C.c_int32), ("value_widths", C.c_int32 * 4),
                ("normalize", C.c_int32), ("clamp_log_std", C.c_int32), ("log_std_lo", C.c_float), ("log_std_hi", C.c_float),
                ("bid_clip_hi", C.c_float), ("deterministic", C.c_int32)]


class ESConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sigma", C.c_float), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("eps", C.c_float), ("l2", C.c_float), ("shaping", C.c_int32), ("optimiser", C.c_int32), ("seed", C.c_uint64)]


class ESStats(C.Structure):
    _fields_ = [("generation", C.c_int64), ("fitness_mean", C.c_double), ("fitness_max", C.c_double), ("fitness_min", C.c_double),
                ("grad_norm", C.c_double), ("theta_norm", C.c_double)]


class PGConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("gamma", C.c_float), ("lambda_", C.c_float), ("eps_clip", C.c_float), ("vf_coef", C.c_float),
                ("ent_coef", C.c_float), ("reward_scale", C.c_float), ("normalize_advantages", C.c_int32), ("max_grad_norm", C.c_float),
                ("optimiser", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("minibatch_envs", C.c_int32)]


class PGStats(C.Structure):
    _fields_ = [("steps", C.c_int64), ("samples", C.c_int64), ("policy_loss", C.c_double), ("value_loss", C.c_double),
                ("entropy", C.c_double), ("approx_kl", C.c_double), ("clip_fraction", C.c_double), ("grad_norm", C.c_double),
                ("explained_variance", C.c_double)]


class PGKLConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kl_coef", C.c_float), ("kl_target", C.c_float), ("adaptive", C.c_int32),
                ("factor_up", C.c_float), ("factor_down", C.c_float), ("vf_clip", C.c_float)]


class PGShuffleConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("minibatch_samples", C.c_int32), ("seed", C.c_uint64), ("target_kl", C.c_float)]


class PGShuffleStats(C.Structure):
    _fields_ = [("epochs_begun", C.c_int32), ("minibatches_evaluated", C.c_int32), ("steps_taken", C.c_int32), ("stopped", C.c_int32)]


class PGKLStats(C.Structure):
    _fields_ = [("kl", C.c_double), ("vf_clip_fraction", C.c_double), ("kl_coef", C.c_float), ("kl_coef_next", C.c_float)]


class IMConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("beta", C.c_float), ("vf_coef", C.c_float), ("w_max", C.c_float), ("ma_start", C.c_double),
                ("ma_rate", C.c_double), ("train_log_std", C.c_int32)]


class IMStats(C.Structure):
    _fields_ = [("steps", C.c_int64), ("samples", C.c_int64), ("policy_loss", C.c_double), ("value_loss", C.c_double),
                ("entropy", C.c_double), ("logp", C.c_double), ("weight", C.c_double), ("grad_norm", C.c_double),
                ("explained_variance", C.c_double)]


class TD3Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("gamma", C.c_float), ("tau", C.c_float), ("policy_delay", C.c_int32),
                ("target_noise", C.c_float), ("target_noise_clip", C.c_float), ("action_lo", C.c_float), ("action_hi", C.c_float),
                ("reward_scale", C.c_float), ("batch_size", C.c_int32), ("capacity", C.c_int32), ("n_critic_layers", C.c_int32),
                ("critic_widths", C.c_int32 * 4), ("actor_lr", C.c_float), ("critic_lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("optimiser", C.c_int32), ("max_grad_norm", C.c_float), ("seed", C.c_uint64)]


class TD3Stats(C.Structure):
    _fields_ = [("updates", C.c_int64), ("actor_steps", C.c_int64), ("buffer_size", C.c_int64), ("samples", C.c_int64),
                ("critic_loss", C.c_double), ("q1_mean", C.c_double), ("q2_mean", C.c_double), ("y_mean", C.c_double),
                ("actor_loss", C.c_double), ("critic_grad_norm", C.c_double), ("actor_grad_norm", C.c_double)]


class SACConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("gamma", C.c_float), ("tau", C.c_float), ("target_update_interval", C.c_int32),
                ("init_alpha", C.c_float), ("target_entropy", C.c_float), ("alpha_lr", C.c_float), ("eps_sq", C.c_float),
                ("reward_scale", C.c_float), ("batch_size", C.c_int32), ("capacity", C.c_int32), ("n_critic_layers", C.c_int32),
                ("critic_widths", C.c_int32 * 4), ("actor_lr", C.c_float), ("critic_lr", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("optimiser", C.c_int32), ("max_grad_norm", C.c_float), ("seed", C.c_uint64)]


class SACStats(C.Structure):
    _fields_ = [("updates", C.c_int64), ("buffer_size", C.c_int64), ("samples", C.c_int64), ("critic_loss", C.c_double),
                ("q1_mean", C.c_double), ("q2_mean", C.c_double), ("y_mean", C.c_double), ("actor_loss", C.c_double),
                ("logp_mean", C.c_double), ("alpha", C.c_double), ("log_alpha", C.c_double), ("critic_grad_norm", C.c_double),
                ("actor_grad_norm", C.c_double)]


class PBTConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("replace_count", C.c_int32), ("fitness_ema", C.c_float), ("factor_lo", C.c_float),
                ("factor_hi", C.c_float), ("log_factor_lo", C.c_float), ("log_factor_hi", C.c_float), ("tuned_mask", C.c_uint32),
                ("lo", C.c_float * 8), ("hi", C.c_float * 8), ("with_ring", C.c_int32), ("seed", C.c_uint64)]


class PBTResult(C.Structure):
    _fields_ = [("fitness", C.c_double), ("smoothed", C.c_double), ("rank", C.c_int32), ("src", C.c_int32), ("hp", C.c_float * 8)]


class ObsNormConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("per_member", C.c_int32), ("min_std", C.c_double), ("count_cap", C.c_int64)]


class RewNormConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("per_member", C.c_int32), ("min_std", C.c_double), ("clip", C.c_float), ("count_cap", C.c_int64)]


class TD3NormConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("observations", C.c_int32), ("rewards", C.c_int32), ("per_member", C.c_int32), ("obs_min_std", C.c_double),
                ("obs_count_cap", C.c_int64), ("rew_min_std", C.c_double), ("rew_count_cap", C.c_int64), ("rew_clip", C.c_float)]


class SACNormConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("observations", C.c_int32), ("rewards", C.c_int32), ("per_member", C.c_int32), ("obs_min_std", C.c_double),
                ("obs_count_cap", C.c_int64), ("rew_min_std", C.c_double), ("rew_count_cap", C.c_int64), ("rew_clip", C.c_float)]


class ReplayPrioConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("alpha", C.c_float), ("beta", C.c_float), ("eps", C.c_float), ("cap", C.c_float)]


class Tape(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("volumes", "bid_cents", "x_impressions", "x_cost", "click", "conv", "rev_cents")]
                + [(n, C.c_int64) for n in ("len_bid", "len_ximp", "len_xcost", "len_click", "len_conv", "len_rev")]
                + [(n, C.c_void_p) for n in ("off_bid", "off_ximp", "off_xcost", "off_click", "off_conv", "off_rev")]
                + [(n, C.c_void_p) for n in ("end_bid", "end_ximp", "end_xcost", "end_click", "end_conv", "end_rev")]
                + [("drift_uniforms", C.c_void_p)])


_lib = None
ABI_VERSION, STREAM_REVISION = 5, 5           # include/adcraft_engine.h ADC_ABI_VERSION, ADC_STREAM_REVISION


def library_path():
    return _build.LIB


def lib():
    """Load (building in-tree first if needed) libadcraft_hip.so; raises if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("ADCRAFT_HIP_LIB") or _build.LIB      # (another build of this same library, for A/B timing)
    if path == _build.LIB and (not os.path.exists(path) or _build.stale()):
        try:
            _build.build()
        except Exception as exc:  # no hipcc / compile error: there is nothing to fall back to
            if not os.path.exists(path):
                raise EngineError(f"HIP engine library {path} is missing and could not be built: {exc}") from exc
            # an older build exists but the sources have changed since: running it would silently test stale kernels
            if os.environ.get("ADCRAFT_ALLOW_STALE_LIB") != "1":
                raise EngineError(f"HIP engine library {path} is older than its sources and the rebuild failed: {exc} "
                                  "(set ADCRAFT_ALLOW_STALE_LIB=1 to load the stale library anyway)") from exc
            import warnings
            warnings.warn(f"loading a STALE {path}: its sources changed and the rebuild failed ({exc})", RuntimeWarning)
    L = C.CDLL(path)
    L.adc_last_error.restype = C.c_char_p
    vp, i32, i64, u64, f32, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
    sig = {
        "adc_abi_version": ([], C.c_int),
        "adc_stream_revision": ([], C.c_int),
        "adc_device_count": ([vp], C.c_int),
        "adc_engine_create": ([C.POINTER(Config), C.POINTER(vp)], C.c_int),
        "adc_engine_destroy": ([vp], None),
        "adc_engine_bid_curves_build": ([vp, C.c_int, vp, C.c_int], C.c_int),
        "adc_engine_ideal_step": ([vp, vp, vp], C.c_int),
        "adc_engine_bid_curves_fetch": ([vp, vp, vp], C.c_int),
        "adc_engine_policy_oracle": ([vp, f32], C.c_int),
        "adc_engine_agent_init": ([vp, f32, vp], C.c_int),
        "adc_engine_agent_update": ([vp, vp, vp, vp], C.c_int),
        "adc_engine_agent_act": ([vp, f32, vp], C.c_int),
        "adc_engine_agent_step": ([vp, f32], C.c_int),
        "adc_engine_agent_state": ([vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_interp_init": ([vp, C.c_double, C.c_double, vp, i32, i32, vp], C.c_int),
        "adc_engine_interp_set_allowed_bids": ([vp, vp, i32], C.c_int),
        "adc_engine_interp_update": ([vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_interp_act": ([vp, f32, vp], C.c_int),
        "adc_engine_interp_step": ([vp, f32], C.c_int),
        "adc_engine_interp_state": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_interp_entries": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_get_actions": ([vp, vp, vp], C.c_int),
        "adc_engine_metrics_read_nk": ([vp, vp, vp, vp], C.c_int),
        "adc_engine_run_days": ([vp, C.c_int, i32, f32], C.c_int),
        "adc_engine_day_graph_enable": ([vp, C.c_int], C.c_int),
        "adc_engine_set_params": ([vp, C.c_int, vp], C.c_int),
        "adc_engine_get_params": ([vp, C.c_int, vp], C.c_int),
        "adc_engine_set_env_params": ([vp, C.c_int, vp], C.c_int),
        "adc_engine_reset": ([vp, vp, vp], C.c_int),
        "adc_engine_generate_keywords": ([vp, C.POINTER(Quantiles), f32, C.c_uint32, vp], C.c_int),
        "adc_engine_generate_explicit_keywords": ([vp, C.c_uint32, vp], C.c_int),
        "adc_engine_set_limits": ([vp, i32, f64], C.c_int),
        "adc_engine_set_drift": ([vp, i32, f32, f32, f32], C.c_int),
        "adc_engine_set_drift_mask": ([vp, vp], C.c_int),
        "adc_engine_set_env_drift": ([vp, vp], C.c_int),
        "adc_engine_get_rng_state": ([vp, vp, vp], C.c_int),
        "adc_engine_set_rng_state": ([vp, vp, vp], C.c_int),
        "adc_engine_get_episode_state": ([vp, vp, vp], C.c_int),
        "adc_engine_set_episode_state": ([vp, vp, vp], C.c_int),
        "adc_engine_step": ([vp, vp, vp, C.POINTER(StepOut)], C.c_int),
        "adc_engine_step_device": ([vp, vp, vp], C.c_int),
        "adc_engine_step_async": ([vp, vp, vp, C.POINTER(StepOut)], C.c_int),
        "adc_engine_step_flat_async": ([vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_wait": ([vp], C.c_int),
        "adc_engine_fetch": ([vp, C.POINTER(StepOut)], C.c_int),
        "adc_engine_out_offsets": ([vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "adc_engine_synchronize": ([vp], C.c_int),
        "adc_engine_step_flat": ([vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_step_replay": ([vp, vp, vp, C.POINTER(Tape), C.POINTER(StepOut)], C.c_int),
        "adc_engine_update_keywords": ([vp], C.c_int),
        "adc_engine_set_general_model": ([vp, i32, f32, i32], C.c_int),
        "adc_host_alloc": ([C.c_size_t, C.POINTER(vp)], C.c_int),
        "adc_host_free": ([vp], None),
        "adc_engine_device_buffer": ([vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)], C.c_int),
        "adc_engine_stream": ([vp, C.POINTER(vp)], C.c_int),
        "adc_engine_sample_actions": ([vp, f32, f32, f32], C.c_int),
        "adc_engine_set_flat_actions_device": ([vp, vp], C.c_int),
        "adc_engine_flat_obs_enable": ([vp, C.c_int], C.c_int),
        "adc_engine_profile_enable": ([vp, C.c_int], C.c_int),
        "adc_engine_profile_sample_every": ([vp, C.c_int32], C.c_int),
        "adc_engine_profile_read": ([vp, vp, C.POINTER(i64)], C.c_int),
        "adc_engine_profile_records": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_region_begin": ([vp], C.c_int),
        "adc_engine_region_end": ([vp, C.POINTER(f64)], C.c_int),
        "adc_engine_comm_stats": ([vp, C.POINTER(i64), C.POINTER(f64), C.POINTER(f64), C.c_int], C.c_int),
        "adc_engine_step_kernel_name": ([vp], C.c_char_p),
        "adc_engine_metrics_enable": ([vp, C.c_int], C.c_int),
        "adc_engine_metrics_reset": ([vp], C.c_int),
        "adc_engine_metrics_read": ([vp, vp, vp], C.c_int),
        "adc_engine_ideal_profit": ([vp, C.c_int, vp, C.c_int, vp], C.c_int),
        "adc_bid_curves_from_samples": ([C.c_int, vp, i32, vp, i32, vp, vp], C.c_int),
        "adc_engine_metrics_akncp_ncp": ([vp, f64, vp, vp], C.c_int),
        "adc_engine_bid_curves_contenders": ([vp, vp, vp, C.POINTER(i32)], C.c_int),
        "adc_engine_outcomes_replay": ([vp, i32, i32, vp, f32, i64, vp, vp, vp, vp, C.POINTER(i64), vp], C.c_int),
        "adc_engine_outcomes_replay_tape": ([vp, i32, vp, f32, C.POINTER(Tape), i64, vp, vp, vp, vp, C.POINTER(i64), vp], C.c_int),
        "adc_nth_price_auction": ([C.c_int, f64, vp, i32, i32, i32, i32, C.POINTER(i32), vp, vp], C.c_int),
        "adc_sigmoid": ([f64, f64, f64], f64),
        "adc_clamp": ([f64, f64, f64], f64),
        "adc_threshold_sigmoid": ([f64, f64, f64, f64], f64),
        "adc_sum_f64": ([vp, i64], f64),
        "adc_count_true": ([vp, i64], i64),
        "adc_nonneg_int_normal": ([f64, f64, u64, u64], u64),
        "adc_binomial": ([u64, f64, u64, u64], u64),
        "adc_cost_create": ([f64, i64, u64, u64, vp], C.c_int),
        "adc_auction_word_intervals": ([f32, f32, f32, f32, vp], C.c_int),
        "adc_auction_word_brackets": ([f32, f32, f32, f32, vp], C.c_int),
        "adc_check_win_brackets": ([i64, vp, vp, vp, vp, vp, vp, vp], i64),
        "adc_lower_bound_v_host": ([i64, vp, vp, vp, vp, vp], C.c_int),
        "adc_lower_bound_v_bisect_host": ([i64, vp, vp, vp, vp, vp], C.c_int),
        "adc_win_intervals_host": ([i64, vp, vp, vp, vp, i32, vp, vp], C.c_int),
        "adc_fast_schedule_host": ([vp, i32, i32, vp, i64, vp, vp], i64),
        "adc_sample_random_keyword": ([C.c_uint64, C.c_uint32, C.c_uint32, vp], C.c_int),
        "adc_interp_act_host": ([f32, i32, f32, i32, C.c_double, C.c_double, C.c_double, vp, i32, i32, vp, vp, i32, vp, vp,
                                 C.c_double, vp, vp, vp, vp, vp], C.c_int),
        "adc_interp_key_host": ([f32], C.c_double),
        "adc_engine_mlp_init": ([vp, C.POINTER(MLPConfig), vp], C.c_int),
        "adc_engine_mlp_init_frames": ([vp, C.POINTER(MLPConfig), vp, i32], C.c_int),
        "adc_engine_mlp_frames": ([vp, vp], C.c_int),
        "adc_engine_mlp_history_get": ([vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_history_set": ([vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_init_recurrent": ([vp, C.POINTER(MLPConfig), vp, i32], C.c_int),
        "adc_engine_mlp_gru_width": ([vp, vp], C.c_int),
        "adc_engine_mlp_set_gru": ([vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_set_member_gru": ([vp, i32, vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_hidden_get": ([vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_hidden_set": ([vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_hidden_forget": ([vp], C.c_int),
        "adc_engine_mlp_set_layer": ([vp, i32, i32, vp, vp], C.c_int),
        "adc_engine_mlp_set_norm": ([vp, vp, vp], C.c_int),
        "adc_engine_mlp_set_log_std": ([vp, vp], C.c_int),
        "adc_engine_mlp_set_deterministic": ([vp, i32], C.c_int),
        "adc_engine_mlp_set_squash": ([vp, vp, vp], C.c_int),
        "adc_engine_mlp_learners_set_squash": ([vp, vp, vp], C.c_int),
        "adc_mlp_squash_host": ([i32, vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_set_bounds": ([vp, vp, vp], C.c_int),
        "adc_engine_mlp_learners_set_bounds": ([vp, vp, vp], C.c_int),
        "adc_engine_mlp_set_explore": ([vp, i32], C.c_int),
        "adc_engine_mlp_get_bounds": ([vp, vp, vp, C.POINTER(i32), C.POINTER(i32)], C.c_int),
        "adc_mlp_bounded_host": ([i32, vp, vp, vp, u64, C.c_uint32, i32, vp, vp, vp, vp], C.c_int),
        "adc_mlp_unbox_host": ([i32, vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_act": ([vp, f32, vp], C.c_int),
        "adc_engine_mlp_step": ([vp, f32], C.c_int),
        "adc_engine_mlp_last": ([vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_bootstrap_value": ([vp, vp], C.c_int),
        "adc_engine_mlp_agent_state": ([vp, vp, vp], C.c_int),
        "adc_engine_rollout_enable": ([vp, i32, i32], C.c_int),
        "adc_engine_rollout_reset": ([vp], C.c_int),
        "adc_engine_rollout_fetch": ([vp, C.POINTER(i32), vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_mlp_population": ([vp, i32, vp], C.c_int),
        "adc_engine_mlp_set_member_layer": ([vp, i32, i32, vp, vp], C.c_int),
        "adc_engine_mlp_param_count": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_mlp_get_params": ([vp, vp], C.c_int),
        "adc_engine_mlp_get_member_params": ([vp, i32, vp], C.c_int),
        "adc_engine_mlp_learners": ([vp, i32], C.c_int),
        "adc_engine_mlp_set_learner_layer": ([vp, i32, i32, i32, vp, vp], C.c_int),
        "adc_engine_mlp_set_learner_log_std": ([vp, i32, vp], C.c_int),
        "adc_engine_mlp_get_learner_params": ([vp, i32, vp], C.c_int),
        "adc_engine_es_init": ([vp, C.POINTER(ESConfig)], C.c_int),
        "adc_engine_es_perturb": ([vp], C.c_int),
        "adc_engine_es_fitness": ([vp, vp], C.c_int),
        "adc_engine_es_update": ([vp, vp, C.POINTER(ESStats)], C.c_int),
        "adc_engine_es_state_get": ([vp, vp, vp, vp, C.POINTER(i64)], C.c_int),
        "adc_engine_es_state_set": ([vp, vp, vp, vp, i64], C.c_int),
        "adc_es_config_check": ([C.POINTER(ESConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_es_noise_host": ([u64, C.c_uint32, C.c_uint32, i64, i64, vp], C.c_int),
        "adc_es_update_host": ([C.POINTER(ESConfig), u64, i32, i64, vp, i64, vp, vp, vp, vp], C.c_int),
        "adc_engine_pg_init": ([vp, C.POINTER(PGConfig)], C.c_int),
        "adc_engine_pg_param_count": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_pg_advantages": ([vp], C.c_int),
        "adc_engine_pg_advantages_fetch": ([vp, vp, vp], C.c_int),
        "adc_engine_pg_minibatch": ([vp, i32, i32, C.POINTER(PGStats)], C.c_int),
        "adc_engine_pg_update": ([vp, i32, C.POINTER(PGStats)], C.c_int),
        "adc_engine_pg_state_get": ([vp, vp, vp, vp, C.POINTER(i64)], C.c_int),
        "adc_engine_pg_state_set": ([vp, vp, vp, vp, i64], C.c_int),
        "adc_pg_pop_config_check": ([C.POINTER(PGConfig), i32, i32, i32, C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_pg_pop_init": ([vp, C.POINTER(PGConfig), i32], C.c_int),
        "adc_engine_pg_pop_advantages": ([vp], C.c_int),
        "adc_engine_pg_pop_advantages_fetch": ([vp, vp, vp], C.c_int),
        "adc_engine_pg_pop_minibatch": ([vp, i32, C.POINTER(PGStats)], C.c_int),
        "adc_engine_pg_pop_update": ([vp, i32, C.POINTER(PGStats)], C.c_int),
        "adc_engine_pg_pop_state_get": ([vp, i32, vp, vp, vp, C.POINTER(i64)], C.c_int),
        "adc_engine_pg_pop_state_set": ([vp, i32, vp, vp, vp, i64], C.c_int),
        "adc_engine_pg_pop_set_config": ([vp, i32, C.POINTER(PGConfig)], C.c_int),
        "adc_engine_pg_pop_copy": ([vp, i32, i32], C.c_int),
        "adc_pg_config_check": ([C.POINTER(PGConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_pg_gae_host": ([C.POINTER(PGConfig), i32, i32, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_pg_param_count_host": ([C.POINTER(MLPConfig), i32, C.POINTER(i64)], C.c_int),
        "adc_pg_grad_host": ([C.POINTER(MLPConfig), i32, C.POINTER(PGConfig), vp, i64, vp, vp, vp, vp, vp, vp, vp, vp,
                              C.POINTER(PGStats)], C.c_int),
        "adc_pg_step_host": ([C.POINTER(PGConfig), i64, i64, vp, vp, vp, vp], C.c_int),
        "adc_pg_kl_config_check": ([C.POINTER(PGKLConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_pg_kl_init": ([vp, C.POINTER(PGKLConfig), i32], C.c_int),
        "adc_engine_pg_kl_stats": ([vp, C.POINTER(PGKLStats)], C.c_int),
        "adc_engine_pg_kl_coef_get": ([vp, i32, C.POINTER(f32)], C.c_int),
        "adc_engine_pg_kl_coef_set": ([vp, i32, f32], C.c_int),
        "adc_engine_pg_kl_old_dist_fetch": ([vp, vp, vp], C.c_int),
        "adc_pg_kl_grad_host": ([C.POINTER(MLPConfig), i32, C.POINTER(PGConfig), vp, i64, vp, vp, vp, vp, vp, vp, C.POINTER(PGKLConfig), f32, vp, vp, i32,
                                 vp, vp, vp, C.POINTER(PGStats), C.POINTER(PGKLStats)], C.c_int),
        "adc_pg_kl_adapt_host": ([C.POINTER(PGKLConfig), f32, f64, C.POINTER(f32)], C.c_int),
        "adc_pg_shuffle_config_check": ([C.POINTER(PGShuffleConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_pg_shuffle_init": ([vp, C.POINTER(PGShuffleConfig), i32], C.c_int),
        "adc_engine_pg_shuffle_epoch": ([vp], C.c_int),
        "adc_engine_pg_shuffle_minibatch": ([vp, i32, C.POINTER(PGStats)], C.c_int),
        "adc_engine_pg_shuffle_order_fetch": ([vp, vp, vp], C.c_int),
        "adc_engine_pg_shuffle_stats": ([vp, C.POINTER(PGShuffleStats)], C.c_int),
        "adc_pg_shuffle_order_host": ([C.c_uint64, i64, C.c_uint32, vp], C.c_int),
        "adc_pg_shuffle_stop_host": ([f64, f32, C.POINTER(i32)], C.c_int),
        "adc_pg_decide_host": ([C.POINTER(PGConfig), f32, vp, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(f32)], C.c_int),
        "adc_engine_pg_update_queued": ([vp, i32, C.POINTER(PGStats)], C.c_int),
        "adc_engine_pg_pop_update_queued": ([vp, i32, C.POINTER(PGStats)], C.c_int),
        "adc_engine_teach_days": ([vp, C.c_int, i32, f32], C.c_int),
        "adc_engine_dagger_days": ([vp, C.c_int, i32, f32, f32], C.c_int),
        "adc_engine_dagger_mask_fetch": ([vp, vp], C.c_int),
        "adc_dagger_coin_host": ([u64, C.c_uint32, f32], C.c_int),
        "adc_im_config_check": ([C.POINTER(IMConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_im_init": ([vp, C.POINTER(IMConfig)], C.c_int),
        "adc_engine_im_advantages": ([vp, vp, vp], C.c_int),
        "adc_engine_im_minibatch": ([vp, i32, i32, C.POINTER(IMStats)], C.c_int),
        "adc_engine_im_update": ([vp, i32, C.POINTER(IMStats)], C.c_int),
        "adc_engine_im_state_get": ([vp, C.POINTER(f64), C.POINTER(i64)], C.c_int),
        "adc_engine_im_state_set": ([vp, f64, i64], C.c_int),
        "adc_im_weight_host": ([C.POINTER(IMConfig), i64, vp, C.POINTER(f64), C.POINTER(f32), vp], C.c_int),
        "adc_im_grad_host": ([C.POINTER(MLPConfig), i32, C.POINTER(IMConfig), f32, vp, i64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(IMStats)], C.c_int),
        "adc_engine_td3_init": ([vp, C.POINTER(TD3Config)], C.c_int),
        "adc_engine_td3_set_critic_layer": ([vp, i32, i32, vp, vp], C.c_int),
        "adc_engine_td3_set_action_norm": ([vp, vp, vp], C.c_int),
        "adc_engine_td3_set_bounded": ([vp, i32], C.c_int),
        "adc_engine_td3_pop_set_bounded": ([vp, i32], C.c_int),
        "adc_engine_td3_get_bounded": ([vp, C.POINTER(i32)], C.c_int),
        "adc_td3_bounded_target_host": ([C.POINTER(MLPConfig), i32, C.POINTER(TD3Config), u64, i64, vp, vp, i32, vp, vp, vp, vp], C.c_int),
        "adc_td3_bounded_actor_grad_host": ([C.POINTER(MLPConfig), i32, C.POINTER(TD3Config), vp, vp, i32, vp, vp, vp], C.c_int),
        "adc_engine_td3_sync_targets": ([vp], C.c_int),
        "adc_engine_td3_store": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_td3_buffer_info": ([vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_engine_td3_buffer_fetch": ([vp, i64, i64, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_td3_buffer_load": ([vp, i64, i64, vp, vp, vp, vp, vp, i64], C.c_int),
        "adc_engine_td3_batch_size": ([vp, C.POINTER(i32)], C.c_int),
        "adc_engine_td3_batch_indices": ([vp, i64, vp], C.c_int),
        "adc_engine_td3_update": ([vp, i32, C.POINTER(TD3Stats)], C.c_int),
        "adc_engine_td3_param_counts": ([vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_engine_td3_state_get": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_engine_td3_state_set": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64], C.c_int),
        "adc_engine_sac_init": ([vp, C.POINTER(SACConfig)], C.c_int),
        "adc_engine_sac_set_critic_layer": ([vp, i32, i32, vp, vp], C.c_int),
        "adc_engine_sac_sync_targets": ([vp], C.c_int),
        "adc_engine_sac_store": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_sac_buffer_info": ([vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_engine_sac_buffer_fetch": ([vp, i64, i64, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_sac_buffer_load": ([vp, i64, i64, vp, vp, vp, vp, vp, i64], C.c_int),
        "adc_engine_sac_batch_size": ([vp, C.POINTER(i32)], C.c_int),
        "adc_engine_sac_batch_indices": ([vp, i64, vp], C.c_int),
        "adc_engine_sac_update": ([vp, i32, C.POINTER(SACStats)], C.c_int),
        "adc_engine_sac_param_counts": ([vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_engine_sac_state_get": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64)], C.c_int),
        "adc_engine_sac_state_set": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, i64], C.c_int),
        "adc_sac_config_check": ([C.POINTER(SACConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_sac_param_counts_host": ([C.POINTER(MLPConfig), i32, C.POINTER(SACConfig), C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_sac_logp_host": ([C.POINTER(MLPConfig), i32, f32, i32, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_sac_target_host": ([C.POINTER(MLPConfig), i32, C.POINTER(SACConfig), u64, i64, f32, vp, vp, i32, vp, vp, vp, vp, vp], C.c_int),
        "adc_sac_critic_grad_host": ([C.POINTER(MLPConfig), i32, C.POINTER(SACConfig), vp, i32, vp, vp, vp, vp, vp], C.c_int),
        "adc_sac_actor_grad_host": ([C.POINTER(MLPConfig), i32, C.POINTER(SACConfig), u64, i64, f32, vp, vp, i32, vp, vp, vp, vp], C.c_int),
        "adc_sac_alpha_step_host": ([C.POINTER(SACConfig), i64, f64, i32, vp, C.POINTER(f32)], C.c_int),
        "adc_sac_log_alpha_init_host": ([f32], f32),
        "adc_td3_pop_config_check": ([C.POINTER(TD3Config), i32, i32, i32, C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_td3_pop_init": ([vp, C.POINTER(TD3Config), i32], C.c_int),
        "adc_engine_td3_pop_set_critic_layer": ([vp, i32, i32, i32, vp, vp], C.c_int),
        "adc_engine_td3_pop_set_action_norm": ([vp, vp, vp], C.c_int),
        "adc_engine_td3_pop_sync_targets": ([vp, i32], C.c_int),
        "adc_engine_td3_pop_store": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_td3_pop_buffer_info": ([vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)], C.c_int),
        "adc_engine_td3_pop_buffer_fetch": ([vp, i32, i64, i64, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_td3_pop_buffer_load": ([vp, i32, i64, i64, vp, vp, vp, vp, vp, i64], C.c_int),
        "adc_engine_td3_pop_batch_indices": ([vp, i32, i64, vp], C.c_int),
        "adc_engine_td3_pop_update": ([vp, i32, C.POINTER(TD3Stats)], C.c_int),
        "adc_engine_td3_pop_param_counts": ([vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_engine_td3_pop_state_get": ([vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_engine_td3_pop_state_set": ([vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64], C.c_int),
        "adc_engine_td3_pop_set_config": ([vp, i32, C.POINTER(TD3Config)], C.c_int),
        "adc_engine_td3_pop_copy": ([vp, i32, i32, i32], C.c_int),
        "adc_sac_pop_config_check": ([C.POINTER(SACConfig), i32, i32, i32, C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_sac_pop_init": ([vp, C.POINTER(SACConfig), i32], C.c_int),
        "adc_engine_sac_pop_set_critic_layer": ([vp, i32, i32, i32, vp, vp], C.c_int),
        "adc_engine_sac_pop_sync_targets": ([vp, i32], C.c_int),
        "adc_engine_sac_pop_store": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_sac_pop_buffer_info": ([vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i32)], C.c_int),
        "adc_engine_sac_pop_buffer_fetch": ([vp, i32, i64, i64, vp, vp, vp, vp, vp], C.c_int),
        "adc_engine_sac_pop_buffer_load": ([vp, i32, i64, i64, vp, vp, vp, vp, vp, i64], C.c_int),
        "adc_engine_sac_pop_batch_indices": ([vp, i32, i64, vp], C.c_int),
        "adc_engine_sac_pop_update": ([vp, i32, C.POINTER(SACStats)], C.c_int),
        "adc_engine_sac_pop_param_counts": ([vp, C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_engine_sac_pop_state_get": ([vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i64)], C.c_int),
        "adc_engine_sac_pop_state_set": ([vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64], C.c_int),
        "adc_engine_sac_pop_set_config": ([vp, i32, C.POINTER(SACConfig)], C.c_int),
        "adc_engine_sac_pop_copy": ([vp, i32, i32, i32], C.c_int),
        "adc_td3_config_check": ([C.POINTER(TD3Config), C.POINTER(C.c_char_p)], C.c_int),
        "adc_pbt_config_check": ([C.POINTER(PBTConfig), i32, i32, C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_pbt_init": ([vp, C.POINTER(PBTConfig)], C.c_int),
        "adc_engine_pbt_init_sac": ([vp, C.POINTER(PBTConfig)], C.c_int),
        "adc_engine_pbt_fitness": ([vp, vp], C.c_int),
        "adc_engine_pbt_exploit": ([vp, vp], C.c_int),
        "adc_engine_pbt_step": ([vp, vp, C.POINTER(PBTResult)], C.c_int),
        "adc_engine_pbt_state_get": ([vp, C.POINTER(i64), vp], C.c_int),
        "adc_engine_pbt_state_set": ([vp, i64, vp], C.c_int),
        "adc_pbt_fitness_host": ([i32, i32, i32, vp, vp], C.c_int),
        "adc_pbt_plan_host": ([C.POINTER(PBTConfig), u64, i32, i64, vp, vp, vp, vp, vp], C.c_int),
        "adc_pbt_explore_host": ([C.POINTER(PBTConfig), i32, C.c_uint32, vp, vp, vp], C.c_int),
        "adc_obs_norm_config_check": ([C.POINTER(ObsNormConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_obs_norm_init": ([vp, C.POINTER(ObsNormConfig)], C.c_int),
        "adc_engine_obs_norm_update": ([vp], C.c_int),
        "adc_engine_obs_norm_state_get": ([vp, i32, C.POINTER(i64), vp, vp, vp, vp], C.c_int),
        "adc_engine_obs_norm_state_set": ([vp, i32, i64, vp, vp, vp, vp], C.c_int),
        "adc_engine_obs_norm_copy": ([vp, vp], C.c_int),
        "adc_obs_norm_host": ([C.POINTER(ObsNormConfig), i64, i32, vp, C.POINTER(i64), vp, vp, vp, vp], C.c_int),
        "adc_rew_norm_config_check": ([C.POINTER(RewNormConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_rew_norm_init": ([vp, C.POINTER(RewNormConfig)], C.c_int),
        "adc_engine_rew_norm_update": ([vp], C.c_int),
        "adc_engine_rew_norm_state_get": ([vp, i32, C.POINTER(i64), C.POINTER(f64), C.POINTER(f64), C.POINTER(f32)], C.c_int),
        "adc_engine_rew_norm_state_set": ([vp, i32, i64, f64, f64, f32], C.c_int),
        "adc_engine_rew_norm_returns_get": ([vp, vp], C.c_int),
        "adc_engine_rew_norm_returns_set": ([vp, vp], C.c_int),
        "adc_engine_rew_norm_copy": ([vp, vp], C.c_int),
        "adc_td3_norm_config_check": ([C.POINTER(TD3NormConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_td3_norm_init": ([vp, C.POINTER(TD3NormConfig)], C.c_int),
        "adc_engine_td3_norm_update": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_td3_norm_state_get": ([vp, i32, C.POINTER(i64), vp, vp, vp, vp, C.POINTER(i64), C.POINTER(f64), C.POINTER(f64), C.POINTER(f32)], C.c_int),
        "adc_engine_td3_norm_state_set": ([vp, i32, i64, vp, vp, vp, vp, i64, f64, f64, f32], C.c_int),
        "adc_engine_td3_norm_returns_get": ([vp, vp], C.c_int),
        "adc_engine_td3_norm_returns_set": ([vp, vp], C.c_int),
        "adc_engine_td3_norm_copy": ([vp, vp], C.c_int),
        "adc_td3_norm_obs_host": ([C.POINTER(TD3NormConfig), i64, i32, vp, C.POINTER(i64), vp, vp, vp, vp], C.c_int),
        "adc_td3_norm_rew_host": ([C.POINTER(TD3NormConfig), i32, i32, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(f64), C.POINTER(f64), C.POINTER(f32), vp], C.c_int),
        "adc_sac_norm_config_check": ([C.POINTER(SACNormConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_sac_norm_init": ([vp, C.POINTER(SACNormConfig)], C.c_int),
        "adc_engine_sac_norm_update": ([vp, C.POINTER(i64)], C.c_int),
        "adc_engine_sac_norm_state_get": ([vp, i32, C.POINTER(i64), vp, vp, vp, vp, C.POINTER(i64), C.POINTER(f64), C.POINTER(f64), C.POINTER(f32)], C.c_int),
        "adc_engine_sac_norm_state_set": ([vp, i32, i64, vp, vp, vp, vp, i64, f64, f64, f32], C.c_int),
        "adc_engine_sac_norm_returns_get": ([vp, vp], C.c_int),
        "adc_engine_sac_norm_returns_set": ([vp, vp], C.c_int),
        "adc_engine_sac_norm_copy": ([vp, vp], C.c_int),
        "adc_sac_y_norm_host": ([C.POINTER(SACConfig), i32, vp, vp, vp, vp, f32, f32, f32, vp], C.c_int),
        "adc_replay_prio_config_check": ([C.POINTER(ReplayPrioConfig), C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_replay_prio_init": ([vp, C.POINTER(ReplayPrioConfig)], C.c_int),
        "adc_engine_replay_prio_set_beta": ([vp, f32], C.c_int),
        "adc_engine_replay_prio_info": ([vp, i32, C.POINTER(f64), C.POINTER(f32)], C.c_int),
        "adc_engine_replay_prio_fetch": ([vp, i32, i64, i64, vp], C.c_int),
        "adc_engine_replay_prio_load": ([vp, i32, i64, i64, vp, f32], C.c_int),
        "adc_engine_replay_prio_batch": ([vp, i32, i64, vp, vp], C.c_int),
        "adc_replay_nstep_check": ([i32, C.POINTER(C.c_char_p)], C.c_int),
        "adc_engine_replay_nstep_init": ([vp, i32], C.c_int),
        "adc_engine_replay_nstep_info": ([vp, C.POINTER(i32)], C.c_int),
        "adc_engine_replay_nstep_fetch": ([vp, i32, i64, i64, vp], C.c_int),
        "adc_engine_replay_nstep_load": ([vp, i32, i64, i64, vp], C.c_int),
        "adc_replay_nstep_host": ([i32, f32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_td3_y_nstep_host": ([C.POINTER(TD3Config), i32, vp, vp, vp, vp, f32, f32, vp], C.c_int),
        "adc_sac_y_nstep_host": ([C.POINTER(SACConfig), i32, vp, vp, vp, vp, vp, f32, f32, f32, vp], C.c_int),
        "adc_per_tree_host": ([i64, vp, vp, vp], C.c_int),
        "adc_per_descend_host": ([i64, vp, f64, C.POINTER(i64)], C.c_int),
        "adc_per_sample_host": ([C.POINTER(ReplayPrioConfig), i64, i64, vp, u64, i64, i32, vp, vp], C.c_int),
        "adc_per_priority_host": ([C.POINTER(ReplayPrioConfig), i32, vp, vp, vp], C.c_int),
        "adc_per_leaf_update_host": ([i64, vp, C.POINTER(f32), i32, vp, vp], C.c_int),
        "adc_td3_y_norm_host": ([C.POINTER(TD3Config), i32, vp, vp, vp, f32, f32, vp], C.c_int),
        "adc_rew_norm_host": ([C.POINTER(RewNormConfig), i32, i32, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(f64), C.POINTER(f64), C.POINTER(f32), vp], C.c_int),
        "adc_pg_gae_norm_host": ([C.POINTER(PGConfig), i32, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp], C.c_int),
        "adc_td3_param_counts_host": ([C.POINTER(MLPConfig), i32, C.POINTER(TD3Config), C.POINTER(i64), C.POINTER(i64)], C.c_int),
        "adc_td3_batch_indices_host": ([u64, i64, i64, i32, vp], C.c_int),
        "adc_td3_target_host": ([C.POINTER(MLPConfig), i32, C.POINTER(TD3Config), u64, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp], C.c_int),
        "adc_td3_critic_grad_host": ([C.POINTER(MLPConfig), i32, C.POINTER(TD3Config), vp, vp, vp, i32, vp, vp, vp, vp, vp], C.c_int),
        "adc_td3_actor_grad_host": ([C.POINTER(MLPConfig), i32, C.POINTER(TD3Config), vp, vp, vp, vp, i32, vp, vp, vp], C.c_int),
        "adc_td3_polyak_host": ([f32, i64, vp, vp], C.c_int),
        "adc_mlp_config_check": ([C.POINTER(MLPConfig), i32, C.POINTER(C.c_char_p)], C.c_int),
        "adc_mlp_stack_row_host": ([i32, i32, vp, vp, vp, vp, i32, i32, vp], C.c_int),
        "adc_mlp_act_host": ([C.POINTER(MLPConfig), i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, C.c_uint32, f32,
                              vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_gru_cell_host": ([i32, i32, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_mlp_act_recurrent_host": ([C.POINTER(MLPConfig), i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, C.c_uint32, f32,
                                        vp, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "adc_gru_state_host": ([i32, i32, vp, vp, vp, vp, vp], C.c_int),
        "adc_mlp_math_host": ([i32, f32], f32),
        "adc_mlp_math_sweep_host": ([i32, f32, f32, vp, vp], i64),
        "adc_mlp_agent_key_host": ([u64], u64),
        "adc_mlp_default_agent_key_host": ([u64, u64], u64),
        "adc_explicit_curve_host": ([C.c_uint64, C.c_uint32, i32, i32, f32, f32, f32, vp, i32, vp, vp, vp], C.c_int),
        "adc_debug_win_brackets_device": ([C.c_int, i64, vp, vp, vp, vp, vp], C.c_int),
        "adc_debug_philox_device": ([C.c_int, i64, vp, vp, vp], C.c_int),
        "adc_debug_walk_stats": ([vp, vp, C.c_int], C.c_int),
        "adc_debug_direct_days": ([vp, vp, C.c_int], C.c_int),
        "adc_debug_chain_device": ([C.c_int, f64, i64, vp, vp], C.c_int),
        "adc_engine_env_groups": ([vp, vp], C.c_int),
        "adc_engine_set_env_groups": ([vp, C.c_int32], C.c_int),
        "adc_comm_get_unique_id": ([vp], C.c_int),
        "adc_engine_comm_init": ([vp, vp, i32, i32], C.c_int),
        "adc_engine_comm_destroy": ([vp], C.c_int),
        "adc_engine_comm_info": ([vp, vp, vp], C.c_int),
        "adc_engine_metrics_allreduce": ([vp, vp, vp, vp], C.c_int),
        "adc_engine_comm_allreduce_f64": ([vp, vp, i32, i32], C.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)      # AttributeError here = the .so does not export what the header declares
        fn.argtypes = args
        fn.restype = res
    if L.adc_abi_version() != ABI_VERSION or L.adc_stream_revision() != STREAM_REVISION:
        raise EngineError(f"{path}: ABI version {L.adc_abi_version()} / stream revision {L.adc_stream_revision()}, this package "
                          f"expects {ABI_VERSION} / {STREAM_REVISION} (a stale build?)")
    _lib = L
    return L


EXPORTED = None  # filled by tests from include/adcraft_engine.h


def check(rc):
    """Map adc_status to the exceptions the reference's callers see (SURVEY 8b error conventions)."""
    if rc == ADC_OK:
        return
    msg = (lib().adc_last_error() or b"").decode("utf-8", "replace")
    if rc == ADC_EINVAL:
        raise ValueError(msg)
    if rc == ADC_ESTATE:
        raise EngineStateError(msg)        # (an AssertionError: gymnasium_kw_env.py:194-196 asserts on step-before-reset)
    if rc == ADC_ENOMEM:
        raise MemoryError(msg)
    if rc == ADC_ETYPE:
        raise TypeError(msg)
    raise EngineError(msg)


def ptr(a):
    return None if a is None else a.ctypes.data


def device_count():
    n = C.c_int(0)
    rc = lib().adc_device_count(C.byref(n))
    return n.value if rc == ADC_OK else 0
