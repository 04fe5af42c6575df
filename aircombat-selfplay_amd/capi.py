"""ctypes binding of include/aircombat.h (the C ABI of libaircombat_hip.so).

The HIP library is the only implementation: there is no CPU fallback. If it is missing, loading raises
``HipExtensionMissing`` — build it with ``python -c "import __graft_entry__ as g; g.build()"``.
"""
import ctypes as C
import os

AC_MAX_AGENTS = 8
AC_MAX_MISSILES_PER_AGENT = 4
AC_STATE_LEN = 128

AC_TASK_HEADING, AC_TASK_SINGLECOMBAT, AC_TASK_DODGE_MISSILE, AC_TASK_SHOOT_MISSILE, AC_TASK_MULTICOMBAT = 0, 1, 2, 3, 4
AC_TASK_SCENARIO1, AC_TASK_SCENARIO_NVN, AC_TASK_WVR, AC_TASK_MANEUVER = 5, 6, 7, 8
AC_ALIVE, AC_CRASH, AC_SHOTDOWN = 0, 1, 2
AC_CTL_FAST, AC_CTL_FP32 = 0, 1   # AcConfig.controller_precision: the low-level controller's arithmetic
AC_CENT_EXPLICIT, AC_CENT_ENV_SHARE = 0, 1   # the MAPPO critic's input: explicit cent_obs rows, or each env's obs block (include/aircombat.h)
AC_POOL_PPO, AC_POOL_MAPPO = 0, 1   # the form of a DevicePolicyPool's members


class HipExtensionMissing(RuntimeError):
    pass


# ---- include/aircombat_buffer.h
(AC_BUF_OBS, AC_BUF_SHARE_OBS, AC_BUF_ACTIONS, AC_BUF_REWARDS, AC_BUF_MASKS, AC_BUF_BAD_MASKS, AC_BUF_ACTIVE_MASKS, AC_BUF_LOGP,
 AC_BUF_VALUES, AC_BUF_RETURNS, AC_BUF_RNN_ACTOR, AC_BUF_RNN_CRITIC, AC_BUF_ADVANTAGES, AC_BUF_NFIELDS) = range(14)
# ---- include/aircombat_epoch.h: the fields of a mini-batch, named as AcBufferBatch's members and in their order
AC_EPOCH_FIELDS = ("obs", "share_obs", "actions", "masks", "active_masks", "action_log_probs", "advantages", "returns", "value_preds",
                   "rnn_states_actor", "rnn_states_critic")
AC_EPOCH_NFIELDS = len(AC_EPOCH_FIELDS)


class AcBufferConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("buffer_size", "n_envs", "n_agents", "obs_dim", "share_obs_dim", "act_dim", "logp_dim",
                                         "hidden_layers", "hidden_size", "use_gae", "use_proper_time_limits")] + \
               [("gamma", C.c_double), ("gae_lambda", C.c_double)]


class AcBufferStep(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "actions", "rewards", "masks", "action_log_probs", "value_preds", "rnn_states_actor",
                                          "rnn_states_critic", "bad_masks", "share_obs", "active_masks")]


class AcBufferBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "share_obs", "actions", "masks", "active_masks", "action_log_probs", "advantages", "returns",
                                          "value_preds", "rnn_states_actor", "rnn_states_critic")]


# ---- include/aircombat_rollout.h
AC_ROLLOUT_NO_OPPONENT, AC_ROLLOUT_OPPONENT_POLICY, AC_ROLLOUT_OPPONENT_POOL = 0, 1, 2


class AcRolloutConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("na", "opponent_kind", "learner_deterministic", "opponent_deterministic")]


class AcRolloutPostStep(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "A", "na", "obs_dim", "env_act_dim", "act_dim", "hidden", "T", "s")] + \
               [(n, C.c_void_p) for n in ("obs", "rewards", "actions", "dones", "OBS", "REWARDS", "ACTIONS", "MASKS", "RNN_ACTOR", "RNN_CRITIC",
                                          "opp_h", "opp_masks")]


# ---- include/aircombat_rollout_share.h (its config is AcRolloutConfig)
class AcShareRolloutPostStep(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "A", "na", "obs_dim", "env_act_dim", "act_dim", "hidden", "T", "s")] + \
               [(n, C.c_void_p) for n in ("obs", "rewards", "actions", "dones", "logp", "OBS", "SHARE_OBS", "REWARDS", "ACTIONS", "LOGP", "MASKS",
                                          "ACTIVE_MASKS", "RNN_ACTOR", "RNN_CRITIC", "opp_h", "opp_masks")]


# ---- include/aircombat_eval.h
AC_EVAL_NO_OPPONENT, AC_EVAL_OPPONENT_POLICY, AC_EVAL_OPPONENT_POOL, AC_EVAL_MAX_EPISODES = 0, 1, 2, 64


class AcEvalConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("na", "opponent_kind", "learner_deterministic", "opponent_deterministic", "episodes_per_env")]


class AcEvalState(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "A", "na", "K", "step", "pad_")] + \
               [(n, C.c_void_p) for n in ("lrn_h", "lrn_masks", "opp_h", "opp_masks", "cum", "len", "count", "log_ret", "log_len", "log_end",
                                          "remaining")]


class AcEvalPostStep(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "A", "na", "hidden", "K", "step")] + \
               [(n, C.c_void_p) for n in ("rewards", "dones", "lrn_h", "lrn_masks", "opp_h", "opp_masks", "cum", "len", "count", "log_ret",
                                          "log_len", "log_end", "remaining")]


class AcLeagueConfig(C.Structure):
    """ac_league_config_t (include/aircombat_league.h)"""
    _fields_ = [("episodes_per_env", C.c_int32), ("deterministic", C.c_int32), ("win_margin", C.c_float), ("pad_", C.c_int32)]


class AcLeagueState(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "A", "K", "C", "step", "pad_")] + \
               [(n, C.c_void_p) for n in ("h", "masks", "cum", "len", "count", "log_ret", "log_len", "log_end", "log_code", "members2",
                                          "remaining")]


class AcLeaguePostStep(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "A", "hidden", "K", "step", "pad_")] + \
               [(n, C.c_void_p) for n in ("rewards", "dones", "info", "h", "masks", "cum", "len", "count", "log_ret", "log_len", "log_end",
                                          "log_code", "remaining")]


class AcLeagueCell(C.Structure):
    """ac_league_cell_t: one cell of the payoff table, 64 bytes"""
    _fields_ = [(n, C.c_int64) for n in ("episodes", "wins_a", "wins_b", "draws", "timeouts", "steps")] + [("sum_a", C.c_double), ("sum_b", C.c_double)]


class AcLeagueTableArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("E", "A", "K", "C")] + [("margin", C.c_float), ("pad_", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("log_ret", "log_len", "log_code", "count", "members2", "out")]


AC_LEAGUE_MAX_EPISODES = 64
AC_DONE_TIMEOUT = 7


class AcInitState(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("lon_deg", "lat_geod_deg", "h_sl_ft", "psi_deg", "u_fps", "v_fps", "w_fps",
                 "p_rad_sec", "q_rad_sec", "r_rad_sec")]


class AcConfig(C.Structure):
    _fields_ = [
        ("task", C.c_int32), ("n_agents", C.c_int32), ("n_ego", C.c_int32), ("sim_freq", C.c_int32),
        ("agent_interaction_steps", C.c_int32), ("max_steps", C.c_int32),
        ("center_lon", C.c_double), ("center_lat", C.c_double), ("center_alt", C.c_double),
        ("altitude_limit", C.c_double), ("acc_limit_x", C.c_double), ("acc_limit_y", C.c_double), ("acc_limit_z", C.c_double),
        ("init", AcInitState * AC_MAX_AGENTS), ("num_missiles", C.c_int32 * AC_MAX_AGENTS),
        ("posture_scale", C.c_double), ("posture_potential", C.c_int32),
        ("altitude_scale", C.c_double), ("altitude_potential", C.c_int32),
        ("event_scale", C.c_double), ("event_potential", C.c_int32),
        ("missile_posture_scale", C.c_double),
        ("shoot_penalty_scale", C.c_double), ("shoot_penalty_potential", C.c_int32),
        ("alt_safe", C.c_double), ("alt_danger", C.c_double), ("alt_kv", C.c_double),
        ("max_attack_angle", C.c_double), ("max_attack_distance", C.c_double), ("min_attack_interval", C.c_int32),
        ("use_artillery", C.c_int32),
        ("heading_scale", C.c_double), ("heading_potential", C.c_int32),
        ("max_heading_increment", C.c_double), ("max_altitude_increment", C.c_double),
        ("max_velocities_u_increment", C.c_double), ("check_interval", C.c_double),
        ("legacy_obs", C.c_int32),
        ("rwr", C.c_int32),
        ("use_baseline", C.c_int32),
        ("hierarchical", C.c_int32), ("approach", C.c_int32),
        ("controller_precision", C.c_int32),
    ]


AC_NET_MAX_BLOCKS = 4
AC_NET_MAX_PARAMS = 64


class AcActHeads(C.Structure):
    """ac_act_heads_t: the training action heads' configuration (ac_act_eval_*)."""
    _fields_ = [("n_cat", C.c_int32), ("nvec", C.c_int32 * 8), ("n_shoot_cols", C.c_int32)]


class AcNet(C.Structure):
    """ac_net_t: one network of the policy as the chains read it (ac_actor_eval_*, ac_critic_*)."""
    _fields_ = [("obs_dim", C.c_int32), ("feature_norm", C.c_int32), ("base_blocks", C.c_int32), ("head_blocks", C.c_int32), ("heads", AcActHeads),
                ("mlp_products", C.c_int32), ("gru_products", C.c_int32), ("gru_dense_products", C.c_int32), ("feature_norm_eps", C.c_float),
                ("block_eps", C.c_float * (2 * AC_NET_MAX_BLOCKS)), ("gru_eps", C.c_float), ("params", C.c_void_p * AC_NET_MAX_PARAMS)]


class AcOptimEntry(C.Structure):
    """ac_optim_entry_t: one tensor of the optimiser's table (ac_optim_*)."""
    _fields_ = [(n, C.c_void_p) for n in ("p", "g", "m", "v")] + [("numel", C.c_int64), ("group", C.c_int32), ("first_chunk", C.c_int32)] + \
               [(n, C.c_double) for n in ("lr", "eps", "beta1", "beta2", "bias_correction1", "bias_correction2")]


class AcRecorderColumn(C.Structure):
    """ac_recorder_column_t (include/aircombat_record.h)."""
    _fields_ = [("name", C.c_char * 16), ("elem_size", C.c_int32), ("count", C.c_int32)]


class AcRecorderLayout(C.Structure):
    """ac_recorder_layout_t: the flight recorder's column table for one handle shape."""
    _fields_ = [("n_columns", C.c_int32), ("bytes_per_aircraft_frame", C.c_int32), ("columns", AcRecorderColumn * 8)]


class AcRecorderInfo(C.Structure):
    """ac_recorder_info_t."""
    _fields_ = [(n, C.c_int32) for n in ("task", "A", "msl_slots", "has_ext", "E", "S", "F", "attached")] + [("count", C.c_int64), ("bytes", C.c_int64)]


AC_REC_DONE, AC_REC_AFTER_RESET = 1, 2


# ---- include/aircombat_spawn.h
AC_SPAWN_FIXED, AC_SPAWN_AUTO = 0, 1
AC_SPAWN_AT, AC_SPAWN_UPTO = 0, 1
AC_SPAWN_MAX_BANK, AC_SPAWN_MAX_WINDOW = 1024, 32


class AcSpawnConfig(C.Structure):
    """ac_spawn_config_t: the spawn curriculum's mode, rule and sampling."""
    _fields_ = [(n, C.c_int32) for n in ("mode", "sample", "window", "min_wins")] + [("win_return", C.c_float), ("pad_", C.c_int32), ("seed", C.c_uint64)]


class AcSpawnState(C.Structure):
    """ac_spawn_state_t: device pointers of the per-env arrays."""
    _fields_ = [("E", C.c_int32), ("K", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("stage", "spawned", "episode", "ret_acc", "wins", "played", "return_sum")]


class AcSpawnPostStep(C.Structure):
    """ac_spawn_post_step_t: one step of the rule on host arrays (ac_spawn_post_step_host)."""
    _fields_ = [(n, C.c_int32) for n in ("E", "A", "n_ego", "K", "all_envs", "pad_")] + [("cfg", AcSpawnConfig)] + \
               [(n, C.c_void_p) for n in ("rewards", "info", "stage", "spawned", "episode", "ret_acc", "wins", "played", "return_sum", "index")]


# ---- include/aircombat_mutual.h
AC_MI_HIDDEN, AC_MI_WIDTH, AC_MI_MAX_ACT, AC_MI_MAX_OBS = 128, 256, 12, 128
AC_MI_WEIGHTS = ("p_w0", "p_b0", "p_w1", "p_b1", "p_w2", "p_b2", "q_w0", "q_b0", "q_w1", "q_b1", "q_w2", "q_b2")


class AcMiScore(C.Structure):
    """ac_mi_score_t: the mutual-support scorer's arguments."""
    _fields_ = [(n, C.c_int32) for n in ("E", "na", "T", "obs_dim", "act_dim", "hidden", "s0", "n", "add")] + [("ratio", C.c_float)] + \
               [(n, C.c_void_p) for n in ("OBS", "ACTIONS", "RNN_ACTOR", "REWARDS") + AC_MI_WEIGHTS + ("r_int", "mse")]


class AcMiGather(C.Structure):
    """ac_mi_gather_t: the gather of one discriminator mini-batch."""
    _fields_ = [(n, C.c_int32) for n in ("E", "na", "T", "obs_dim", "act_dim", "hidden", "m", "pad_")] + \
               [(n, C.c_void_p) for n in ("OBS", "ACTIONS", "RNN_ACTOR", "times", "X", "Y")]


AC_LATE_FRACTION_DEFAULT, AC_LATE_BUDGET_DEFAULT = 1.0, 400000   # include/aircombat.h


class AcLateStats(C.Structure):
    """ac_late_stats_t (include/aircombat.h): what the host steps through ac_step_host_actions counted and, while timing is on, took."""
    _fields_ = [("steps", C.c_int64), ("retries", C.c_int64), ("last_retries", C.c_int32), ("last_late", C.c_int32), ("retry_steps", C.c_int64), ("lowered", C.c_int64), ("disabled", C.c_int64), ("fraction", C.c_double), ("timed_steps", C.c_int64),
                ("copy_before_us", C.c_double), ("dispatch_us", C.c_double), ("copy_after_us", C.c_double), ("wait_us", C.c_double)]


AC_PPO_STAT_LOSS, AC_PPO_STAT_POLICY_LOSS, AC_PPO_STAT_VALUE_LOSS, AC_PPO_STAT_ENTROPY_LOSS, AC_PPO_STAT_RATIO_MEAN, AC_PPO_STAT_DENOMINATOR = range(6)
AC_PPO_NSTAT = 8

# ac_probe_math (include/aircombat.h): row widths and the ops in enum order
AC_PROBE_IN, AC_PROBE_OUT, AC_PROBE_MAX_ROWS = 6, 12, 1 << 22
AC_PROBE_OPS = ("fx_rcp", "fx_rsqrt", "fx_sqrt", "fx_sqrt_both", "fx_sincos", "atan2_fast", "acos_fast", "pow_pos", "tanh_fast", "atanh_fast",
                "sigmoid_f", "tanh_f", "atmosphere", "pitot", "vcas", "in_range_deg", "in_range_rad", "slew", "tef_kinematic", "seek",
                "posture_fn", "missile_height_f", "missile_height_d", "neu_height64", "locate", "locate_fast")
# ac_probe_missile (include/aircombat.h): row widths and limits
AC_PROBE_MSL_IN, AC_PROBE_MSL_TGT, AC_PROBE_MSL_OUT = 16, 7, 16
AC_PROBE_MSL_MAX_ROWS, AC_PROBE_MSL_MAX_TICKS, AC_PROBE_MSL_MAX_CELLS = 512, 4200, 1 << 19

# every symbol include/aircombat.h declares: (restype, argtypes)
_p = C.c_void_p
SIGNATURES = {
    "ac_state_field_name": (C.c_char_p, [C.c_int]),
    "ac_create": (C.c_int, [C.POINTER(AcConfig), C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_p)]),
    "ac_destroy": (C.c_int, [_p]),
    "ac_obs_dim": (C.c_int, [_p]),
    "ac_act_dim": (C.c_int, [_p]),
    "ac_num_envs": (C.c_int, [_p]),
    "ac_num_agents": (C.c_int, [_p]),
    "ac_reset": (C.c_int, [_p, _p]),
    "ac_step": (C.c_int, [_p, _p, _p, _p, _p, _p]),
    "ac_host_buffers": (C.c_int, [_p, C.c_int32, C.POINTER(_p), C.POINTER(_p), C.POINTER(_p), C.POINTER(_p), C.POINTER(_p)]),
    "ac_host_set_detach": (C.c_int, [_p, C.c_int32]),
    "ac_host_set_free": (None, [_p, _p, _p, _p, _p]),
    "ac_step_host_async": (C.c_int, [_p, C.c_int32]),
    "ac_step_host_wait": (C.c_int, [_p]),
    "ac_step_host": (C.c_int, [_p, C.c_int32]),
    "ac_step_host_actions": (C.c_int, [_p, C.c_int32, _p, C.c_size_t]),
    "ac_step_host_actions_begin": (C.c_int, [_p, C.c_int32, _p, C.c_size_t]),
    "ac_step_host_actions_wait": (C.c_int, [_p]),
    "ac_late_config": (C.c_int, [_p, C.c_double, C.c_int32, C.c_int32, C.c_int32]),
    "ac_late_stats": (C.c_int, [_p, _p]),   # (AcLateStats by reference)
    "ac_order_after": (C.c_int, [_p, _p]),
    "ac_order_before": (C.c_int, [_p, _p]),
    "ac_step_async_device": (C.c_int, [_p, _p]),
    "ac_device_buffers": (C.c_int, [_p, C.POINTER(_p), C.POINTER(_p), C.POINTER(_p), C.POINTER(_p), C.POINTER(_p)]),
    "ac_stream": (_p, [_p]),
    "ac_dispatch_path": (C.c_char_p, [_p]),
    "ac_sync": (C.c_int, [_p]),
    "ac_get_state": (C.c_int, [_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "ac_set_state": (C.c_int, [_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "ac_set_status": (C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32]),
    "ac_get_entity": (C.c_int, [_p, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "ac_get_missile": (C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "ac_get_missile_target": (C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "ac_timing_begin": (C.c_int, [_p]),
    "ac_timing_end": (C.c_int, [_p, C.POINTER(C.c_float)]),
    "ac_step_timed_device": (C.c_int, [_p, _p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ac_state_checksum": (C.c_int, [_p, C.POINTER(C.c_uint64)]),
    "ac_munitions_in_flight": (C.c_int, [_p, C.POINTER(C.c_int32)]),
    "ac_seed_envs": (C.c_int, [_p, _p]),
    "ac_get_heading_state": (C.c_int, [_p, C.c_int32, _p]),
    "ac_pin_host_buffer": (C.c_int, [_p, _p, C.c_int64]),
    "ac_unpin_host_buffer": (C.c_int, [_p, _p]),
    "ac_load_controller": (C.c_int, [_p, _p, C.c_int64]),
    "ac_split_f16x2": (C.c_int, [_p, C.c_int64, _p, _p]),
    "ac_split_bf16x3": (C.c_int, [_p, C.c_int64, _p, _p, _p]),
    "ac_controller_precision": (C.c_int, [_p]),
    "ac_controller_forward": (C.c_int, [C.c_int32, C.c_int32, _p, C.c_int64, C.c_int64, _p, _p, _p, _p]),
    "ac_selftest_missile_walk": (C.c_int, [C.c_int32, _p]),
    "ac_probe_math": (C.c_int, [_p, C.c_int32, C.c_int64, _p, _p]),
    "ac_probe_missile": (C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _p, _p, _p]),
    "ac_get_controller_state": (C.c_int, [_p, C.c_int32, C.c_int32, _p, _p]),
    "ac_set_controller_state": (C.c_int, [_p, C.c_int32, C.c_int32, _p]),
    "ac_snapshot_bytes": (C.c_int, [_p, C.POINTER(C.c_int64)]),
    "ac_snapshot_header": (C.c_int, [_p, _p]),
    "ac_snapshot_save": (C.c_int, [_p, _p]),
    "ac_snapshot_load": (C.c_int, [_p, _p]),
    "ac_snapshot_save_host": (C.c_int, [_p, _p, C.c_int64]),
    "ac_snapshot_load_host": (C.c_int, [_p, _p, C.c_int64]),
    "ac_clone_envs": (C.c_int, [_p, _p, _p, C.c_int32]),
    "ac_snapshot_load_envs": (C.c_int, [_p, _p, _p, C.c_int32]),
    "ac_get_obs": (C.c_int, [_p, _p]),
    "ac_snapshot_checksum": (C.c_int, [_p, C.POINTER(C.c_uint64)]),
    "ac_policy_blob_floats": (C.c_int, [_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ac_policy_create": (C.c_int, [C.c_int32, _p, C.POINTER(_p)]),
    "ac_policy_destroy": (C.c_int, [_p]),
    "ac_policy_load": (C.c_int, [_p, _p, C.c_int64, _p, C.c_int64]),
    "ac_policy_load_device": (C.c_int, [_p, _p, _p, C.c_int64, _p, C.c_int64]),
    "ac_policy_load_refused": (C.c_int, [_p, _p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ac_policy_packed": (C.c_int, [_p, C.c_int32, C.POINTER(_p), C.POINTER(C.c_int64)]),
    "ac_policy_get_actions": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, C.c_int32, C.c_uint64, C.c_uint64, _p, _p, _p, _p, _p]),
    "ac_policy_draw_host": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.c_int32, _p]),
    "ac_policy_mappo_blob_floats": (C.c_int, [_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ac_policy_mappo_create": (C.c_int, [C.c_int32, _p, C.POINTER(_p)]),
    "ac_policy_get_actions_mappo": (C.c_int, [_p, _p, _p, _p, _p, C.c_int32, _p, _p, _p, C.c_int32, C.c_uint64, C.c_uint64, _p, _p, _p, _p, _p]),
    "ac_policy_get_values": (C.c_int, [_p, _p, _p, _p, C.c_int32, _p, _p, _p, _p]),
    "ac_policy_pool_member_floats": (C.c_int, [_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ac_policy_pool_compatible": (C.c_int, [_p, C.c_int32, _p, C.c_int32]),
    "ac_policy_pool_create": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, C.POINTER(_p)]),
    "ac_policy_pool_destroy": (C.c_int, [_p]),
    "ac_policy_pool_load": (C.c_int, [_p, C.c_int32, _p, C.c_int64]),
    "ac_policy_pool_load_device": (C.c_int, [_p, _p, C.c_int32, _p, C.c_int64]),
    "ac_policy_pool_load_refused": (C.c_int, [_p, _p, C.POINTER(C.c_int32)]),
    "ac_policy_pool_copy_from": (C.c_int, [_p, _p, C.c_int32, _p]),
    "ac_policy_pool_packed": (C.c_int, [_p, C.c_int32, C.POINTER(_p), C.POINTER(C.c_int64)]),
    "ac_policy_pool_assign": (C.c_int, [_p, _p, _p, C.c_int64, C.c_int32]),
    "ac_policy_pool_assign_sides": (C.c_int, [_p, _p, _p, C.c_int64, C.c_int32]),
    "ac_policy_pool_check": (C.c_int, [_p, _p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ac_policy_pool_plan_host": (C.c_int, [_p, C.c_int64, C.c_int32, C.c_int32, _p, _p, _p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ac_policy_pool_max_tiles": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "ac_policy_pool_set_tile_order": (C.c_int, [_p, C.c_int32]),
    "ac_policy_pool_act": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int32, C.c_uint64, C.c_uint64, _p, _p, _p]),
    "ac_gru_seq_forward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "ac_gru_seq_backward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "ac_gru_layer_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "ac_gru_layer_forward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32] + [_p] * 9 + [C.c_float] + [_p] * 6),
    "ac_gru_layer_backward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32] + [_p] * 20),
    "ac_gru_layer_constant": (C.c_int32, [C.c_int32]),
    # the four calls above with `products` (AC_PRODUCTS_FP32 0, AC_PRODUCTS_BF16X3 1) as the last argument
    "ac_gru_seq_forward_p": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, C.c_int32]),
    "ac_gru_seq_backward_p": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, C.c_int32]),
    "ac_gru_layer_forward_p": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32] + [_p] * 9 + [C.c_float] + [_p] * 6 + [C.c_int32]),
    "ac_gru_layer_backward_p": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32] + [_p] * 20 + [C.c_int32]),
    # the two layer calls above with `dense_products` (the same two constants) after `products`
    "ac_gru_layer_forward_pd": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32] + [_p] * 9 + [C.c_float] + [_p] * 6 + [C.c_int32, C.c_int32]),
    "ac_gru_layer_backward_pd": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32] + [_p] * 20 + [C.c_int32, C.c_int32]),
    "ac_mlp_block_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "ac_mlp_block_forward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, C.c_float, _p, _p, _p, _p, _p, _p, _p]),
    "ac_mlp_block_backward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "ac_mlp_block_forward_p": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, C.c_float, _p, _p, _p, _p, _p, _p, _p, C.c_int32]),
    "ac_mlp_block_backward_p": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32] + [_p] * 12 + [C.c_int32]),
    "ac_mlp_block_constant": (C.c_int32, [C.c_int32]),
    "ac_act_eval_workspace_floats": (C.c_int64, [C.POINTER(AcActHeads), C.c_int32]),
    "ac_act_eval_forward": (C.c_int, [C.c_int32, _p, C.POINTER(AcActHeads), C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "ac_act_eval_backward": (C.c_int, [C.c_int32, _p, C.POINTER(AcActHeads), C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "ac_ppo_loss_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "ac_ppo_loss_forward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, C.c_int32, _p, _p, _p, _p, _p, _p, _p, _p, C.c_double, C.c_double, C.c_double, C.c_int32,
                                      _p, _p, _p, _p, _p]),
    "ac_ppo_loss_backward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, _p, _p, _p, C.c_double, _p, _p, _p]),
    "ac_optim_workspace_floats": (C.c_int64, [_p, C.c_int32, C.c_int32]),
    "ac_optim_grad_norms": (C.c_int, [C.c_int32, _p, _p, _p, C.c_int32, C.c_int32, _p, _p]),
    "ac_optim_clip_adam_step": (C.c_int, [C.c_int32, _p, _p, _p, C.c_int32, C.c_int32, _p, C.c_double, C.c_int32]),
    "ac_ppo_update_constant": (C.c_int32, [C.c_int32]),
    "ac_value_head_forward": (C.c_int, [C.c_int32, _p, C.c_int32, _p, _p, _p, _p]),
    "ac_value_head_workspace_floats": (C.c_int64, [C.c_int32]),
    "ac_value_head_backward": (C.c_int, [C.c_int32, _p, C.c_int32] + [_p] * 7),
    "ac_feature_norm_forward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, C.c_float] + [_p] * 5),
    "ac_feature_norm_workspace_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "ac_feature_norm_backward": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32] + [_p] * 8),
    "ac_shoot_prior": (C.c_int, [C.c_int32, _p, C.c_int32, C.c_int32, _p, _p, _p]),
    "ac_net_constant": (C.c_int32, [C.c_int32]),
    "ac_net_workspace_floats": (C.c_int64, [C.POINTER(AcNet), C.c_int32, C.c_int32]),
    "ac_net_saved_floats": (C.c_int64, [C.POINTER(AcNet), C.c_int32, C.c_int32]),
    "ac_actor_eval_forward": (C.c_int, [C.c_int32, _p, C.POINTER(AcNet), C.c_int32, C.c_int32] + [_p] * 8),
    "ac_actor_eval_backward": (C.c_int, [C.c_int32, _p, C.POINTER(AcNet), C.c_int32, C.c_int32] + [_p] * 9),
    "ac_critic_forward": (C.c_int, [C.c_int32, _p, C.POINTER(AcNet), C.c_int32, C.c_int32] + [_p] * 7),
    "ac_critic_backward": (C.c_int, [C.c_int32, _p, C.POINTER(AcNet), C.c_int32, C.c_int32] + [_p] * 8),
    "ac_last_error": (C.c_char_p, []),
    "ac_version": (C.c_char_p, []),
    # include/aircombat_buffer.h
    "ac_buffer_create": (_p, [C.POINTER(AcBufferConfig), C.c_int]),
    "ac_buffer_destroy": (None, [_p]),
    "ac_buffer_insert": (C.c_int, [_p, C.POINTER(AcBufferStep), C.c_int]),
    "ac_buffer_step_index": (C.c_int, [_p]),
    "ac_buffer_after_update": (C.c_int, [_p]),
    "ac_buffer_clear": (C.c_int, [_p]),
    "ac_buffer_compute_returns": (C.c_int, [_p, _p, C.c_int]),
    "ac_buffer_advantages": (C.c_int, [_p]),
    "ac_buffer_minibatch": (C.c_int, [_p, _p, C.c_int32, C.c_int32, C.POINTER(AcBufferBatch), C.c_int]),
    "ac_buffer_device_ptr": (C.c_int, [_p, C.c_int32, C.POINTER(_p), C.POINTER(C.c_int64)]),
    "ac_buffer_read": (C.c_int, [_p, C.c_int32, _p]),
    "ac_buffer_write_slot": (C.c_int, [_p, C.c_int32, C.c_int32, _p]),
    "ac_buffer_last_kernel_ms": (C.c_int, [_p, C.POINTER(C.c_float)]),
    # include/aircombat_epoch.h
    "ac_buffer_compute_returns_on": (C.c_int, [_p, _p, _p]),
    "ac_buffer_advantages_on": (C.c_int, [_p, _p]),
    "ac_buffer_epoch_layout": (C.c_int, [_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ac_buffer_epoch_layout_for": (C.c_int, [C.POINTER(AcBufferConfig), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ac_buffer_gather_epoch": (C.c_int, [_p, _p, _p, C.c_int32, C.c_int32, C.c_int32, _p]),
    "ac_buffer_epoch_source_row_host": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ac_buffers_epoch_layout": (C.c_int, [C.POINTER(_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ac_buffers_gather_epoch": (C.c_int, [C.POINTER(_p), C.c_int32, _p, _p, C.c_int32, C.c_int32, C.c_int32, _p]),
    "ac_buffers_minibatch": (C.c_int, [C.POINTER(_p), C.c_int32, _p, C.c_int32, C.c_int32, C.POINTER(AcBufferBatch), C.c_int]),
    "ac_buffers_epoch_source_host": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    # include/aircombat_rollout.h
    "ac_rollout_create": (C.c_int, [_p, _p, _p, _p, _p, C.POINTER(_p)]),
    "ac_rollout_destroy": (C.c_int, [_p]),
    "ac_rollout_opponent_state": (C.c_int, [_p, C.POINTER(_p), C.POINTER(_p)]),
    "ac_rollout_collect": (C.c_int, [_p, _p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
    "ac_rollout_post_step_host": (C.c_int, [_p]),
    # include/aircombat_rollout_share.h
    "ac_share_rollout_create": (C.c_int, [_p, _p, _p, _p, _p, C.POINTER(_p)]),
    "ac_share_rollout_destroy": (C.c_int, [_p]),
    "ac_share_rollout_opponent_state": (C.c_int, [_p, C.POINTER(_p), C.POINTER(_p)]),
    "ac_share_rollout_collect": (C.c_int, [_p, _p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
    "ac_share_rollout_post_step_host": (C.c_int, [_p]),
    # include/aircombat_eval.h
    "ac_eval_create": (C.c_int, [_p, _p, _p, _p, C.POINTER(_p)]),
    "ac_eval_destroy": (C.c_int, [_p]),
    "ac_eval_begin": (C.c_int, [_p, _p]),
    "ac_eval_run": (C.c_int, [_p, _p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
    "ac_eval_state": (C.c_int, [_p, _p]),
    "ac_eval_post_step_host": (C.c_int, [_p]),
    # include/aircombat_league.h
    "ac_league_create": (C.c_int, [_p, _p, _p, C.POINTER(_p)]),
    "ac_league_destroy": (C.c_int, [_p]),
    "ac_league_begin": (C.c_int, [_p, _p]),
    "ac_league_run": (C.c_int, [_p, _p, C.c_int32, C.c_uint64, C.c_uint64]),
    "ac_league_state": (C.c_int, [_p, _p]),
    "ac_league_post_step_host": (C.c_int, [_p]),
    "ac_league_table": (C.c_int, [_p, _p, _p]),
    "ac_league_table_host": (C.c_int, [_p]),
    # include/aircombat_record.h
    "ac_recorder_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AcRecorderLayout)]),
    "ac_recorder_create": (C.c_int, [_p, _p, C.c_int32, C.c_int32, C.POINTER(_p)]),
    "ac_recorder_destroy": (C.c_int, [_p]),
    "ac_recorder_bytes": (C.c_int, [_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "ac_recorder_attach": (C.c_int, [_p, _p]),
    "ac_recorder_detach": (C.c_int, [_p]),
    "ac_recorder_capture": (C.c_int, [_p, C.c_int32]),
    "ac_recorder_count": (C.c_int64, [_p]),
    "ac_recorder_info": (C.c_int, [_p, C.POINTER(AcRecorderInfo)]),
    "ac_recorder_read": (C.c_int, [_p, C.c_int32, C.c_int64, C.c_int32, _p]),
    "ac_recorder_device_ptr": (C.c_int, [_p, C.c_int32, C.POINTER(_p), C.POINTER(C.c_int64)]),
    # include/aircombat_spawn.h
    "ac_spawn_check": (C.c_int, [C.c_int32, C.c_int32, _p, C.c_int32, _p]),
    "ac_spawn_attach": (C.c_int, [_p, _p, C.c_int32, _p, C.POINTER(_p)]),
    "ac_spawn_detach": (C.c_int, [_p]),
    "ac_spawn_set_config": (C.c_int, [_p, _p]),
    "ac_spawn_state": (C.c_int, [_p, _p]),
    "ac_spawn_post_step_host": (C.c_int, [_p]),
    "ac_spawn_draw_host": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]),
    # include/aircombat_mutual.h
    "ac_mi_score": (C.c_int, [_p, _p]),
    "ac_mi_score_host": (C.c_int, [_p]),
    "ac_mi_gather": (C.c_int, [_p, _p]),
    "ac_mi_gather_host": (C.c_int, [_p]),
}


def library_path():
    override = os.environ.get("AIRCOMBAT_HIP_LIB")   # another build of the same extension (profiling variants); never a fallback
    if override:
        return override
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "libaircombat_hip.so")


class Lib:
    """Loaded libaircombat_hip.so with typed entry points."""

    def __init__(self, path=None):
        path = path or library_path()
        if not os.path.exists(path):
            raise HipExtensionMissing(
                f"{path} not found: the HIP extension is the only implementation of the step() path. "
                "Build it with __graft_entry__.build() (hipcc --offload-arch=gfx950).")
        try:
            self.dll = C.CDLL(path)
        except OSError as exc:  # e.g. libamdhip64 missing
            raise HipExtensionMissing(f"cannot load {path}: {exc}") from exc
        self.path = path
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(self.dll, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def last_error(self):
        return (self.ac_last_error() or b"").decode()

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {self.last_error()}")

    def state_field_names(self):
        return [self.ac_state_field_name(i).decode() for i in range(AC_STATE_LEN)]


_LIB = None


def load_library(path=None):
    global _LIB
    if _LIB is None or (path and _LIB.path != path):
        # Kernel arguments in device memory: with them in host memory every kernel's first scalar load crosses PCIe (measured on this
        # stack: the BASELINE step kernel 16.3 -> 19.4 us with HIP_FORCE_DEV_KERNARG=0). ROCm 7 defaults to device memory; on a runtime
        # that does not, this asks for it -- it only takes effect if no HIP call has been made in the process yet, and never overrides
        # the caller's setting. (Here and not on every call: every training launch comes through this function.)
        os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")
        _LIB = Lib(path)
    return _LIB
