"""ctypes binding of libdbaz_hip.so (C ABI: include/dbaz.h).

This is the stub a reference maintainer would add.  There
is no fallback: if the HIP library is missing or cannot be loaded, importing
the product path raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DBAZ_LIB") or os.path.join(_HERE, "libdbaz_hip.so")  # DBAZ_LIB: diagnostic builds (tools/)

OK, EINVAL, EILLEGAL, EDEVICE, EPOOL, ESTATE = range(6)
RESULT_NONE = 2
EVAL_FORMULA_HASH, EVAL_FORMULA_UNIFORM, EVAL_RESNET, EVAL_SIMPLENN, EVAL_EXTERNAL, EVAL_SOLVER = range(6)
ABI_VERSION = 3  # DBAZ_ABI_VERSION of include/dbaz.h
DBG_EARLY_JOIN = 1
DBG_NO_FALLBACK = 2  # reserved bit of dbaz_config.debug_flags: dbaz_create rejects it (DBAZ_EINVAL)

# every symbol include/dbaz.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "dbaz_last_error", "dbaz_version", "dbaz_build_info", "dbaz_nodes_per_slot", "dbaz_create", "dbaz_destroy", "dbaz_sync",
    "dbaz_rules_init", "dbaz_rules_valid_moves", "dbaz_rules_play", "dbaz_rules_result", "dbaz_rules_features",
    "dbaz_nn_configure", "dbaz_nn_select_model", "dbaz_nn_set_tensor", "dbaz_nn_commit", "dbaz_nn_predict",
    "dbaz_set_search_params", "dbaz_set_positions", "dbaz_search", "dbaz_search_timed", "dbaz_set_pending", "dbaz_search_begin", "dbaz_select", "dbaz_expand_backup",
    "dbaz_get_roots", "dbaz_get_root_states", "dbaz_advance",
    "dbaz_selfplay_start", "dbaz_selfplay_set_start", "dbaz_selfplay_script", "dbaz_selfplay_fastforward", "dbaz_selfplay_stagger", "dbaz_selfplay_quickplay",
    "dbaz_selfplay_set_playout_cap", "dbaz_get_playout_cap", "dbaz_playout_cap_is_full",
    "dbaz_selfplay_set_forced_playouts", "dbaz_get_forced_playouts", "dbaz_prune_visits", "dbaz_fetch_row_flags",
    "dbaz_selfplay_set_gumbel", "dbaz_get_gumbel", "dbaz_gumbel_considered", "dbaz_gumbel_target",
    "dbaz_selfplay_set_gumbel_mode", "dbaz_get_gumbel_mode", "dbaz_gumbel_improved_policy", "dbaz_gumbel_nonroot_pick", "dbaz_gumbel_target_full",
    "dbaz_match_set_search", "dbaz_match_get_search",
    "dbaz_step", "dbaz_run",
    "dbaz_get_counters", "dbaz_timing_begin", "dbaz_timing_end", "dbaz_fetch_samples", "dbaz_replay_rows_dev",
    "dbaz_replay_rows_clear", "dbaz_dataset_select", "dbaz_dataset_begin", "dbaz_dataset_add_rows", "dbaz_dataset_finish", "dbaz_dataset_fetch", "dbaz_dataset_batch", "dbaz_dataset_batch_on",
    "dbaz_symmetry_apply", "dbaz_symmetry_table",
    "dbaz_trainer_last_error", "dbaz_trainer_board_supported", "dbaz_trainer_create", "dbaz_trainer_destroy", "dbaz_trainer_forward", "dbaz_trainer_backward",
    "dbaz_trainer_net_forward", "dbaz_trainer_net_backward",
    "dbaz_bn2d_workspace_bytes", "dbaz_bn2d_forward", "dbaz_bn2d_backward",
    "dbaz_az_loss_workspace_bytes", "dbaz_az_loss", "dbaz_sgd_step",
    "dbaz_solver_last_error", "dbaz_solver_create", "dbaz_solver_destroy", "dbaz_solver_solve", "dbaz_solver_info", "dbaz_solver_table",
    "dbaz_solver_score", "dbaz_perfect_policy", "dbaz_attach_solver",
    "dbaz_endgame_last_error", "dbaz_endgame_create", "dbaz_endgame_destroy", "dbaz_endgame_score", "dbaz_exact_policy", "dbaz_exact_policy_from", "dbaz_attach_endgame",
    "dbaz_get_endgame_stats", "dbaz_exact_targets", "dbaz_dataset_exact_targets",
    "dbaz_deep_last_error", "dbaz_deep_create", "dbaz_deep_destroy", "dbaz_deep_solve", "dbaz_deep_info", "dbaz_deep_table",
    "dbaz_deep_score", "dbaz_deep_policy",
    "dbaz_tables_last_error", "dbaz_tables_create", "dbaz_tables_destroy", "dbaz_tables_solve", "dbaz_tables_info", "dbaz_tables_roots",
    "dbaz_tables_table", "dbaz_tables_score", "dbaz_tables_targets", "dbaz_replay_exact_targets",
    "dbaz_attach_tables", "dbaz_get_slot_table",
    "dbaz_attach_tables_pool", "dbaz_get_table_pool", "dbaz_get_slot_table_index", "dbaz_attach_tables_pool_wait", "dbaz_get_table_pool_waits",
    "dbaz_attach_leaf_solver", "dbaz_get_leaf_solves",
]


class NetTensors(C.Structure):
    """dbaz_net_tensors (include/dbaz.h): device pointers to a ResNetZero's parameters -- or to where their gradients go."""
    _fields_ = [(k, C.c_void_p) for k in (
        "bn_input_w", "bn_input_b", "conv0_w", "conv0_b", "bn0_w", "bn0_b", "blk_conv_w", "blk_conv_b", "blk_bn_w", "blk_bn_b",
        "ph_conv_w", "ph_conv_b", "ph_bn_w", "ph_bn_b", "ph_fc_w", "ph_fc_b", "vh_conv_w", "vh_conv_b", "vh_bn_w", "vh_bn_b",
        "vh_fc0_w", "vh_fc0_b", "vh_fc1_w", "vh_fc1_b")]


class NetRunning(C.Structure):
    """dbaz_net_running: the BatchNorm layers' running statistics."""
    _fields_ = [(k, C.c_void_p) for k in ("bn_input_mean", "bn_input_var", "bn0_mean", "bn0_var", "blk_mean", "blk_var", "ph_mean", "ph_var",
                                          "vh_mean", "vh_var")]


class Config(C.Structure):
    _fields_ = [
        ("rows", C.c_int32), ("cols", C.c_int32), ("n_slots", C.c_int32), ("nodes_per_slot", C.c_int32),
        ("mcts_num_read", C.c_int32), ("cpuct", C.c_double), ("cpuct_base", C.c_double),
        ("noise_alpha", C.c_double), ("noise_coeff", C.c_double), ("reuse_tree", C.c_int32),
        ("n_temp", C.c_int32), ("temp_idx", C.c_int32 * 8), ("temp_val", C.c_double * 8),
        ("evaluator", C.c_int32), ("device", C.c_int32), ("seed", C.c_uint64), ("max_out_rows", C.c_int32),
        ("nn_precision", C.c_int32), ("match_play", C.c_int32), ("evaluator2", C.c_int32),
        ("transposition_cache", C.c_int32), ("max_pending_evals", C.c_int32), ("selfplay_pending", C.c_int32),
        ("eval_round", C.c_int32), ("eval_defer_max", C.c_int32), ("debug_flags", C.c_uint32), ("reserved", C.c_int32 * 3),
    ]


class Counters(C.Structure):
    _fields_ = [
        ("steps", C.c_int64), ("expansions", C.c_int64), ("nn_evals", C.c_int64), ("terminal_leaves", C.c_int64),
        ("sum_path", C.c_int64), ("games_finished", C.c_int64), ("rows_ready", C.c_int64), ("moves_played", C.c_int64),
        ("pool_high_water", C.c_int64), ("active_slots", C.c_int32), ("error_slots", C.c_int32), ("blocked_slots", C.c_int32), ("f32_fallback_evals", C.c_int32),
        ("ms_total", C.c_double), ("ms_tree", C.c_double), ("ms_nn", C.c_double), ("nn_launches", C.c_int64),
        ("ms_nn_tower", C.c_double), ("cache_hits", C.c_int64), ("pool_resets", C.c_int64),
    ]


class DbazError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


_lib = None


def load():
    """Load the HIP library or raise -- never falls back to a CPU path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `python -m dotsboxesaz_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    # A process that also uses torch must load torch's bundled HIP runtime BEFORE this library pulls in
    # the system one: in the other order torch's later initialisation finds "No HIP GPUs" (two runtimes
    # competing for the device; measured on ROCm 7.2 + torch 2.10/rocm7.0).  The library itself has no
    # torch dependency -- a process without torch simply runs on the system runtime.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    L.dbaz_version.restype = C.c_int
    if L.dbaz_version() != ABI_VERSION:
        raise ImportError("%s has ABI version %d, this binding expects %d: rebuild with `python -m dotsboxesaz_amd.build`"
                          % (LIB_PATH, L.dbaz_version(), ABI_VERSION))
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.dbaz_last_error.argtypes = [vp]
    L.dbaz_last_error.restype = C.c_char_p
    L.dbaz_version.restype = C.c_int
    L.dbaz_nodes_per_slot.argtypes = [vp]
    L.dbaz_build_info.restype = C.c_char_p
    L.dbaz_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.dbaz_destroy.argtypes = [vp]
    L.dbaz_destroy.restype = None
    L.dbaz_sync.argtypes = [vp]
    L.dbaz_rules_init.argtypes = [vp, i32, vp, vp, vp, vp]
    L.dbaz_rules_valid_moves.argtypes = [vp, i32, vp, vp]
    L.dbaz_rules_play.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.dbaz_rules_result.argtypes = [vp, i32, vp, vp, vp]
    L.dbaz_rules_features.argtypes = [vp, i32, vp, vp, vp, vp]
    L.dbaz_nn_configure.argtypes = [vp, i32, i32, i32, i32, i32]
    L.dbaz_nn_select_model.argtypes = [vp, i32]
    L.dbaz_nn_set_tensor.argtypes = [vp, C.c_char_p, vp, i64]
    L.dbaz_nn_commit.argtypes = [vp]
    L.dbaz_nn_predict.argtypes = [vp, i32, vp, vp, vp]
    L.dbaz_set_search_params.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double]
    L.dbaz_set_positions.argtypes = [vp, vp, vp]
    L.dbaz_search.argtypes = [vp, vp, vp]
    L.dbaz_search_timed.argtypes = [vp, vp, vp, C.c_double]
    L.dbaz_set_pending.argtypes = [vp, i32, i32]
    L.dbaz_search_begin.argtypes = [vp, vp, vp]
    L.dbaz_select.argtypes = [vp, vp, vp, vp]
    L.dbaz_expand_backup.argtypes = [vp, vp, vp]
    L.dbaz_get_roots.argtypes = [vp] + [vp] * 8
    L.dbaz_get_root_states.argtypes = [vp] + [vp] * 6
    L.dbaz_advance.argtypes = [vp, vp, i32]
    L.dbaz_selfplay_start.argtypes = [vp, i64, i64]
    L.dbaz_selfplay_set_start.argtypes = [vp, vp, vp, i32, i32]
    L.dbaz_selfplay_script.argtypes = [vp, i64, vp, i32, vp]
    L.dbaz_selfplay_fastforward.argtypes = [vp, vp]
    L.dbaz_selfplay_stagger.argtypes = [vp, vp]
    L.dbaz_selfplay_quickplay.argtypes = [vp, vp, i32]
    L.dbaz_selfplay_set_playout_cap.argtypes = [vp, C.c_double, i32]
    L.dbaz_get_playout_cap.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]
    L.dbaz_playout_cap_is_full.argtypes = [C.c_uint64, i64, i32, C.c_double]
    L.dbaz_selfplay_set_forced_playouts.argtypes = [vp, C.c_double, i32]
    L.dbaz_get_forced_playouts.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]
    L.dbaz_prune_visits.argtypes = [i32, C.c_double, C.c_double, C.c_double, i64, vp, vp, vp, vp, vp]
    L.dbaz_fetch_row_flags.argtypes = [vp, i32, C.POINTER(i32), vp]
    L.dbaz_selfplay_set_gumbel.argtypes = [vp, i32, C.c_double, C.c_double]
    L.dbaz_get_gumbel.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i64), C.POINTER(i64)]
    L.dbaz_gumbel_considered.argtypes = [i32, i32, vp]
    L.dbaz_gumbel_target.argtypes = [i32, C.c_double, C.c_double, vp, vp, vp, vp, vp]
    L.dbaz_selfplay_set_gumbel_mode.argtypes = [vp, i32]
    L.dbaz_get_gumbel_mode.argtypes = [vp, C.POINTER(i32)]
    L.dbaz_match_set_search.argtypes = [vp, i32, i32, i32, C.c_double, C.c_double, i32, C.c_double]
    L.dbaz_match_get_search.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i32),
                                        C.POINTER(C.c_double)]
    for f in (L.dbaz_gumbel_improved_policy, L.dbaz_gumbel_nonroot_pick, L.dbaz_gumbel_target_full):
        f.argtypes = [i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp, vp]
    L.dbaz_step.argtypes = [vp, i32]
    L.dbaz_run.argtypes = [vp, i64]
    L.dbaz_get_counters.argtypes = [vp, C.POINTER(Counters)]
    L.dbaz_timing_begin.argtypes = [vp]
    L.dbaz_timing_end.argtypes = [vp]
    L.dbaz_fetch_samples.argtypes = [vp, i32, vp] + [vp] * 13
    L.dbaz_replay_rows_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32)]
    L.dbaz_trainer_last_error.argtypes = [vp]
    L.dbaz_trainer_last_error.restype = C.c_char_p
    L.dbaz_trainer_board_supported.argtypes = [i32, i32]
    L.dbaz_trainer_create.argtypes = [i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.dbaz_trainer_destroy.argtypes = [vp]
    L.dbaz_trainer_destroy.restype = None
    L.dbaz_trainer_forward.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dbaz_trainer_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dbaz_trainer_net_forward.argtypes = [vp, i32, vp, C.POINTER(NetTensors), C.POINTER(NetRunning), i32, i32, i32, vp, vp, vp]
    L.dbaz_trainer_net_backward.argtypes = [vp, vp, vp, vp, C.POINTER(NetTensors), C.POINTER(NetTensors), vp]
    L.dbaz_bn2d_workspace_bytes.argtypes = [i32]
    L.dbaz_bn2d_forward.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, C.c_float, C.c_float, i32, vp, vp, vp, vp, vp]
    L.dbaz_bn2d_backward.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.dbaz_az_loss_workspace_bytes.argtypes = []
    L.dbaz_az_loss.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, vp, vp, vp, vp, vp]
    L.dbaz_sgd_step.argtypes = [i32, vp, vp, vp, vp, vp, vp, vp, i32, C.c_float, C.c_float, C.c_float, vp]
    L.dbaz_solver_last_error.argtypes = [vp]
    L.dbaz_solver_last_error.restype = C.c_char_p
    L.dbaz_solver_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.dbaz_solver_destroy.argtypes = [vp]
    L.dbaz_solver_destroy.restype = None
    L.dbaz_solver_solve.argtypes = [vp, i32]
    L.dbaz_solver_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(i32)]
    L.dbaz_solver_table.argtypes = [vp, vp, i64, i64]
    L.dbaz_solver_score.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.dbaz_perfect_policy.argtypes = [vp, i32, vp, C.c_uint64, vp, vp, vp]
    L.dbaz_attach_solver.argtypes = [vp, i32, vp, C.c_uint64, i32]
    L.dbaz_endgame_last_error.argtypes = [vp]
    L.dbaz_endgame_last_error.restype = C.c_char_p
    L.dbaz_endgame_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.dbaz_endgame_destroy.argtypes = [vp]
    L.dbaz_endgame_destroy.restype = None
    L.dbaz_endgame_score.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dbaz_exact_policy.argtypes = [vp, i32, vp, C.c_uint64, vp, vp, vp, vp]
    L.dbaz_exact_policy_from.argtypes = [vp, i32, vp, i32, vp, C.c_uint64, vp, vp, C.POINTER(C.c_float), vp]
    L.dbaz_attach_endgame.argtypes = [vp, i32, vp, C.c_uint64, i32]
    L.dbaz_get_endgame_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.dbaz_exact_targets.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.dbaz_dataset_exact_targets.argtypes = [vp, vp, i32, i32, vp]
    L.dbaz_deep_last_error.argtypes = [vp]
    L.dbaz_deep_last_error.restype = C.c_char_p
    L.dbaz_deep_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.dbaz_deep_destroy.argtypes = [vp]
    L.dbaz_deep_destroy.restype = None
    L.dbaz_deep_solve.argtypes = [vp, vp, i32]
    L.dbaz_deep_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(C.c_double), C.POINTER(i32)]
    L.dbaz_deep_table.argtypes = [vp, vp, i64, i64]
    L.dbaz_deep_score.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dbaz_deep_policy.argtypes = [vp, i32, vp, C.c_uint64, vp, vp, vp, vp]
    L.dbaz_tables_last_error.argtypes = [vp]
    L.dbaz_tables_last_error.restype = C.c_char_p
    L.dbaz_tables_create.argtypes = [i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.dbaz_tables_destroy.argtypes = [vp]
    L.dbaz_tables_destroy.restype = None
    L.dbaz_tables_solve.argtypes = [vp, i32, vp, i32]
    L.dbaz_tables_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_double)]
    L.dbaz_tables_roots.argtypes = [vp, vp, vp]
    L.dbaz_tables_table.argtypes = [vp, i32, vp, i64, i64]
    L.dbaz_tables_score.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.dbaz_tables_targets.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.dbaz_replay_exact_targets.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp, vp]
    L.dbaz_attach_tables.argtypes = [vp, i32, vp, C.c_uint64, i32]
    L.dbaz_get_slot_table.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), vp, vp, i64, i64]
    L.dbaz_attach_tables_pool.argtypes = [vp, i32, vp, i32, C.c_uint64, i32]
    L.dbaz_get_table_pool.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.dbaz_attach_tables_pool_wait.argtypes = [vp, i32, vp, i32, C.c_uint64, i32]
    L.dbaz_get_table_pool_waits.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.dbaz_get_slot_table_index.argtypes = [vp, i32, C.POINTER(i32)]
    L.dbaz_attach_leaf_solver.argtypes = [vp, i32, vp, i32, C.c_uint64]
    L.dbaz_get_leaf_solves.argtypes = [vp, C.POINTER(i64)]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if name not in ("dbaz_last_error", "dbaz_build_info", "dbaz_destroy", "dbaz_trainer_last_error", "dbaz_trainer_destroy", "dbaz_bn2d_workspace_bytes",
                        "dbaz_az_loss_workspace_bytes", "dbaz_solver_last_error", "dbaz_solver_destroy", "dbaz_endgame_last_error", "dbaz_endgame_destroy", "dbaz_get_endgame_stats",
                        "dbaz_deep_last_error", "dbaz_deep_destroy", "dbaz_tables_last_error", "dbaz_tables_destroy"):
            fn.restype = C.c_int
    L.dbaz_bn2d_workspace_bytes.restype = C.c_int64
    L.dbaz_az_loss_workspace_bytes.restype = C.c_int64
    L.dbaz_get_endgame_stats.restype = None
    _lib = L
    return L


def build_info():
    """{"src": hash of all kernel sources, "nn": hash of the network kernels} of the LOADED library (csrc/buildinfo.cpp)."""
    info = load().dbaz_build_info().decode()
    return dict(kv.split("=", 1) for kv in info.split() if "=" in kv)


def check(handle, rc):
    if rc == OK:
        return
    msg = load().dbaz_last_error(handle)
    msg = msg.decode() if msg else "error %d" % rc
    if rc == EILLEGAL:
        raise ValueError(msg)  # the reference raises ValueError for illegal moves
    raise DbazError(rc, msg)
