"""MI355X Coffee self-play engine — Python host mirror of the C ABI.

The product is ``libkatacoffee.so`` (HIP kernels for gfx950 behind the C ABI in
``include/katacoffee.h``).  This module only binds it with ctypes and moves
arrays through torch device tensors; it has no compute path of its own and
raises if the library is missing or no GPU is present.

Reference interfaces mirrored here (same argument meaning and error behaviour):
  rules/encoder  Board::isLegal board.cpp:185-227, NNInputs::fillRowV1 nninputs.cpp:508-657
  network        NeuralNet::getOutput nninterface.h:31-171
  self-play      `katago selfplay` command/selfplay.cpp:44-72, Play::runGame play.cpp:1146-1701
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libkatacoffee.so")
CSRC = os.path.join(HERE, "csrc")

NUM_SPATIAL = 15
COFFEE_OK = 0
# network precision / path (include/katacoffee.h COFFEE_NN_*)
PRECISIONS = {"default": 0, "accurate": 1, "fast-layered": 2, "corrected": 3, "accurate-nb2": 4, "fast": 5}
PRECISION_NAMES = {v: k for k, v in PRECISIONS.items()}

_lib = None

c_p = ctypes.c_void_p
c_i = ctypes.c_int
c_u64 = ctypes.c_uint64


class CoffeeError(RuntimeError):
    pass


class SearchParams(ctypes.Structure):
    _fields_ = [
        ("max_visits", ctypes.c_int32),
        ("cpuct_exploration", ctypes.c_float), ("cpuct_exploration_log", ctypes.c_float),
        ("cpuct_exploration_base", ctypes.c_float),
        ("fpu_reduction_max", ctypes.c_float), ("root_fpu_reduction_max", ctypes.c_float),
        ("fpu_loss_prop", ctypes.c_float), ("root_fpu_loss_prop", ctypes.c_float),
        ("fpu_parent_weight_by_visited_policy", ctypes.c_int32),
        ("fpu_parent_weight_by_visited_policy_pow", ctypes.c_float),
        ("value_weight_exponent", ctypes.c_float),
        ("root_noise_enabled", ctypes.c_int32),
        ("root_dirichlet_noise_total_concentration", ctypes.c_float),
        ("root_dirichlet_noise_weight", ctypes.c_float),
        ("root_policy_temperature", ctypes.c_float), ("root_policy_temperature_early", ctypes.c_float),
        ("root_desired_per_child_visits_coeff", ctypes.c_float),
        ("root_num_symmetries_to_sample", ctypes.c_int32),
        ("chosen_move_temperature", ctypes.c_float), ("chosen_move_temperature_early", ctypes.c_float),
        ("chosen_move_temperature_halflife", ctypes.c_float),
        ("chosen_move_subtract", ctypes.c_float), ("chosen_move_prune", ctypes.c_float),
        ("use_lcb_for_selection", ctypes.c_int32),
        ("lcb_stdevs", ctypes.c_float), ("min_visit_prop_for_lcb", ctypes.c_float),
        ("subtree_value_bias_factor", ctypes.c_float), ("subtree_value_bias_weight_exponent", ctypes.c_float),
        ("subtree_value_bias_free_prop", ctypes.c_float),
        ("use_graph_search", ctypes.c_int32),
        ("cheap_search_prob", ctypes.c_float), ("cheap_search_visits", ctypes.c_int32),
        ("cheap_search_target_weight", ctypes.c_float), ("reduce_visits", ctypes.c_int32),
        ("reduce_visits_threshold", ctypes.c_float), ("reduce_visits_threshold_lookback", ctypes.c_int32),
        ("reduced_visits_min", ctypes.c_int32), ("reduced_visits_weight", ctypes.c_float),
        ("policy_surprise_data_weight", ctypes.c_float), ("value_surprise_data_weight", ctypes.c_float),
        ("init_games_with_policy", ctypes.c_int32), ("policy_init_area_prop", ctypes.c_float),
        ("policy_init_area_temperature", ctypes.c_float),
        ("early_fork_game_prob", ctypes.c_float), ("early_fork_game_expected_move_prop", ctypes.c_float),
        ("fork_game_prob", ctypes.c_float), ("fork_game_min_choices", ctypes.c_int32),
        ("early_fork_game_max_choices", ctypes.c_int32), ("fork_game_max_choices", ctypes.c_int32),
        ("side_position_prob", ctypes.c_float),
        ("record_tree_positions", ctypes.c_int32), ("record_tree_threshold", ctypes.c_int32),
        ("record_tree_target_weight", ctypes.c_float),
    ]


class SelfplayConfig(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_int32), ("y", ctypes.c_int32), ("win_len", ctypes.c_int32),
        ("num_games", ctypes.c_int32), ("node_cap", ctypes.c_int32), ("row_capacity", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("slot_base", ctypes.c_int32), ("use_fake_net", ctypes.c_int32),
        ("commit_interval", ctypes.c_int32),
        ("model_path", ctypes.c_char_p),
        ("search", SearchParams),
        ("nn_cache_log2", ctypes.c_int32),
        ("nn_batch_cap", ctypes.c_int32),
        ("nn_precision", ctypes.c_int32),
        ("start_stagger", ctypes.c_int32),
        ("engines_per_device", ctypes.c_int32),
    ]


class SelfplayStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ["rounds", "playouts", "nn_evals", "moves", "games_finished", "rows_written", "rows_pending",
                 "rows_dropped", "games_dropped", "errors", "tree_levels", "tree_children", "errors_node_pool",
                 "errors_edge_pool", "edge_pool_peak", "edge_pool_cap", "nn_precision", "nn_audits",
                 "nn_audit_switches"]] + [("nn_audit_max_diff", ctypes.c_double)]


class MatchConfig(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_int32), ("y", ctypes.c_int32), ("win_len", ctypes.c_int32),
        ("num_games", ctypes.c_int32), ("node_cap", ctypes.c_int32),
        ("seed", ctypes.c_uint64), ("slot_base", ctypes.c_int32), ("commit_interval", ctypes.c_int32),
        ("start_stagger", ctypes.c_int32),
        ("model_path", ctypes.c_char_p * 2),
        ("search", SearchParams),
        ("nn_cache_log2", ctypes.c_int32),
        ("nn_batch_cap", ctypes.c_int32),
        ("nn_precision", ctypes.c_int32),
        ("engines_per_device", ctypes.c_int32),
    ]


class MatchStats(ctypes.Structure):
    _fields_ = [("rounds", ctypes.c_uint64), ("playouts", ctypes.c_uint64), ("nn_evals", ctypes.c_uint64 * 2),
                ("moves", ctypes.c_uint64), ("games_finished", ctypes.c_uint64), ("games_dropped", ctypes.c_uint64),
                ("errors", ctypes.c_uint64), ("nn_precision", ctypes.c_uint64 * 2),
                ("nn_batch_peak", ctypes.c_uint64 * 2), ("nn_audits", ctypes.c_uint64 * 2),
                ("nn_audit_switches", ctypes.c_uint64 * 2), ("nn_audit_max_diff", ctypes.c_double * 2)]


class UncertaintyParams(ctypes.Structure):
    _fields_ = [("use_uncertainty", ctypes.c_int32), ("uncertainty_coeff", ctypes.c_float),
                ("uncertainty_exponent", ctypes.c_float), ("uncertainty_max_weight", ctypes.c_float)]


class ExplorationParams(ctypes.Structure):
    """coffee_exploration_params: variance-scaled exploration and noise pruning."""
    _fields_ = [("use_noise_pruning", ctypes.c_int32), ("noise_prune_utility_scale", ctypes.c_float),
                ("noise_pruning_cap", ctypes.c_float), ("cpuct_utility_stdev_prior", ctypes.c_float),
                ("cpuct_utility_stdev_prior_weight", ctypes.c_float), ("cpuct_utility_stdev_scale", ctypes.c_float)]


class RootSearchParams(ctypes.Structure):
    """coffee_root_search_params: wide root noise and futile-visit pruning."""
    _fields_ = [("wide_root_noise", ctypes.c_float), ("futile_visits_threshold", ctypes.c_float)]


SEARCH_THREADS_MAX = 32
ROUND_PATH_MAX = 102
LEAF_NN, LEAF_TERMINAL, LEAF_CATCHUP, LEAF_NOCHILD, LEAF_CACHED, LEAF_COLLISION = 1, 2, 3, 4, 6, 12


class SearchThreadsInfo(ctypes.Structure):
    """coffee_search_threads_info: parallel playouts per search."""
    _fields_ = [("threads", ctypes.c_int32), ("virtual_losses_per_thread", ctypes.c_float),
                ("descents", ctypes.c_uint64), ("collisions", ctypes.c_uint64),
                ("live_virtual_losses", ctypes.c_uint64)]


class RoundPath(ctypes.Structure):
    _fields_ = [("leaf_kind", ctypes.c_int32), ("path_len", ctypes.c_int32),
                ("node", ctypes.c_int32 * ROUND_PATH_MAX), ("child_slot", ctypes.c_int32 * ROUND_PATH_MAX)]


class RoundPaths(ctypes.Structure):
    """coffee_round_paths: the descents of a slot's last round."""
    _fields_ = [("num_descents", ctypes.c_int32), ("pad", ctypes.c_int32), ("path", RoundPath * SEARCH_THREADS_MAX)]


class MatchSide(ctypes.Structure):
    """coffee_match_side: one side's search parameters and uncertainty weighting."""
    _fields_ = [("search", SearchParams), ("unc", UncertaintyParams)]


class MatchOptions(ctypes.Structure):
    """coffee_match_options (coffee_match_create2)."""
    _fields_ = [("per_side", ctypes.c_int32), ("share_net", ctypes.c_int32), ("side", MatchSide * 2)]


class StartPositionsParams(ctypes.Structure):
    _fields_ = [("prob", ctypes.c_float), ("turn_weight_lambda", ctypes.c_float),
                ("start_policy_init_area_prop", ctypes.c_float)]


ANALYSIS_MAX_MOVES = 100
ANALYSIS_MAX_PV = 16
ANALYSIS_OK, ANALYSIS_ILLEGAL_MOVE, ANALYSIS_GAME_OVER, ANALYSIS_NO_LEGAL_MOVE = 0, 1, 2, 3


class AnalysisConfig(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_int32), ("y", ctypes.c_int32), ("win_len", ctypes.c_int32),
        ("num_slots", ctypes.c_int32), ("node_cap", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("model_path", ctypes.c_char_p),
        ("search", SearchParams),
        ("nn_cache_log2", ctypes.c_int32),
        ("nn_batch_cap", ctypes.c_int32),
        ("nn_precision", ctypes.c_int32),
        ("engines_per_device", ctypes.c_int32),
        ("commit_interval", ctypes.c_int32),
        ("query_capacity", ctypes.c_int32),
        ("max_pv_len", ctypes.c_int32),
    ]


class AnalysisStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in
                ["rounds", "playouts", "nn_evals", "queries_loaded", "queries_finished", "queries_rejected", "errors",
                 "nn_precision", "nn_audits", "nn_audit_switches"]] + [("nn_audit_max_diff", ctypes.c_double)]


# coffee_analysis_query / _result / _move as numpy record layouts (C alignment)
ANALYSIS_QUERY = np.dtype([("id", np.uint64), ("rng_counter", np.uint64), ("stream", np.uint32),
                           ("game_num", np.uint32), ("num_moves", np.int32), ("max_visits", np.int32),
                           ("moves", np.uint16, (ANALYSIS_MAX_MOVES,))], align=True)
ANALYSIS_RESULT = np.dtype([("id", np.uint64), ("status", np.int32), ("info", np.int32), ("turn", np.int32),
                            ("pla", np.int32), ("visits", np.uint32), ("weight_sum", np.float32),
                            ("utility_avg", np.float32), ("win_loss_avg", np.float32), ("nn_win", np.float32),
                            ("nn_loss", np.float32), ("num_children", np.int32), ("pad", np.int32)], align=True)
ANALYSIS_MOVE = np.dtype([("move", np.int32), ("edge_visits", np.uint32), ("visits", np.uint32),
                          ("weight_sum", np.float32), ("utility_avg", np.float32), ("win_loss_avg", np.float32),
                          ("prior", np.float32), ("lcb", np.float32), ("radius", np.float32),
                          ("play_selection_value", np.float32), ("order", np.int32), ("pv_len", np.int32),
                          ("pv", np.uint16, (ANALYSIS_MAX_PV,))], align=True)
# coffee_analysis_restrict / _root_info (root restrictions)
ANALYSIS_NO_ALLOWED_MOVE = 4
ANALYSIS_RESTRICT_WORDS = 11
ANALYSIS_RESTRICT = np.dtype([("avoid", np.uint32, (ANALYSIS_RESTRICT_WORDS,)), ("mode", np.int32)], align=True)
ANALYSIS_ROOT_INFO = np.dtype([("symmetries", np.uint32), ("num_masked", np.int32)], align=True)
assert ANALYSIS_RESTRICT.itemsize == 48 and ANALYSIS_ROOT_INFO.itemsize == 8


class AnalysisRootOptions(ctypes.Structure):
    _fields_ = [("root_symmetry_pruning", ctypes.c_int32), ("include_policy", ctypes.c_int32)]


# coffee_start_position
START_POSITION =np.dtype([("weight", np.float32), ("num_moves", np.int32),
                           ("moves", np.uint16, (ANALYSIS_MAX_MOVES,))], align=True)
assert START_POSITION.itemsize == 208
assert ANALYSIS_QUERY.itemsize == 232 and ANALYSIS_RESULT.itemsize == 56 and ANALYSIS_MOVE.itemsize == 80


# Every symbol include/katacoffee.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "coffee_last_error", "coffee_abi_version", "coffee_device_count", "coffee_set_device", "coffee_device_compute_units", "coffee_malloc",
    "coffee_free", "coffee_memcpy", "coffee_synchronize", "coffee_rules_batch", "coffee_play_batch",
    "coffee_encode_batch", "coffee_model_write_random", "coffee_model_flops", "coffee_nn_create",
    "coffee_nn_forward", "coffee_nn_forward2", "coffee_nn_destroy", "coffee_nn_create2", "coffee_nn_is_fused", "coffee_nn_precision", "coffee_fake_net", "coffee_search_params_default",
    "coffee_selfplay_create", "coffee_selfplay_step", "coffee_selfplay_sync", "coffee_selfplay_stats_get",
    "coffee_selfplay_drain_rows", "coffee_selfplay_drain_games", "coffee_selfplay_set_model",
    "coffee_selfplay_stage_rows", "coffee_selfplay_row_capacity", "coffee_row_bytes", "coffee_selfplay_stream",
    "coffee_selfplay_set_model_bytes",
    "coffee_selfplay_destroy", "coffee_selfplay_game_info",
    "coffee_selfplay_game_tree", "coffee_selfplay_root_policy", "coffee_debug_cdf_table", "coffee_debug_zobrist",
    "coffee_selfplay_enable_timing", "coffee_selfplay_kernel_time", "coffee_selfplay_timed_nn_evals",
    "coffee_write_npz",
    "coffee_match_params_default", "coffee_match_create", "coffee_match_step", "coffee_match_sync",
    "coffee_match_stream", "coffee_match_destroy", "coffee_match_stats_get", "coffee_match_drain_games",
    "coffee_match_score", "coffee_match_game_info", "coffee_match_game_tree", "coffee_match_root_policy",
    "coffee_analysis_params_default", "coffee_analysis_create", "coffee_analysis_step", "coffee_analysis_sync",
    "coffee_analysis_stream", "coffee_analysis_destroy", "coffee_analysis_submit", "coffee_analysis_query_check",
    "coffee_analysis_drain", "coffee_analysis_stats_get", "coffee_analysis_game_info", "coffee_analysis_game_tree",
    "coffee_analysis_root_policy",
    "coffee_uncertainty_params_default", "coffee_uncertainty_weight", "coffee_selfplay_set_uncertainty",
    "coffee_match_set_uncertainty", "coffee_analysis_set_uncertainty",
    "coffee_start_positions_params_default", "coffee_start_positions_check", "coffee_start_positions_thresholds",
    "coffee_start_position_pick", "coffee_start_position_draws", "coffee_start_position_index", "coffee_selfplay_set_start_positions",
    "coffee_match_set_start_positions", "coffee_selfplay_start_position_games", "coffee_match_start_position_games",
    "coffee_match_create2", "coffee_match_elo",
    "coffee_analysis_set_root_options", "coffee_analysis_submit2", "coffee_analysis_drain2", "coffee_root_mask",
    "coffee_symmetry_move",
    "coffee_exploration_params_default", "coffee_explore_stdev_factor", "coffee_prune_noise_weight",
    "coffee_selfplay_set_exploration", "coffee_analysis_set_exploration", "coffee_match_set_exploration",
    "coffee_selfplay_game_tree_priors", "coffee_match_game_tree_priors", "coffee_analysis_game_tree_priors",
    "coffee_root_search_params_default", "coffee_wide_root_noise", "coffee_futile_visits",
    "coffee_selfplay_set_root_search", "coffee_analysis_set_root_search", "coffee_match_set_root_search",
    "coffee_analysis_set_search_threads", "coffee_analysis_search_threads_info", "coffee_analysis_round_paths",
    "coffee_virtual_loss",
]


def build(jobs=8):
    """Compile libkatacoffee.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-j%d" % jobs, "-C", CSRC], check=True)


def lib():
    """The loaded C-ABI library.  Raises if it was not built — there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CoffeeError("libkatacoffee.so not built (run katacoffee_amd.build()); no CPU fallback exists")
        # One HIP runtime per process: torch's libraries ask for "libamdhip64.so" while
        # ours asks for the SONAME "libamdhip64.so.7".  Loading torch first lets our
        # request resolve to torch's already-loaded copy; the reverse order would load
        # two runtimes, and ours would then see no device.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        # KATACOFFEE_LIB: an alternative build of the same library (profiling builds)
        L = ctypes.CDLL(os.environ.get("KATACOFFEE_LIB", LIB_PATH))
        L.coffee_last_error.restype = ctypes.c_char_p
        L.coffee_model_write_random.argtypes = [ctypes.c_char_p, c_u64, ctypes.c_char_p]
        L.coffee_model_flops.argtypes = [ctypes.c_char_p, c_i, c_p]
        L.coffee_nn_create.argtypes = [ctypes.c_char_p, c_i, c_i, c_i, c_p]
        L.coffee_nn_create2.argtypes = [ctypes.c_char_p, c_i, c_i, c_i, c_i, c_p]
        L.coffee_nn_is_fused.argtypes = [c_p, c_p]
        if hasattr(L, "coffee_nn_precision"):  # (absent in round-4 builds run as A/B references)
            L.coffee_nn_precision.argtypes = [c_p, c_p, c_p]
        L.coffee_nn_forward.argtypes = [c_p, c_i, c_p, c_p, c_p]
        L.coffee_nn_forward2.argtypes = [c_p, c_i, c_p, c_p, c_p, c_p]
        L.coffee_nn_destroy.argtypes = [c_p]
        L.coffee_fake_net.argtypes = [c_i, c_i, c_i, c_i, c_p, c_p, c_p]
        L.coffee_rules_batch.argtypes = [c_i, c_i, c_i, c_i] + [c_p] * 7
        L.coffee_play_batch.argtypes = [c_i, c_i, c_i, c_i] + [c_p] * 12
        L.coffee_encode_batch.argtypes = [c_i, c_i, c_i, c_i] + [c_p] * 8
        L.coffee_search_params_default.argtypes = [c_p]
        L.coffee_search_params_default.restype = None
        L.coffee_selfplay_create.argtypes = [c_p, c_p]
        L.coffee_selfplay_step.argtypes = [c_p, c_i, c_p]
        L.coffee_selfplay_sync.argtypes = [c_p]
        L.coffee_selfplay_stats_get.argtypes = [c_p, c_p]
        L.coffee_selfplay_drain_rows.argtypes = [c_p, c_i] + [c_p] * 7
        L.coffee_selfplay_drain_games.argtypes = [c_p, c_i, c_p, c_p, c_p]
        L.coffee_selfplay_stage_rows.argtypes = [c_p, c_p, c_i, c_p, c_i]
        L.coffee_selfplay_row_capacity.argtypes = [c_p, c_p]
        L.coffee_row_bytes.argtypes = [c_i, c_i, c_p]
        L.coffee_selfplay_stream.argtypes = [c_p, c_p]
        L.coffee_selfplay_set_model.argtypes = [c_p, ctypes.c_char_p]
        L.coffee_selfplay_set_model_bytes.argtypes = [c_p, c_p, c_u64]
        L.coffee_selfplay_destroy.argtypes = [c_p]
        L.coffee_selfplay_game_info.argtypes = [c_p, c_i, c_p]
        L.coffee_selfplay_game_tree.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p]
        L.coffee_selfplay_root_policy.argtypes = [c_p, c_i, c_p]
        L.coffee_selfplay_enable_timing.argtypes = [c_p, c_i]
        L.coffee_selfplay_kernel_time.argtypes = [c_p, c_i, c_p, c_p]
        L.coffee_selfplay_timed_nn_evals.argtypes = [c_p, c_p]
        L.coffee_debug_cdf_table.argtypes = [c_i, c_i, c_i, c_p]
        L.coffee_debug_zobrist.argtypes = [c_i, c_i, c_i] + [c_p] * 5
        L.coffee_write_npz.argtypes = [ctypes.c_char_p, c_i, c_i, c_i] + [c_p] * 5
        L.coffee_match_params_default.argtypes = [c_p]
        L.coffee_match_params_default.restype = None
        L.coffee_match_create.argtypes = [c_p, c_p]
        L.coffee_match_step.argtypes = [c_p, c_i, c_p]
        L.coffee_match_sync.argtypes = [c_p]
        L.coffee_match_stream.argtypes = [c_p, c_p]
        L.coffee_match_destroy.argtypes = [c_p]
        L.coffee_match_stats_get.argtypes = [c_p, c_p]
        L.coffee_match_drain_games.argtypes = [c_p, c_i, c_p, c_p, c_p]
        L.coffee_match_score.argtypes = [c_p, c_i, c_p, c_p]
        L.coffee_match_game_info.argtypes = [c_p, c_i, c_p]
        L.coffee_match_game_tree.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p]
        L.coffee_match_root_policy.argtypes = [c_p, c_i, c_p]
        L.coffee_analysis_params_default.argtypes = [c_p]
        L.coffee_analysis_params_default.restype = None
        L.coffee_analysis_create.argtypes = [c_p, c_p]
        L.coffee_analysis_step.argtypes = [c_p, c_i, c_p]
        L.coffee_analysis_sync.argtypes = [c_p]
        L.coffee_analysis_stream.argtypes = [c_p, c_p]
        L.coffee_analysis_destroy.argtypes = [c_p]
        L.coffee_analysis_submit.argtypes = [c_p, c_p, c_i, c_p]
        L.coffee_analysis_query_check.argtypes = [c_i, c_i, c_i, c_p]
        L.coffee_analysis_drain.argtypes = [c_p, c_i, c_p, c_p, c_p]
        L.coffee_analysis_stats_get.argtypes = [c_p, c_p]
        L.coffee_analysis_game_info.argtypes = [c_p, c_i, c_p]
        L.coffee_analysis_game_tree.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p]
        L.coffee_analysis_root_policy.argtypes = [c_p, c_i, c_p]
        L.coffee_uncertainty_params_default.argtypes = [c_p]
        L.coffee_uncertainty_params_default.restype = None
        L.coffee_uncertainty_weight.argtypes = [c_p, ctypes.c_float, c_p, c_p]
        L.coffee_selfplay_set_uncertainty.argtypes = [c_p, c_p]
        L.coffee_match_set_uncertainty.argtypes = [c_p, c_p]
        L.coffee_analysis_set_uncertainty.argtypes = [c_p, c_p]
        if hasattr(L, "coffee_start_positions_check"):  # (absent in earlier builds run as A/B references)
            L.coffee_start_positions_params_default.argtypes = [c_p]
            L.coffee_start_positions_params_default.restype = None
            L.coffee_start_positions_check.argtypes = [c_i, c_i, c_i, c_i, c_p, c_p, c_p]
            L.coffee_start_positions_thresholds.argtypes = [c_p, c_i, ctypes.c_float, c_p]
            L.coffee_start_position_index.argtypes = [c_p, c_i, c_u64, c_p]
            L.coffee_start_position_pick.argtypes = [c_u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, c_p, c_i,
                                                     c_p]
            L.coffee_start_position_draws.argtypes = [c_u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, c_p, c_i,
                                                      c_p, c_p]
            L.coffee_selfplay_set_start_positions.argtypes = [c_p, c_p, c_i, c_p]
            L.coffee_match_set_start_positions.argtypes = [c_p, c_p, c_i, c_p]
            L.coffee_selfplay_start_position_games.argtypes = [c_p, c_p]
            L.coffee_match_start_position_games.argtypes = [c_p, c_p]
        if hasattr(L, "coffee_match_create2"):  # (absent in earlier builds run as A/B references)
            L.coffee_match_create2.argtypes = [c_p, c_p, c_p]
            L.coffee_match_elo.argtypes = [ctypes.c_int64] * 3 + [c_p] * 5
        if hasattr(L, "coffee_root_mask"):  # (absent in earlier builds run as A/B references)
            L.coffee_analysis_set_root_options.argtypes = [c_p, c_p]
            L.coffee_analysis_submit2.argtypes = [c_p, c_p, c_p, c_i, c_p]
            L.coffee_analysis_drain2.argtypes = [c_p, c_i, c_p, c_p, c_p, c_p, c_p]
            L.coffee_root_mask.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_p, c_i, c_i, c_p, c_p]
            L.coffee_symmetry_move.argtypes = [c_i, c_i, c_i, c_i]
        if hasattr(L, "coffee_explore_stdev_factor"):  # (absent in earlier builds run as A/B references)
            L.coffee_exploration_params_default.argtypes = [c_p]
            L.coffee_exploration_params_default.restype = None
            L.coffee_explore_stdev_factor.argtypes = [c_p, ctypes.c_int64, ctypes.c_float, ctypes.c_float,
                                                      ctypes.c_float, c_p]
            L.coffee_prune_noise_weight.argtypes = [c_p, c_i, c_p, c_p, c_p, c_p, c_p]
            L.coffee_selfplay_set_exploration.argtypes = [c_p, c_p]
            L.coffee_analysis_set_exploration.argtypes = [c_p, c_p]
            L.coffee_match_set_exploration.argtypes = [c_p, c_i, c_p]
            for f in (L.coffee_selfplay_game_tree_priors, L.coffee_match_game_tree_priors,
                      L.coffee_analysis_game_tree_priors):
                f.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p, c_p]
        if hasattr(L, "coffee_wide_root_noise"):  # (absent in earlier builds run as A/B references)
            L.coffee_root_search_params_default.argtypes = [c_p]
            L.coffee_root_search_params_default.restype = None
            L.coffee_wide_root_noise.argtypes = [c_p, c_u64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int32,
                                                 ctypes.c_uint32, ctypes.c_int32, ctypes.c_float, c_p, c_p]
            L.coffee_futile_visits.argtypes = [c_p, ctypes.c_float, ctypes.c_float, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_int64, ctypes.c_float, c_i, c_p]
            L.coffee_selfplay_set_root_search.argtypes = [c_p, c_p]
            L.coffee_analysis_set_root_search.argtypes = [c_p, c_p]
            L.coffee_match_set_root_search.argtypes = [c_p, c_i, c_p]
        if hasattr(L, "coffee_virtual_loss"):  # (absent in earlier builds run as A/B references)
            L.coffee_analysis_set_search_threads.argtypes = [c_p, c_i, ctypes.c_float]
            L.coffee_analysis_search_threads_info.argtypes = [c_p, c_p]
            L.coffee_analysis_round_paths.argtypes = [c_p, c_i, c_p]
            L.coffee_virtual_loss.argtypes = [ctypes.c_float, ctypes.c_uint32, c_i, ctypes.c_float, ctypes.c_float,
                                              c_p, c_p]
        _lib = L
    return _lib


def check(rc):
    if rc != COFFEE_OK:
        msg = lib().coffee_last_error()
        raise CoffeeError("libkatacoffee error %d: %s" % (rc, msg.decode() if msg else ""))


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def virtual_loss(per_thread, vl, mover, utility, weight):
    """(utility, weight) of a child that vl unfinished playouts of the round have entered, as its
    parent's selection values it (coffee_virtual_loss, the host run of the kernels' code): mover 1
    black / 2 white to move at the parent.  f32 results; vl = 0 returns the inputs."""
    u, w = ctypes.c_float(), ctypes.c_float()
    check(lib().coffee_virtual_loss(ctypes.c_float(float(per_thread)), int(vl), int(mover),
                                    ctypes.c_float(float(utility)), ctypes.c_float(float(weight)),
                                    ctypes.byref(u), ctypes.byref(w)))
    return np.float32(u.value), np.float32(w.value)


def default_search_params(**over):
    p = SearchParams()
    lib().coffee_search_params_default(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def default_match_params(**over):
    """coffee_match_params_default: gatekeeper1.cfg's search values, every play setting off."""
    p = SearchParams()
    lib().coffee_match_params_default(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def default_analysis_params(**over):
    """coffee_analysis_params_default: the match values with analysis_example.cfg's visits, LCB
    settings and root symmetries; root noise off and no pruning of the reported values."""
    p = SearchParams()
    lib().coffee_analysis_params_default(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def default_uncertainty_params(**over):
    """coffee_uncertainty_params_default: off, coefficient 0.25, exponent 1, maximum weight 8
    (gatekeeper1.cfg:108-110 turns it on with these values)."""
    p = UncertaintyParams()
    lib().coffee_uncertainty_params_default(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _uncertainty_params(params, over):
    p = default_uncertainty_params() if params is None else UncertaintyParams.from_buffer_copy(params)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def uncertainty_weight(logit, params=None, **over):
    """(err, weight) of one short-term error logit (a network row's out[P+3]) as np.float32:
    coffee_uncertainty_weight, the host run of the search kernels' own sequence.  params: an
    UncertaintyParams (default: default_uncertainty_params()); keyword overrides on top."""
    p = _uncertainty_params(params, over)
    err, w = ctypes.c_float(), ctypes.c_float()
    check(lib().coffee_uncertainty_weight(ctypes.byref(p), ctypes.c_float(float(logit)), ctypes.byref(err),
                                          ctypes.byref(w)))
    return np.float32(err.value), np.float32(w.value)


def default_exploration_params(**over):
    """coffee_exploration_params_default: both mechanisms off (stdev scale 0, no noise pruning),
    stdev prior 0.40 with weight 2, utility scale 0.15, no cap (FLT_MAX).  The reference's match,
    analysis and GTP set-ups run with cpuct_utility_stdev_scale=0.85 and use_noise_pruning=1."""
    p = ExplorationParams()
    lib().coffee_exploration_params_default(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _exploration_params(params, over):
    p = default_exploration_params() if params is None else ExplorationParams.from_buffer_copy(params)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def explore_stdev_factor(visits, weight_sum, utility_avg, utility_sq_avg, params=None, **over):
    """The factor on a node's exploration scaling from the spread of its utility, as np.float32:
    coffee_explore_stdev_factor, the host run of the search kernels' own sequence.  params: an
    ExplorationParams (default: default_exploration_params()); keyword overrides on top."""
    p = _exploration_params(params, over)
    f = ctypes.c_float()
    check(lib().coffee_explore_stdev_factor(ctypes.byref(p), int(visits), ctypes.c_float(float(weight_sum)),
                                            ctypes.c_float(float(utility_avg)),
                                            ctypes.c_float(float(utility_sq_avg)), ctypes.byref(f)))
    return np.float32(f.value)


def prune_noise_weight(weight, utility, prior, params=None, **over):
    """(new_weight float32 [n], new_total np.float32) of the noise-pruning scan over n children in
    order (their weights, utilities from the parent's side and priors): coffee_prune_noise_weight,
    the host run of the search kernels' own sequence.  params / overrides as explore_stdev_factor."""
    p = _exploration_params(params, over)
    w = np.ascontiguousarray(weight, np.float32)
    u = np.ascontiguousarray(utility, np.float32)
    pr = np.ascontiguousarray(prior, np.float32)
    if not (w.ndim == 1 and w.shape == u.shape == pr.shape):
        raise ValueError("weight, utility and prior must be 1-D arrays of one length")
    out = np.zeros_like(w)
    tot = ctypes.c_float()
    check(lib().coffee_prune_noise_weight(ctypes.byref(p), len(w), _ptr(w), _ptr(u), _ptr(pr), _ptr(out),
                                          ctypes.byref(tot)))
    return out, np.float32(tot.value)


def default_root_search_params(**over):
    """coffee_root_search_params_default: both rules off (wide_root_noise 0,
    futile_visits_threshold 0).  The reference's analysis set-up runs with wide_root_noise=0.04."""
    p = RootSearchParams()
    lib().coffee_root_search_params_default(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def _root_search_params(params, over):
    p = default_root_search_params() if params is None else RootSearchParams.from_buffer_copy(params)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def wide_root_noise(seed, global_slot_or_stream, game_num, turn, root_visits, pos, prior, params=None, **over):
    """(smoothed_prior, bonus) as np.float32 of the move at policy position `pos` in the root
    selection at `root_visits` visits of turn `turn` of game `game_num` of global slot (analysis:
    stream) `global_slot_or_stream` on an engine created with `seed`: coffee_wide_root_noise, the
    host run of the search kernels' own sequence.  params: a RootSearchParams (default:
    default_root_search_params()); keyword overrides on top."""
    p = _root_search_params(params, over)
    sm, b = ctypes.c_float(), ctypes.c_float()
    check(lib().coffee_wide_root_noise(ctypes.byref(p), int(seed), int(global_slot_or_stream), int(game_num),
                                       int(turn), int(root_visits), int(pos), ctypes.c_float(float(prior)),
                                       ctypes.byref(sm), ctypes.byref(b)))
    return np.float32(sm.value), np.float32(b.value)


def futile_visits(max_child_weight, parent_weight_sum, parent_visits, visits_left, edge_visits=0, child_visits=0,
                  child_weight=0.0, is_new=False, params=None, **over):
    """Whether futile-visit pruning skips a root move (coffee_futile_visits, the host run of the
    search kernels' own sequence): an existing child by its edge visits, visits and weight, or with
    is_new the unexpanded candidate.  params / overrides as wide_root_noise."""
    p = _root_search_params(params, over)
    out = ctypes.c_int()
    check(lib().coffee_futile_visits(ctypes.byref(p), ctypes.c_float(float(max_child_weight)),
                                     ctypes.c_float(float(parent_weight_sum)), int(parent_visits), int(visits_left),
                                     int(edge_visits), int(child_visits), ctypes.c_float(float(child_weight)),
                                     1 if is_new else 0, ctypes.byref(out)))
    return bool(out.value)


def _game_tree_priors(fn, h, P, slot, max_nodes):
    priors = np.zeros((max_nodes, P), np.float32)
    next_prior = np.zeros(max_nodes, np.float32)
    next_pos = np.zeros(max_nodes, np.int32)
    n = ctypes.c_int()
    check(fn(h, slot, max_nodes, _ptr(priors), _ptr(next_prior), _ptr(next_pos), ctypes.byref(n)))
    return priors[:n.value], next_prior[:n.value], next_pos[:n.value]


def start_positions(positions):
    """Start positions as a START_POSITION array.  positions: such an array, or a list whose
    entries are move lists (policy positions dir * A + cell from the empty board, black first;
    weight 1), (moves, weight) pairs or dicts with `moves` and optionally `weight`."""
    if isinstance(positions, np.ndarray) and positions.dtype == START_POSITION:
        return np.ascontiguousarray(positions)
    out = np.zeros(len(positions), START_POSITION)
    for i, q in enumerate(positions):
        if isinstance(q, dict):
            moves, w = q.get("moves", ()), q.get("weight", 1.0)
        elif len(q) == 2 and not np.isscalar(q[0]) and np.isscalar(q[1]):
            moves, w = q
        else:
            moves, w = q, 1.0
        moves = list(moves)
        if len(moves) > ANALYSIS_MAX_MOVES:
            raise CoffeeError("start position %d: more than %d moves" % (i, ANALYSIS_MAX_MOVES))
        if any(m < 0 or m > 0xFFFF for m in moves):
            raise CoffeeError("start position %d: a move is not a policy position" % i)
        out[i]["weight"] = w
        out[i]["num_moves"] = len(moves)
        out[i]["moves"][:len(moves)] = moves
    return out


def start_positions_check(X, Y, W, positions):
    """(status, info) int32 arrays of coffee_start_positions_check: every sample replayed with
    the device rules (ANALYSIS_OK / _ILLEGAL_MOVE + move index / _GAME_OVER + winner /
    _NO_LEGAL_MOVE)."""
    _torch_cuda()
    t = start_positions(positions)
    status = np.zeros(len(t), np.int32)
    info = np.zeros(len(t), np.int32)
    check(lib().coffee_start_positions_check(X, Y, W, len(t), _ptr(t), _ptr(status), _ptr(info)))
    return status, info


def start_positions_thresholds(positions, turn_weight_lambda=0.0):
    """The table's 64-bit cumulative thresholds (coffee_start_positions_thresholds, host only)."""
    t = start_positions(positions)
    cum = np.zeros(len(t), np.uint64)
    check(lib().coffee_start_positions_thresholds(_ptr(t) if len(t) else None, len(t),
                                                  ctypes.c_float(turn_weight_lambda), _ptr(cum) if len(t) else None))
    return cum


def start_position_index(cum, r):
    """The sample of raw 64-bit draw r under thresholds cum (coffee_start_position_index)."""
    c = np.ascontiguousarray(cum, np.uint64)
    idx = ctypes.c_int()
    check(lib().coffee_start_position_index(_ptr(c) if len(c) else None, len(c), r, ctypes.byref(idx)))
    return idx.value


def start_position_pick(seed, global_slot, game_num, prob, cum, with_counter=False):
    """The sample game `game_num` of global slot `global_slot` takes, or -1 for the empty
    board (coffee_start_position_pick: the kernels' own code on the host).  cum: the thresholds
    or None (no table).  with_counter: (index, the stream's counter after the draws)."""
    idx = ctypes.c_int()
    ctr = ctypes.c_uint64()
    n = 0 if cum is None else len(cum)
    c = None if n == 0 else _ptr(np.ascontiguousarray(cum, np.uint64))
    if with_counter:
        check(lib().coffee_start_position_draws(seed, global_slot, game_num, ctypes.c_float(prob), c, n,
                                                ctypes.byref(idx), ctypes.byref(ctr)))
        return idx.value, ctr.value
    check(lib().coffee_start_position_pick(seed, global_slot, game_num, ctypes.c_float(prob), c, n,
                                           ctypes.byref(idx)))
    return idx.value


def _set_start_positions(fn, h, positions, prob, turn_weight_lambda, start_policy_init_area_prop):
    t = start_positions(positions if positions is not None else [])
    p = StartPositionsParams(prob, turn_weight_lambda, start_policy_init_area_prop)
    check(fn(h, _ptr(t) if len(t) else None, len(t), ctypes.byref(p)))


def analysis_queries(queries):
    """Queries as an ANALYSIS_QUERY array.  queries: such an array, or a list of dicts with
    `id`, `moves` (policy positions dir * A + cell from the empty board) and optionally
    `max_visits` (0 = the config's), `stream` (default: the low 32 bits of id), `game_num` (0)
    and `rng_counter` (0)."""
    if isinstance(queries, np.ndarray):
        if queries.dtype != ANALYSIS_QUERY:
            raise CoffeeError("queries: a structured array must have dtype ANALYSIS_QUERY")
        return np.ascontiguousarray(queries)
    out = np.zeros(len(queries), ANALYSIS_QUERY)
    for i, q in enumerate(queries):
        moves = list(q.get("moves", ()))
        if len(moves) > ANALYSIS_MAX_MOVES:
            raise CoffeeError("query %r: more than %d moves" % (q.get("id"), ANALYSIS_MAX_MOVES))
        if any(not 0 <= int(m) < 65536 for m in moves):
            raise CoffeeError("query %r: a move is out of range" % (q.get("id"),))
        out[i]["id"] = q["id"]
        out[i]["stream"] = q.get("stream", int(q["id"]) & 0xFFFFFFFF)
        out[i]["game_num"] = q.get("game_num", 0)
        out[i]["rng_counter"] = q.get("rng_counter", 0)
        out[i]["max_visits"] = q.get("max_visits", 0)
        out[i]["num_moves"] = len(moves)
        out[i]["moves"][:len(moves)] = moves
    return out


def move_bits(moves, words):
    """Policy positions as a bit set of `words` uint32 words (bit p of word p // 32)."""
    out = np.zeros(words, np.uint32)
    for m in moves:
        m = int(m)
        if not 0 <= m < 32 * words:
            raise CoffeeError("move %d does not fit a set of %d words" % (m, words))
        out[m >> 5] |= np.uint32(1 << (m & 31))
    return out


def analysis_restricts(queries, P):
    """The root restrictions of query dicts as an ANALYSIS_RESTRICT array, or None when no query
    carries one (or queries is a structured array).  A query's `avoid_moves` / `allow_moves` are
    lists of policy positions; giving both is an error."""
    if isinstance(queries, np.ndarray) or not any("avoid_moves" in q or "allow_moves" in q for q in queries):
        return None
    out = np.zeros(len(queries), ANALYSIS_RESTRICT)
    for i, q in enumerate(queries):
        if "avoid_moves" in q and "allow_moves" in q:
            raise CoffeeError("query %r: avoid_moves and allow_moves are exclusive" % (q.get("id"),))
        for key, mode in (("avoid_moves", 1), ("allow_moves", 2)):
            if key in q:
                out[i]["avoid"] = move_bits(q[key], ANALYSIS_RESTRICT_WORDS)
                out[i]["mode"] = mode
    return out


def symmetry_move(X, Y, sym, move):
    """The image of policy position `move` under symmetry `sym` (coffee_symmetry_move; host)."""
    rc = lib().coffee_symmetry_move(X, Y, sym, move)
    if rc < 0:
        check(rc)
    return rc


def root_mask(X, Y, W, colours, hist_cell, hist_dir, legal, avoid_moves=None, allow_moves=None, prune=True,
              avoid_bits=None, mode=None):
    """The root restriction rule on the host (coffee_root_mask; no device): a dict with `mask`
    (bool [P]), `symmetries` (the used ones, a sorted list), `bits` (the same as a bit set),
    `num_masked` (masked legal moves) and `left` (legal moves left unmasked; 0 is the engine's
    NO_ALLOWED_MOVE answer).  colours [A] 0 / 1 / 2; hist_cell / hist_dir: the last moves, most
    recent first (at most five); legal: bool [P].  avoid_bits / mode pass raw words instead of a
    move list."""
    A, P = X * Y, 4 * X * Y
    nw = (P + 31) // 32
    if avoid_moves is not None and allow_moves is not None:
        raise CoffeeError("root_mask: avoid_moves and allow_moves are exclusive")
    if avoid_bits is None:
        mode = 1 if avoid_moves is not None else (2 if allow_moves is not None else 0)
        lst = avoid_moves if avoid_moves is not None else (allow_moves if allow_moves is not None else [])
        avoid_bits = move_bits(lst, ANALYSIS_RESTRICT_WORDS)
    avoid_bits = np.ascontiguousarray(avoid_bits, np.uint32)
    col = np.ascontiguousarray(colours, np.uint8).reshape(A)
    hc = np.ascontiguousarray(hist_cell, np.int32)
    hd = np.ascontiguousarray(hist_dir, np.int32)
    lg = np.ascontiguousarray(legal).astype(bool).reshape(P)
    legal_bits = np.zeros(nw, np.uint32)
    for p in np.nonzero(lg)[0]:
        legal_bits[p >> 5] |= np.uint32(1 << (int(p) & 31))
    mask = np.zeros(nw, np.uint32)
    syms = ctypes.c_uint32()
    rc = lib().coffee_root_mask(X, Y, W, _ptr(col), _ptr(hc) if len(hc) else None, _ptr(hd) if len(hd) else None,
                                len(hc), _ptr(legal_bits), _ptr(avoid_bits), int(mode), int(bool(prune)), _ptr(mask),
                                ctypes.byref(syms))
    if rc < 0:
        check(rc)
    m = np.array([(int(mask[p >> 5]) >> (p & 31)) & 1 for p in range(P)], bool)
    return {"mask": m, "symmetries": [s for s in range(8) if (syms.value >> s) & 1], "bits": syms.value,
            "num_masked": int((m & lg).sum()), "left": rc}


def analysis_query_check(X, Y, W, query):
    """The host-side checks of a submit (coffee_analysis_query_check): raises CoffeeError naming
    the field.  Needs no device."""
    q = analysis_queries([query] if isinstance(query, dict) else query)
    for i in range(len(q)):
        check(lib().coffee_analysis_query_check(X, Y, W, ctypes.c_void_p(q[i:i + 1].ctypes.data)))


def match_score(header):
    """(candidate points, baseline points) of drained match games (header [n][5]): a win 1,
    a draw 0.5 to each side (coffee_match_score)."""
    header = np.ascontiguousarray(header, np.int32).reshape(-1, 5)
    c, b = ctypes.c_double(), ctypes.c_double()
    check(lib().coffee_match_score(_ptr(header), len(header), ctypes.byref(c), ctypes.byref(b)))
    return c.value, b.value


def match_elo(wins, draws, losses):
    """Elo of a result from one side's view (coffee_match_elo; host, doubles): a dict with the
    score, elo, the 95% interval elo_lo / elo_hi (-inf / inf where it leaves (0, 1)) and los,
    the likelihood of superiority.  No games: CoffeeError."""
    out = [ctypes.c_double() for _ in range(5)]
    check(lib().coffee_match_elo(int(wins), int(draws), int(losses), *[ctypes.byref(o) for o in out]))
    return dict(zip(["score", "elo", "elo_lo", "elo_hi", "los"], [o.value for o in out]))


def _match_side(base, spec, index):
    """One entry of Match(sides=...) as a MatchSide on top of the engine's search `base`: a dict
    of SearchParams / UncertaintyParams field overrides, or a (SearchParams, UncertaintyParams)
    pair (either may be None: the engine's search / uncertainty off)."""
    side = MatchSide()
    side.search = SearchParams.from_buffer_copy(base)
    side.unc = default_uncertainty_params()
    if isinstance(spec, dict):
        sfields = {n for n, _ in SearchParams._fields_}
        ufields = {n for n, _ in UncertaintyParams._fields_}
        for k, v in spec.items():
            if k in sfields:
                setattr(side.search, k, v)
            elif k in ufields:
                setattr(side.unc, k, v)
            else:
                raise CoffeeError("Match sides[%d]: %r is neither a SearchParams nor an UncertaintyParams field"
                                  % (index, k))
    elif isinstance(spec, (tuple, list)) and len(spec) == 2:
        sp, un = spec
        if sp is not None:
            if not isinstance(sp, SearchParams):
                raise CoffeeError("Match sides[%d]: the pair's first entry must be a SearchParams" % index)
            side.search = SearchParams.from_buffer_copy(sp)
        if un is not None:
            if not isinstance(un, UncertaintyParams):
                raise CoffeeError("Match sides[%d]: the pair's second entry must be an UncertaintyParams" % index)
            side.unc = UncertaintyParams.from_buffer_copy(un)
    else:
        raise CoffeeError("Match sides[%d]: a dict of field overrides or a (SearchParams, UncertaintyParams) pair"
                          % index)
    return side


# ---------------------------------------------------------------------------
# Batched rules / encoder / network through device tensors.

def _torch_cuda():
    import torch
    if not torch.cuda.is_available():
        raise CoffeeError("no GPU visible: the HIP path is the only implementation")
    return torch


def _dev(torch, a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype=dtype))
    return torch.from_numpy(a).to("cuda")


def _dp(t):
    return ctypes.c_void_p(t.data_ptr())


def _sync(torch):
    torch.cuda.synchronize()


def rules_batch(X, Y, W, cells, last_cell, last_dir, pla):
    """Legal-move masks [n][4A] u8 and has-legal flags [n] u8 (Board::isLegal board.cpp:185-227)."""
    torch = _torch_cuda()
    n = len(pla)
    A = X * Y
    dc, dl, dd, dp_ = (_dev(torch, cells, np.uint8), _dev(torch, last_cell, np.int8), _dev(torch, last_dir, np.int8),
                       _dev(torch, pla, np.uint8))
    legal = torch.zeros((n, 4 * A), dtype=torch.uint8, device="cuda")
    has = torch.zeros(n, dtype=torch.uint8, device="cuda")
    _sync(torch)
    check(lib().coffee_rules_batch(X, Y, W, n, _dp(dc), _dp(dl), _dp(dd), _dp(dp_), _dp(legal), _dp(has), None))
    _sync(torch)
    return legal.cpu().numpy(), has.cpu().numpy()


def play_batch(X, Y, W, cells, last_cell, last_dir, pla, move):
    torch = _torch_cuda()
    n = len(pla)
    A = X * Y
    ins = [_dev(torch, cells, np.uint8), _dev(torch, last_cell, np.int8), _dev(torch, last_dir, np.int8),
           _dev(torch, pla, np.uint8), _dev(torch, move, np.int32)]
    out_cells = torch.zeros((n, A), dtype=torch.uint8, device="cuda")
    fin = torch.zeros(n, dtype=torch.uint8, device="cuda")
    win = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mr = torch.zeros(n, dtype=torch.int32, device="cuda")
    ph = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    sh = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    _sync(torch)
    check(lib().coffee_play_batch(X, Y, W, n, *[_dp(t) for t in ins], _dp(out_cells), _dp(fin), _dp(win), _dp(mr),
                                  _dp(ph), _dp(sh), None))
    _sync(torch)
    u = lambda t: t.cpu().numpy().view(np.uint64)
    return (out_cells.cpu().numpy(), fin.cpu().numpy(), win.cpu().numpy(), mr.cpu().numpy(), u(ph), u(sh))


def encode_batch(X, Y, W, cells, hist_cell, hist_dir, pla, sym, want_planes=True):
    """Packed V1 rows [n][ceil(15A/64)] u64 and optionally planes [n][15][A] f32."""
    torch = _torch_cuda()
    n = len(pla)
    A = X * Y
    words = (NUM_SPATIAL * A + 63) // 64
    ins = [_dev(torch, cells, np.uint8), _dev(torch, hist_cell, np.int8), _dev(torch, hist_dir, np.int8),
           _dev(torch, pla, np.uint8), _dev(torch, sym, np.int32)]
    packed = torch.zeros((n, words), dtype=torch.int64, device="cuda")
    planes = torch.zeros((n, NUM_SPATIAL, A), dtype=torch.float32, device="cuda") if want_planes else None
    _sync(torch)
    check(lib().coffee_encode_batch(X, Y, W, n, *[_dp(t) for t in ins], _dp(packed),
                                    _dp(planes) if planes is not None else None, None))
    _sync(torch)
    pk = packed.cpu().numpy().view(np.uint64)
    return pk, (planes.cpu().numpy() if planes is not None else None)


def write_random_model(arch, seed, path):
    check(lib().coffee_model_write_random(arch.encode(), seed, path.encode()))


def model_flops(path, area):
    f = ctypes.c_double()
    check(lib().coffee_model_flops(path.encode(), area, ctypes.byref(f)))
    return f.value


class Network:
    """NeuralNet compute handle (nninterface.h createComputeHandle / getOutput).

    precision (include/katacoffee.h COFFEE_NN_*): "default" (the 1e-3-of-fp32 path:
    "corrected" where the fused kernel covers the net, "accurate" otherwise), "corrected"
    (fp16 products + block-scaled e4m3 cross terms), "accurate" (fp16 hi/lo operand pairs:
    within 1e-3 of fp32 for any net), "fast" (fp16 operands; the fused kernel where it
    covers the net) or "fast-layered" (fp16 operands on the per-convolution kernels)."""

    def __init__(self, model_path, X, Y, W, precision="default"):
        self.X, self.Y, self.W = X, Y, W
        self.h = ctypes.c_void_p()
        check(lib().coffee_nn_create2(model_path.encode(), X, Y, W, PRECISIONS[precision], ctypes.byref(self.h)))

    @property
    def fused(self):
        f = ctypes.c_int()
        check(lib().coffee_nn_is_fused(self.h, ctypes.byref(f)))
        return bool(f.value)

    @property
    def precision(self):
        """(name of the precision the handle runs, calibration difference of the default
        precision's corrected-vs-accurate check or 0.0) -- coffee_nn_precision."""
        p, e = ctypes.c_int(), ctypes.c_float()
        check(lib().coffee_nn_precision(self.h, ctypes.byref(p), ctypes.byref(e)))
        return PRECISION_NAMES[p.value], float(e.value)

    def forward_device(self, n, packed_dev, out_dev, stream=None):
        check(lib().coffee_nn_forward(self.h, n, _dp(packed_dev), _dp(out_dev), stream))

    def forward(self, packed):
        """packed [n][words] u64 (host) -> [n][P+4] f32 (host)."""
        torch = _torch_cuda()
        n = packed.shape[0]
        P = 4 * self.X * self.Y
        din = _dev(torch, np.ascontiguousarray(packed).view(np.int64))
        out = torch.zeros((n, P + 4), dtype=torch.float32, device="cuda")
        _sync(torch)
        self.forward_device(n, din, out)
        _sync(torch)
        return out.cpu().numpy()

    def forward_canonical(self, packed, sym):
        """NeuralNet::getOutput (eigenbackend.cpp:1776-1796): packed [n][words] u64 rows
        encoded with symmetries sym [n] -> [n][P+4] f32 with the policy logits in the
        canonical frame (coffee_nn_forward2)."""
        torch = _torch_cuda()
        n = packed.shape[0]
        P = 4 * self.X * self.Y
        din = _dev(torch, np.ascontiguousarray(packed).view(np.int64))
        dsym = _dev(torch, sym, np.int32)
        out = torch.zeros((n, P + 4), dtype=torch.float32, device="cuda")
        _sync(torch)
        check(lib().coffee_nn_forward2(self.h, n, _dp(din), _dp(dsym), _dp(out), None))
        _sync(torch)
        return out.cpu().numpy()

    def close(self):
        if self.h:
            lib().coffee_nn_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fake_net(X, Y, W, packed):
    torch = _torch_cuda()
    n = packed.shape[0]
    P = 4 * X * Y
    din = _dev(torch, np.ascontiguousarray(packed).view(np.int64))
    out = torch.zeros((n, P + 4), dtype=torch.float32, device="cuda")
    _sync(torch)
    check(lib().coffee_fake_net(X, Y, W, n, _dp(din), _dp(out), None))
    _sync(torch)
    return out.cpu().numpy()


def cdf_table(X=5, Y=5, W=4):
    out = np.zeros(2000, np.float32)
    check(lib().coffee_debug_cdf_table(X, Y, W, _ptr(out)))
    return out


def row_bytes(X, Y):
    """Bytes of one packed row (coffee_row_bytes; katacoffee_amd.rows.row_bytes)."""
    b = ctypes.c_int()
    check(lib().coffee_row_bytes(X, Y, ctypes.byref(b)))
    return b.value


def write_npz(path, rows, X, Y):
    """Training rows -> .npz in the reference's format (native writer)."""
    n = len(rows["globalInputNC"])
    arrs = [np.ascontiguousarray(rows[k], dtype=t) for k, t in
            [("binaryInputNCHWPacked", np.uint8), ("globalInputNC", np.float32), ("policyTargetsNCMove", np.int16),
             ("globalTargetsNC", np.float32), ("valueTargetsNCHW", np.int8)]]
    check(lib().coffee_write_npz(path.encode(), n, X, Y, *[_ptr(a) for a in arrs]))


def zobrist_tables(X, Y, W):
    A = X * Y
    out = dict(board=np.zeros((A, 3, 2), np.uint64), board2=np.zeros((A, 4, 2), np.uint64),
               player=np.zeros((3, 2), np.uint64), init=np.zeros(2, np.uint64), game_over=np.zeros(2, np.uint64))
    check(lib().coffee_debug_zobrist(X, Y, W, *[_ptr(out[k]) for k in ["board", "board2", "player", "init",
                                                                          "game_over"]]))
    return out


class Selfplay:
    """One device's self-play engine (games [slot_base, slot_base + num_games))."""

    def __init__(self, X=5, Y=5, W=4, num_games=4096, max_visits=600, seed=1, slot_base=0, model_path=None,
                 node_cap=0, row_capacity=0, commit_interval=0, nn_cache_log2=0, nn_batch_cap=0, nn_precision="default",
                 start_stagger=0, engines_per_device=0, **search_over):
        _torch_cuda()
        self.X, self.Y, self.W = X, Y, W
        self.A, self.P = X * Y, 4 * X * Y
        self.num_games = num_games
        cfg = SelfplayConfig()
        cfg.x, cfg.y, cfg.win_len = X, Y, W
        cfg.num_games = num_games
        cfg.node_cap = node_cap
        cfg.row_capacity = row_capacity
        cfg.seed = seed
        cfg.slot_base = slot_base
        cfg.use_fake_net = 1 if model_path is None else 0
        cfg.commit_interval = commit_interval
        cfg.nn_cache_log2 = nn_cache_log2
        cfg.nn_batch_cap = nn_batch_cap
        cfg.nn_precision = PRECISIONS[nn_precision]
        cfg.start_stagger = start_stagger
        cfg.engines_per_device = engines_per_device
        self._model = model_path.encode() if model_path else None
        cfg.model_path = self._model
        cfg.search = default_search_params(max_visits=max_visits, **search_over)
        self.cfg = cfg
        self.h = ctypes.c_void_p()
        check(lib().coffee_selfplay_create(ctypes.byref(cfg), ctypes.byref(self.h)))

    def step(self, rounds, stream=None):
        check(lib().coffee_selfplay_step(self.h, rounds, stream))

    def set_uncertainty(self, params=None, **over):
        """Uncertainty weighting of the engine's evaluations (coffee_selfplay_set_uncertainty): an
        UncertaintyParams and / or its fields as keywords, e.g. use_uncertainty=1.  Only before
        the first round; afterwards, or for out-of-range values, CoffeeError."""
        p = _uncertainty_params(params, over)
        check(lib().coffee_selfplay_set_uncertainty(self.h, ctypes.byref(p)))

    def set_exploration(self, params=None, **over):
        """Variance-scaled exploration and noise pruning (coffee_selfplay_set_exploration): an
        ExplorationParams and / or its fields as keywords, e.g. use_noise_pruning=1,
        cpuct_utility_stdev_scale=0.85.  Only before the engine's first round."""
        p = _exploration_params(params, over)
        check(lib().coffee_selfplay_set_exploration(self.h, ctypes.byref(p)))

    def set_root_search(self, params=None, **over):
        """Wide root noise and futile-visit pruning (coffee_selfplay_set_root_search): a
        RootSearchParams and / or its fields as keywords, e.g. wide_root_noise=0.04,
        futile_visits_threshold=0.15.  Only before the engine's first round."""
        p = _root_search_params(params, over)
        check(lib().coffee_selfplay_set_root_search(self.h, ctypes.byref(p)))

    def set_start_positions(self, positions, prob, turn_weight_lambda=0.0, start_policy_init_area_prop=0.0):
        """Start positions (coffee_selfplay_set_start_positions): games that start from now on
        begin with probability `prob` from a sample of `positions` (see start_positions()),
        weighted by weight * exp(-moves * turn_weight_lambda).  Between steps at any time; before
        the first round the slots' first games are started again.  A sample the device rules
        reject, or an out-of-range value: CoffeeError, engine untouched.  No positions or
        prob 0: off."""
        _set_start_positions(lib().coffee_selfplay_set_start_positions, self.h, positions, prob,
                             turn_weight_lambda, start_policy_init_area_prop)

    def start_position_games(self):
        """Games started from the start-position table so far."""
        n = ctypes.c_uint64()
        check(lib().coffee_selfplay_start_position_games(self.h, ctypes.byref(n)))
        return n.value

    def sync(self):
        check(lib().coffee_selfplay_sync(self.h))

    def stats(self):
        s = SelfplayStats()
        check(lib().coffee_selfplay_stats_get(self.h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in SelfplayStats._fields_}

    def drain_rows(self, max_rows=1 << 30):
        st = self.stats()
        n = min(max_rows, st["rows_pending"])
        A, P, pb = self.A, self.P, (self.A + 7) // 8
        rows = {
            "binaryInputNCHWPacked": np.zeros((n, NUM_SPATIAL, pb), np.uint8),
            "globalInputNC": np.zeros((n, 1), np.float32),
            "policyTargetsNCMove": np.zeros((n, 2, P), np.int16),
            "globalTargetsNC": np.zeros((n, 64), np.float32),
            "valueTargetsNCHW": np.zeros((n, 5, self.Y, self.X), np.int8),
            "meta": np.zeros((n, 4), np.int32),
        }
        got = ctypes.c_int()
        order = ["binaryInputNCHWPacked", "globalInputNC", "policyTargetsNCMove", "globalTargetsNC",
                 "valueTargetsNCHW", "meta"]
        check(lib().coffee_selfplay_drain_rows(self.h, n, *[_ptr(rows[k]) for k in order], ctypes.byref(got)))
        assert got.value == n
        return rows

    def row_capacity(self):
        n = ctypes.c_int()
        check(lib().coffee_selfplay_row_capacity(self.h, ctypes.byref(n)))
        return n.value

    def stream_ptr(self):
        """The engine's hipStream_t (for torch.cuda.ExternalStream)."""
        p = ctypes.c_void_p()
        check(lib().coffee_selfplay_stream(self.h, ctypes.byref(p)))
        return p.value

    def stage_rows(self, dst, count, discard_games=True):
        """Device-resident row hand-off (coffee_selfplay_stage_rows), enqueued on the
        engine's stream: dst a device uint8 tensor [>= row_capacity][row_bytes], count a
        pinned host int64 tensor element (filled asynchronously)."""
        assert dst.is_cuda and dst.dtype.itemsize == 1 and dst.is_contiguous()
        # the kernel writes up to dst.shape[0] whole rows: a buffer of another shape or on
        # another device would be written out of bounds
        assert dst.dim() == 2 and dst.shape[1] == row_bytes(self.X, self.Y), \
            "dst must be [rows][row_bytes(X, Y)] uint8, got %s" % (tuple(dst.shape),)
        import torch
        assert dst.device.index == torch.cuda.current_device(), "dst must be on the engine's (current) device"
        assert count.is_pinned() and count.dtype.itemsize == 8
        check(lib().coffee_selfplay_stage_rows(self.h, ctypes.c_void_p(dst.data_ptr()), dst.shape[0],
                                               ctypes.c_void_p(count.data_ptr()), 1 if discard_games else 0))

    def drain_games(self, max_games=1 << 20):
        """Finished-game records: header [g][4] i32 (slot, game number, moves, winner)
        and moves [g][A][2] u8 (cell, direction; 0xFF past the last move)."""
        cap = min(max_games, 2 * self.num_games)
        header = np.zeros((cap, 4), np.int32)
        moves = np.zeros((cap, self.A, 2), np.uint8)
        got = ctypes.c_int()
        check(lib().coffee_selfplay_drain_games(self.h, cap, _ptr(header), _ptr(moves), ctypes.byref(got)))
        return header[:got.value], moves[:got.value]

    def set_model(self, model_path):
        """Hot reload: every later round of every game uses this network."""
        self._model = model_path.encode()
        check(lib().coffee_selfplay_set_model(self.h, self._model))

    def set_model_bytes(self, data):
        """Hot reload from a CFNN image in memory (bytes / uint8 array), e.g. weights
        broadcast from rank 0 (katacoffee_amd.weights.broadcast_model)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        check(lib().coffee_selfplay_set_model_bytes(self.h, _ptr(buf), buf.size))

    def game_info(self, slot):
        info = np.zeros(16, np.int64)
        check(lib().coffee_selfplay_game_info(self.h, slot, _ptr(info)))
        keys = ["phase", "rootK", "liveCount", "rootIdx", "gameNum", "turn", "pla", "finished", "winner",
                "playouts", "nnEvals", "moves", "gamesFinished", "lastCell", "lastDir", "rngCtr"]
        return dict(zip(keys, info.tolist()))

    def game_tree(self, slot, max_nodes=4096):
        nodes = np.zeros((max_nodes, 24), np.uint32)
        edges = np.zeros((max_nodes, self.P, 3), np.uint32)
        n = ctypes.c_int()
        check(lib().coffee_selfplay_game_tree(self.h, slot, max_nodes, _ptr(nodes), _ptr(edges), ctypes.byref(n)))
        return nodes[:n.value], edges[:n.value]

    def game_tree_priors(self, slot, max_nodes=4096):
        """(priors [n][P], next_prior [n], next_pos [n]) beside game_tree, in its node order: each
        node's child priors in slot order and its cached next expansion (coffee_selfplay_game_tree_priors)."""
        return _game_tree_priors(lib().coffee_selfplay_game_tree_priors, self.h, self.P, slot, max_nodes)

    def root_policy(self, slot):
        out = np.zeros(self.P, np.float32)
        check(lib().coffee_selfplay_root_policy(self.h, slot, _ptr(out)))
        return out

    def enable_timing(self, every=1):
        """Time every `every`-th launch of each kernel group with HIP events (0 = off)."""
        check(lib().coffee_selfplay_enable_timing(self.h, int(every)))

    def timed_nn_evals(self):
        """Network evaluations performed by the timed network launches."""
        n = ctypes.c_uint64()
        check(lib().coffee_selfplay_timed_nn_evals(self.h, ctypes.byref(n)))
        return n.value

    def kernel_time(self, which):
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        check(lib().coffee_selfplay_kernel_time(self.h, which, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def close(self):
        if self.h:
            lib().coffee_selfplay_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Match:
    """One device's two-network match engine (coffee_match_*): games [slot_base, slot_base +
    num_games) between net 0 (baseline_path) and net 1 (candidate_path); None = the stand-in
    network.  The candidate plays black in game n of global slot s iff s + n is even, and
    every evaluation of a game in a round is done by the net of its root player.  Mirrors
    Selfplay's stepping and inspection interface; there are no training rows.
    search: a SearchParams to start from instead of default_match_params(); keyword
    overrides apply on top of either.
    sides (coffee_match_create2): a pair, side 0 (the baseline's side) then side 1 (the
    candidate's), each a dict of SearchParams / UncertaintyParams / RootSearchParams field
    overrides on top of the engine's search (uncertainty and root search off), or a (SearchParams, UncertaintyParams) pair.  Every
    search then runs with the parameters of the side that searches; set_uncertainty is
    refused.  The game-level settings (init_games_with_policy and its two area settings) stay
    the engine's.
    share_net: both sides on one network instance (equal paths required): one launch a round
    and one evaluation cache."""

    def __init__(self, X=5, Y=5, W=4, num_games=128, baseline_path=None, candidate_path=None, seed=1, slot_base=0,
                 node_cap=0, commit_interval=0, nn_cache_log2=0, nn_batch_cap=0, nn_precision="default",
                 start_stagger=0, engines_per_device=0, search=None, sides=None, share_net=False, **search_over):
        self.X, self.Y, self.W = X, Y, W
        self.A, self.P = X * Y, 4 * X * Y
        self.num_games = num_games
        self.slot_base = slot_base
        search = default_match_params() if search is None else SearchParams.from_buffer_copy(search)
        for k, v in search_over.items():
            setattr(search, k, v)
        cfg = MatchConfig()
        cfg.x, cfg.y, cfg.win_len = X, Y, W
        cfg.num_games = num_games
        cfg.node_cap = node_cap
        cfg.seed = seed
        cfg.slot_base = slot_base
        cfg.commit_interval = commit_interval
        cfg.start_stagger = start_stagger
        self._models = [p.encode() if p else None for p in (baseline_path, candidate_path)]
        cfg.model_path[0], cfg.model_path[1] = self._models
        cfg.search = search
        cfg.nn_cache_log2 = nn_cache_log2
        cfg.nn_batch_cap = nn_batch_cap
        cfg.nn_precision = PRECISIONS[nn_precision]
        cfg.engines_per_device = engines_per_device
        self.cfg = cfg
        self.h = ctypes.c_void_p()
        if sides is None and not share_net:
            check(lib().coffee_match_create(ctypes.byref(cfg), ctypes.byref(self.h)))
            return
        opts = MatchOptions()
        opts.share_net = 1 if share_net else 0
        root_search = []
        if sides is not None:
            if not isinstance(sides, (tuple, list)) or len(sides) != 2:
                raise CoffeeError("Match sides: a pair (side 0, side 1)")
            opts.per_side = 1
            rfields = {n for n, _ in RootSearchParams._fields_}
            for i in range(2):
                spec = sides[i]
                if isinstance(spec, dict):
                    # (the root-search fields travel in their own struct: set after the create)
                    root_search.append({k: v for k, v in spec.items() if k in rfields})
                    spec = {k: v for k, v in spec.items() if k not in rfields}
                else:
                    root_search.append({})
                opts.side[i] = _match_side(search, spec, i)
        self.opts = opts
        check(lib().coffee_match_create2(ctypes.byref(cfg), ctypes.byref(opts), ctypes.byref(self.h)))
        for i, over in enumerate(root_search):
            if over:
                try:
                    self.set_root_search(side=i, **over)
                except CoffeeError:
                    self.close()
                    raise

    def step(self, rounds, stream=None):
        check(lib().coffee_match_step(self.h, rounds, stream))

    def set_uncertainty(self, params=None, **over):
        """Uncertainty weighting of the engine's evaluations (coffee_match_set_uncertainty): an
        UncertaintyParams and / or its fields as keywords, e.g. use_uncertainty=1.  Only before
        the first round (one setting serves both nets); afterwards, or for out-of-range values, CoffeeError."""
        p = _uncertainty_params(params, over)
        check(lib().coffee_match_set_uncertainty(self.h, ctypes.byref(p)))

    def set_exploration(self, params=None, side=-1, **over):
        """Variance-scaled exploration and noise pruning (coffee_match_set_exploration): an
        ExplorationParams and / or its fields as keywords.  side: -1 on an engine without per-side
        settings, 0 / 1 on one with them.  Only before the engine's first round."""
        p = _exploration_params(params, over)
        check(lib().coffee_match_set_exploration(self.h, int(side), ctypes.byref(p)))

    def set_root_search(self, params=None, side=-1, **over):
        """Wide root noise and futile-visit pruning (coffee_match_set_root_search): a
        RootSearchParams and / or its fields as keywords.  side: -1 on an engine without per-side
        settings, 0 / 1 on one with them.  Only before the engine's first round."""
        p = _root_search_params(params, over)
        check(lib().coffee_match_set_root_search(self.h, int(side), ctypes.byref(p)))

    def set_start_positions(self, positions, prob, turn_weight_lambda=0.0, start_policy_init_area_prop=0.0):
        """Start positions (coffee_match_set_start_positions), as Selfplay.set_start_positions:
        opening variety that depends on neither net's policy."""
        _set_start_positions(lib().coffee_match_set_start_positions, self.h, positions, prob,
                             turn_weight_lambda, start_policy_init_area_prop)

    def start_position_games(self):
        """Games started from the start-position table so far."""
        n = ctypes.c_uint64()
        check(lib().coffee_match_start_position_games(self.h, ctypes.byref(n)))
        return n.value

    def sync(self):
        check(lib().coffee_match_sync(self.h))

    def stats(self):
        s = MatchStats()
        check(lib().coffee_match_stats_get(self.h, ctypes.byref(s)))
        out = {}
        for k, t in MatchStats._fields_:
            v = getattr(s, k)
            out[k] = list(v) if hasattr(v, "__len__") else v
        return out

    def stream_ptr(self):
        p = ctypes.c_void_p()
        check(lib().coffee_match_stream(self.h, ctypes.byref(p)))
        return p.value

    def drain_games(self, max_games=1 << 20):
        """Finished-game records: header [g][5] i32 (slot, game number, moves, winner,
        candidate's colour) and moves [g][A][2] u8 (cell, direction; 0xFF past the last move)."""
        cap = min(max_games, 2 * self.num_games)
        header = np.zeros((cap, 5), np.int32)
        moves = np.zeros((cap, self.A, 2), np.uint8)
        got = ctypes.c_int()
        check(lib().coffee_match_drain_games(self.h, cap, _ptr(header), _ptr(moves), ctypes.byref(got)))
        return header[:got.value], moves[:got.value]

    score = staticmethod(match_score)

    def game_info(self, slot):
        info = np.zeros(16, np.int64)
        check(lib().coffee_match_game_info(self.h, slot, _ptr(info)))
        keys = ["phase", "rootK", "liveCount", "rootIdx", "gameNum", "turn", "pla", "finished", "winner",
                "playouts", "nnEvals", "moves", "gamesFinished", "lastCell", "lastDir", "rngCtr"]
        return dict(zip(keys, info.tolist()))

    def game_tree(self, slot, max_nodes=4096):
        nodes = np.zeros((max_nodes, 24), np.uint32)
        edges = np.zeros((max_nodes, self.P, 3), np.uint32)
        n = ctypes.c_int()
        check(lib().coffee_match_game_tree(self.h, slot, max_nodes, _ptr(nodes), _ptr(edges), ctypes.byref(n)))
        return nodes[:n.value], edges[:n.value]

    def game_tree_priors(self, slot, max_nodes=4096):
        """(priors [n][P], next_prior [n], next_pos [n]) beside game_tree, in its node order: each
        node's child priors in slot order and its cached next expansion (coffee_match_game_tree_priors)."""
        return _game_tree_priors(lib().coffee_match_game_tree_priors, self.h, self.P, slot, max_nodes)

    def root_policy(self, slot):
        out = np.zeros(self.P, np.float32)
        check(lib().coffee_match_root_policy(self.h, slot, _ptr(out)))
        return out

    def close(self):
        if self.h:
            lib().coffee_match_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Analysis:
    """One device's batched position analysis (coffee_analysis_*): num_slots concurrent
    searches of queued positions.  submit() queues queries (see analysis_queries), step() runs
    rounds, drain() returns the finished results as structured arrays: headers [n]
    (ANALYSIS_RESULT) and per-child records [n][P] (ANALYSIS_MOVE, child-slot order, the first
    num_children valid).  Values are from white's perspective as stored; `pla` is the side to
    move.  search: a SearchParams to start from instead of default_analysis_params(); keyword
    overrides apply on top of either."""

    def __init__(self, X=5, Y=5, W=4, num_slots=64, model_path=None, search=None, seed=1, node_cap=0,
                 commit_interval=0, nn_cache_log2=0, nn_batch_cap=0, nn_precision="default", engines_per_device=0,
                 query_capacity=0, max_pv_len=ANALYSIS_MAX_PV, root_symmetry_pruning=False, include_policy=False,
                 search_threads=1, virtual_losses_per_thread=1.0, **search_over):
        self.X, self.Y, self.W = X, Y, W
        self.root_symmetry_pruning, self.include_policy = False, False
        self.A, self.P = X * Y, 4 * X * Y
        self.num_slots = num_slots
        search = default_analysis_params() if search is None else SearchParams.from_buffer_copy(search)
        for k, v in search_over.items():
            setattr(search, k, v)
        cfg = AnalysisConfig()
        cfg.x, cfg.y, cfg.win_len = X, Y, W
        cfg.num_slots = num_slots
        cfg.node_cap = node_cap
        cfg.seed = seed
        self._model = model_path.encode() if model_path else None
        cfg.model_path = self._model
        cfg.search = search
        cfg.nn_cache_log2 = nn_cache_log2
        cfg.nn_batch_cap = nn_batch_cap
        cfg.nn_precision = PRECISIONS[nn_precision]
        cfg.engines_per_device = engines_per_device
        cfg.commit_interval = commit_interval
        cfg.query_capacity = query_capacity if query_capacity else 4 * num_slots
        cfg.max_pv_len = max_pv_len
        self.query_capacity = cfg.query_capacity
        self.cfg = cfg
        self.h = ctypes.c_void_p()
        check(lib().coffee_analysis_create(ctypes.byref(cfg), ctypes.byref(self.h)))
        if root_symmetry_pruning or include_policy:
            self.set_root_options(root_symmetry_pruning, include_policy)
        self.search_threads = 1
        if search_threads != 1 or virtual_losses_per_thread != 1.0:
            try:
                self.set_search_threads(search_threads, virtual_losses_per_thread)
            except CoffeeError:
                self.close()
                raise

    def set_search_threads(self, threads, virtual_losses_per_thread=1.0):
        """Parallel playouts per search (coffee_analysis_set_search_threads): up to `threads`
        descents of a searching slot a round, steered apart by virtual losses.  Only while the
        engine holds no query; num_slots x threads must fit one network launch."""
        check(lib().coffee_analysis_set_search_threads(self.h, int(threads),
                                                       ctypes.c_float(float(virtual_losses_per_thread))))
        self.search_threads = int(threads)

    def search_threads_info(self):
        """coffee_analysis_search_threads_info as a dict: threads, virtual_losses_per_thread,
        descents, collisions, live_virtual_losses."""
        s = SearchThreadsInfo()
        check(lib().coffee_analysis_search_threads_info(self.h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in SearchThreadsInfo._fields_}

    def round_paths(self, slot):
        """The descents of the slot's last round (coffee_analysis_round_paths), in order: dicts of
        leaf_kind (LEAF_*), nodes and child_slots (one entry per path level from the root down)
        and, for a LEAF_COLLISION, collision = (node, child slot) it was abandoned at."""
        r = RoundPaths()
        check(lib().coffee_analysis_round_paths(self.h, int(slot), ctypes.byref(r)))
        out = []
        for j in range(r.num_descents):
            p = r.path[j]
            d = {"leaf_kind": p.leaf_kind, "nodes": list(p.node[:p.path_len]),
                 "child_slots": list(p.child_slot[:p.path_len]), "collision": None}
            if p.leaf_kind == LEAF_COLLISION:
                d["collision"] = (p.node[p.path_len], p.child_slot[p.path_len])
            out.append(d)
        return out

    def submit(self, queries, restricts=None):
        """Queues queries; returns how many were accepted (the first ones): submitted minus
        drained never exceeds query_capacity.  A query dict's `avoid_moves` / `allow_moves` (or
        restricts, an ANALYSIS_RESTRICT array beside a query array) restrict its root; such
        queries go through coffee_analysis_submit2, others through coffee_analysis_submit."""
        q = analysis_queries(queries)
        r = analysis_restricts(queries, self.P) if restricts is None else np.ascontiguousarray(restricts)
        if r is None:
            n = ctypes.c_int()
            check(lib().coffee_analysis_submit(self.h, _ptr(q), len(q), ctypes.byref(n)))
            return n.value
        return self.submit2(q, r)

    def submit2(self, queries, restricts=None):
        """submit() through coffee_analysis_submit2 whether or not a query is restricted."""
        q = analysis_queries(queries)
        r = analysis_restricts(queries, self.P) if restricts is None else np.ascontiguousarray(restricts)
        if r is not None and (r.dtype != ANALYSIS_RESTRICT or len(r) != len(q)):
            raise CoffeeError("restricts: one ANALYSIS_RESTRICT entry per query")
        n = ctypes.c_int()
        check(lib().coffee_analysis_submit2(self.h, _ptr(q), None if r is None else _ptr(r), len(q), ctypes.byref(n)))
        return n.value

    def set_root_options(self, root_symmetry_pruning=False, include_policy=False):
        """coffee_analysis_set_root_options; only before the first submitted query."""
        o = AnalysisRootOptions(int(root_symmetry_pruning), int(include_policy))
        check(lib().coffee_analysis_set_root_options(self.h, ctypes.byref(o)))
        self.root_symmetry_pruning, self.include_policy = bool(root_symmetry_pruning), bool(include_policy)

    def step(self, rounds, stream=None):
        check(lib().coffee_analysis_step(self.h, rounds, stream))

    def set_uncertainty(self, params=None, **over):
        """Uncertainty weighting of the engine's evaluations (coffee_analysis_set_uncertainty): an
        UncertaintyParams and / or its fields as keywords, e.g. use_uncertainty=1.  Only before
        the first submitted query and round; afterwards, or for out-of-range values, CoffeeError."""
        p = _uncertainty_params(params, over)
        check(lib().coffee_analysis_set_uncertainty(self.h, ctypes.byref(p)))

    def set_exploration(self, params=None, **over):
        """Variance-scaled exploration and noise pruning (coffee_analysis_set_exploration): an
        ExplorationParams and / or its fields as keywords, e.g. use_noise_pruning=1,
        cpuct_utility_stdev_scale=0.85.  Only before the engine's first round and query."""
        p = _exploration_params(params, over)
        check(lib().coffee_analysis_set_exploration(self.h, ctypes.byref(p)))

    def set_root_search(self, params=None, **over):
        """Wide root noise and futile-visit pruning (coffee_analysis_set_root_search): a
        RootSearchParams and / or its fields as keywords, e.g. wide_root_noise=0.04.  Only before
        the engine's first round and query."""
        p = _root_search_params(params, over)
        check(lib().coffee_analysis_set_root_search(self.h, ctypes.byref(p)))

    def sync(self):
        check(lib().coffee_analysis_sync(self.h))

    def drain(self, max_results=None, with_root=False):
        """(headers [n], moves [n][P]) of the finished results, in completion order.  with_root:
        (headers, moves, root, policy) through coffee_analysis_drain2 -- root [n]
        (ANALYSIS_ROOT_INFO: `symmetries` bits and `num_masked`), policy [n][P] on an engine
        with include_policy (else None)."""
        cap = self.query_capacity if max_results is None else min(max_results, self.query_capacity)
        header = np.zeros(cap, ANALYSIS_RESULT)
        moves = np.zeros((cap, self.P), ANALYSIS_MOVE)
        n = ctypes.c_int()
        if not with_root:
            check(lib().coffee_analysis_drain(self.h, cap, _ptr(header), _ptr(moves), ctypes.byref(n)))
            return header[:n.value], moves[:n.value]
        root = np.zeros(cap, ANALYSIS_ROOT_INFO)
        policy = np.zeros((cap, self.P), np.float32) if self.include_policy else None
        check(lib().coffee_analysis_drain2(self.h, cap, _ptr(header), _ptr(moves), _ptr(root),
                                           None if policy is None else _ptr(policy), ctypes.byref(n)))
        return header[:n.value], moves[:n.value], root[:n.value], None if policy is None else policy[:n.value]

    def drain2(self, max_results=None):
        return self.drain(max_results, with_root=True)

    def analyze(self, queries, rounds_per_step=32, max_steps=1 << 20, with_root=False):
        """Submits every query (as capacity allows), steps and drains until each id is back;
        returns (headers, moves) in the order of `queries`, with_root (headers, moves, root,
        policy) as drain() does.  The ids must be distinct."""
        q = analysis_queries(queries)
        r = analysis_restricts(queries, self.P)
        ids = [int(i) for i in q["id"]]
        if len(set(ids)) != len(ids):
            raise CoffeeError("analyze: query ids must be distinct")
        sent, got, want = 0, {}, set(ids)
        for _ in range(max_steps):
            if len(got) == len(ids):
                break
            if sent < len(q):
                sent += self.submit(q[sent:], None if r is None else r[sent:])
            self.step(rounds_per_step)
            res = self.drain(with_root=with_root)
            for i in range(len(res[0])):
                if int(res[0][i]["id"]) in want:  # (results of queries submitted before this call are dropped)
                    got[int(res[0][i]["id"])] = tuple(None if a is None else a[i].copy() for a in res)
        else:
            raise CoffeeError("analyze: the queries did not finish")
        header = np.zeros(len(ids), ANALYSIS_RESULT)
        moves = np.zeros((len(ids), self.P), ANALYSIS_MOVE)
        root = np.zeros(len(ids), ANALYSIS_ROOT_INFO)
        policy = np.zeros((len(ids), self.P), np.float32) if with_root and self.include_policy else None
        for k, i in enumerate(ids):
            header[k], moves[k] = got[i][0], got[i][1]
            if with_root:
                root[k] = got[i][2]
                if policy is not None:
                    policy[k] = got[i][3]
        return (header, moves, root, policy) if with_root else (header, moves)

    def stats(self):
        s = AnalysisStats()
        check(lib().coffee_analysis_stats_get(self.h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in AnalysisStats._fields_}

    def stream_ptr(self):
        p = ctypes.c_void_p()
        check(lib().coffee_analysis_stream(self.h, ctypes.byref(p)))
        return p.value

    def game_info(self, slot):
        info = np.zeros(16, np.int64)
        check(lib().coffee_analysis_game_info(self.h, slot, _ptr(info)))
        keys = ["phase", "rootK", "liveCount", "rootIdx", "gameNum", "turn", "pla", "finished", "winner",
                "playouts", "nnEvals", "moves", "gamesFinished", "lastCell", "lastDir", "rngCtr"]
        return dict(zip(keys, info.tolist()))

    def game_tree(self, slot, max_nodes=4096):
        nodes = np.zeros((max_nodes, 24), np.uint32)
        edges = np.zeros((max_nodes, self.P, 3), np.uint32)
        n = ctypes.c_int()
        check(lib().coffee_analysis_game_tree(self.h, slot, max_nodes, _ptr(nodes), _ptr(edges), ctypes.byref(n)))
        return nodes[:n.value], edges[:n.value]

    def game_tree_priors(self, slot, max_nodes=4096):
        """(priors [n][P], next_prior [n], next_pos [n]) beside game_tree, in its node order: each
        node's child priors in slot order and its cached next expansion (coffee_analysis_game_tree_priors)."""
        return _game_tree_priors(lib().coffee_analysis_game_tree_priors, self.h, self.P, slot, max_nodes)

    def root_policy(self, slot):
        out = np.zeros(self.P, np.float32)
        check(lib().coffee_analysis_root_policy(self.h, slot, _ptr(out)))
        return out

    def close(self):
        if self.h:
            lib().coffee_analysis_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
