"""The C ABI as ctypes sees it: the constants and structures of include/azk.h and the argument types of every entry point."""
import ctypes as C

GAME_ID = {"tictactoe": 0, "connect4": 1, "gomoku": 2}
LEAF_F32, LEAF_BF16 = 0, 1
EMBED_POOL_COMPACT_MAX_SLOTS = 65279       # AZK_EMBED_POOL_COMPACT_MAX_SLOTS (include/azk.h)
EMBED_FOLD_ROW = 384        # include/azk.h AZK_EMBED_FOLD_ROW
EMBED_FOLD_MAX_SLOTS = 8192 # include/azk.h AZK_EMBED_FOLD_MAX_SLOTS: pending-leaf slots azk_nn_embed_fold_leaves ranks in LDS


class Config(C.Structure):
    _fields_ = [("game", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("n_games", C.c_int32),
                ("max_sims", C.c_int32), ("leaf_dtype", C.c_int32), ("device", C.c_int32),
                ("arena_nodes", C.c_int32), ("cache_entries", C.c_int32), ("cache_shared", C.c_int32), ("leaves_per_step", C.c_int32),
                ("tree_reuse", C.c_int32), ("emit_elements", C.c_int32), ("reserved", C.c_int32 * 3)]


class LeafSource(C.Structure):
    """azk_leaf_source (include/azk.h): where azk_nn_embed_pool_leaves finds the pending leaves of an engine."""
    _fields_ = [("leaf_flag", C.c_void_p), ("leaf_cells", C.c_void_p), ("to_move", C.c_void_p), ("leaf_depth", C.c_void_p),
                ("leaf_slot", C.c_void_p), ("n_leaf", C.c_void_p), ("n_games", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("rc", C.c_int32), ("rc_pad", C.c_int32), ("planes", C.c_int32), ("flag_bytes", C.c_int32), ("cache_stamp", C.c_void_p)]


class EmbedPoolConsts(C.Structure):
    """azk_embed_pool_consts (include/azk.h): the per-token tables of the compacting embedding + pooling kernel."""
    _fields_ = [("wt_frag", C.c_void_p), ("cpos_tok", C.c_void_p), ("score_tok", C.c_void_p), ("wconst_tok", C.c_void_p),
                ("xnconst_tok", C.c_void_p), ("z_all", C.c_void_p), ("l_all", C.c_void_p), ("score_msum", C.c_void_p),
                ("score_ref", C.c_void_p), ("num_heads", C.c_int32), ("ksize", C.c_int32), ("kp", C.c_int32),
                ("embed_dim", C.c_int32), ("ln_eps", C.c_float), ("work_stats", C.c_void_p)]


class EmbedFoldConsts(C.Structure):
    """azk_embed_fold_consts (include/azk.h): tables of the patch-pooling embedding kernel."""
    _fields_ = [("g_frag", C.c_void_p), ("e_frag", C.c_void_p), ("u2_tok", C.c_void_p), ("score_tok", C.c_void_p),
                ("wconst_tok", C.c_void_p), ("l_all", C.c_void_p), ("score_ref", C.c_void_p), ("inv_scales", C.c_void_p),
                ("num_heads", C.c_int32), ("ksize", C.c_int32), ("embed_dim", C.c_int32), ("ln_eps", C.c_float),
                ("work_stats", C.c_void_p)]


class TailGemm(C.Structure):
    """azk_tail_gemm (include/azk.h): one link of the cls-row tail."""
    _fields_ = [("a_bf16", C.c_void_p), ("lda", C.c_int32), ("a_batch_stride", C.c_int32), ("w_packed", C.c_void_p),
                ("m", C.c_int32), ("n_out", C.c_int32), ("k", C.c_int32), ("nbatch", C.c_int32), ("n_valid", C.c_void_p),
                ("bias", C.c_void_p), ("layernorm_a", C.c_int32), ("epilogue", C.c_int32), ("ln_eps", C.c_float),
                ("a_stats", C.c_void_p), ("a_stats_groups", C.c_int32), ("stats_out", C.c_void_p),
                ("out_bf16", C.c_void_p), ("ldo", C.c_int32), ("resid_bf16", C.c_void_p), ("ldr", C.c_int32),
                ("logits_out", C.c_void_p), ("values_out", C.c_void_p), ("action_dim", C.c_int32), ("a_col_sums", C.c_void_p)]


class GemmTok(C.Structure):
    """azk_gemm_tok (include/azk.h): the LDS-staged GEMM of the full-token transformer block."""
    _fields_ = [("a_bf16", C.c_void_p), ("lda", C.c_int32), ("w_packed", C.c_void_p), ("m", C.c_int32), ("n_out", C.c_int32), ("k", C.c_int32),
                ("n_valid", C.c_void_p), ("bias", C.c_void_p), ("epilogue", C.c_int32), ("out", C.c_void_p), ("ldo", C.c_int32),
                ("resid_bf16", C.c_void_p), ("ldr", C.c_int32)]


class EmbedPoolXConsts(C.Structure):
    """azk_embed_pool_x_consts (include/azk.h): tables of the fp32-accurate embedding + pooling kernel."""
    _fields_ = [("wt_frag", C.c_void_p), ("cpos_tok", C.c_void_p), ("score_tok", C.c_void_p), ("wconst_tok", C.c_void_p),
                ("xnconst_tok", C.c_void_p), ("z_all", C.c_void_p), ("l_all", C.c_void_p), ("score_msum", C.c_void_p),
                ("score_ref", C.c_void_p), ("num_heads", C.c_int32), ("ksize", C.c_int32), ("kp", C.c_int32),
                ("embed_dim", C.c_int32), ("ln_eps", C.c_float), ("wt_scale", C.c_float), ("work_stats", C.c_void_p),
                ("wconst_h16_tok", C.c_void_p), ("pool_scale", C.c_float)]


class GemmH(C.Structure):
    """azk_gemm_h (include/azk.h): one link of the cls-row tail on fp16 (hi, lo) operand planes."""
    _fields_ = [("a_hi", C.c_void_p), ("a_lo", C.c_void_p), ("a_f32", C.c_void_p), ("lda", C.c_int32), ("a_batch_stride", C.c_int32),
                ("w_packed", C.c_void_p), ("m", C.c_int32), ("n_out", C.c_int32), ("k", C.c_int32), ("nbatch", C.c_int32),
                ("n_valid", C.c_void_p), ("bias", C.c_void_p), ("col_sums", C.c_void_p), ("layernorm_a", C.c_int32), ("epilogue", C.c_int32),
                ("ln_eps", C.c_float), ("a_scale", C.c_float), ("w_scale", C.c_float), ("a_stats", C.c_void_p), ("stats_out", C.c_void_p),
                ("out_hi", C.c_void_p), ("out_lo", C.c_void_p), ("out_f32", C.c_void_p), ("ldo", C.c_int32), ("resid_f32", C.c_void_p),
                ("ldr", C.c_int32), ("logits_out", C.c_void_p), ("values_out", C.c_void_p), ("action_dim", C.c_int32), ("overflow_flag", C.c_void_p)]


class AsyncConfig(C.Structure):
    """azk_async_config (include/azk.h)."""
    _fields_ = [("n_sims", C.c_int32), ("max_sims_per_launch", C.c_int32), ("sample_until_move", C.c_int32), ("dirichlet", C.c_int32),
                ("recycle", C.c_int32), ("young_launch_us", C.c_int32), ("seed", C.c_uint64), ("first_global_game", C.c_int64), ("alpha", C.c_double),
                ("stats_dev", C.c_void_p), ("record_capacity", C.c_int64), ("rec_meta_dev", C.c_void_p), ("rec_q_dev", C.c_void_p),
                ("rec_pi_dev", C.c_void_p)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("sims", "edges_scanned", "trace_nodes", "edges_created",
                                          "leaves_evaluated", "terminal_sims", "moves_played", "cache_hits", "roots_reused", "nodes_carried",
                                          "forced_selections", "visits_pruned", "visits_before_pruning")] + [("reserved", C.c_int64 * 3)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_[:13]}


def declare(L, symbols):
    """Set argtypes / restype on every entry point of the loaded library L (symbols: azk.SYMBOLS)."""
    vp, i32, i64, u64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    L.azk_last_error.restype = C.c_char_p
    L.azk_last_error.argtypes = [vp]
    L.azk_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.azk_destroy.argtypes = [vp]
    L.azk_destroy.restype = None
    L.azk_geometry.argtypes = [vp] + [C.POINTER(i32)] * 5
    L.azk_reset_games.argtypes = [vp, i32, i32, vp]
    L.azk_set_positions.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.azk_begin_search.argtypes = [vp, vp, vp]
    L.azk_step_select.argtypes = [vp, vp, vp, vp]
    L.azk_step_expand_backup.argtypes = [vp, vp, vp, vp]
    L.azk_step.argtypes = [vp, vp, vp, vp, vp, vp]
    L.azk_root_stats.argtypes = [vp, vp, vp, vp, vp]
    L.azk_root_children.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp]
    L.azk_export_tree.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.azk_export_tree_quotients.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.azk_debug_fill_quotients.argtypes = [vp, i32, vp]
    L.azk_advance.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.azk_get_positions.argtypes = [vp, vp, vp, vp, vp]
    L.azk_get_counters.argtypes = [vp, C.POINTER(Counters), vp]
    L.azk_reset_counters.argtypes = [vp, vp]
    L.azk_clear_cache.argtypes = [vp, vp]
    L.azk_emit_finished.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
    L.azk_emit_elements.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.azk_replay_gather.argtypes = [i32, i32, i32, i32, C.c_uint32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    L.azk_debug_stamps.argtypes = [vp, vp]
    L.azk_check_device_error.argtypes = [vp, vp]
    L.azk_gen_noise.argtypes = [vp, u64, i64, i32, f64, vp, vp, vp]
    for name in ("azk_rules_legal_moves",):
        getattr(L, name).argtypes = [i32, i32, i32, vp, i32, vp, vp, vp]
    L.azk_rules_legal_mask.argtypes = [i32, i32, i32, vp, i32, vp, vp]
    L.azk_rules_apply_move.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, vp]
    L.azk_rules_undo_move.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp]
    L.azk_rules_check_winner.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp, vp]
    L.azk_rules_canonical.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp]
    L.azk_softmax_rows.argtypes = [vp, i32, i32, vp, vp]
    L.azk_step_tree.argtypes = [vp, vp, vp, vp]
    L.azk_vanilla_set_rng.argtypes = [vp, i32, i32, vp, vp]
    L.azk_vanilla_get_rng.argtypes = [vp, i32, i32, vp, vp]
    L.azk_vanilla_search.argtypes = [vp, i32, vp]
    L.azk_step_gather.argtypes = [vp, vp, vp, vp]
    L.azk_recycle_finished.argtypes = [vp, vp, vp]
    L.azk_nn_patch_embed_scores.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, C.c_float, vp, vp]
    L.azk_nn_embed_pool.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, C.c_float, vp, vp]
    L.azk_leaf_source_of.argtypes = [vp, vp, C.POINTER(LeafSource)]
    L.azk_nn_embed_pool_leaves.argtypes = [C.POINTER(LeafSource), vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, C.c_float, vp]
    L.azk_nn_embed_pool_compact.argtypes = [vp, i32, C.POINTER(EmbedPoolConsts), vp, i32, i32, i32, i32, vp, vp, vp]
    L.azk_nn_embed_pool_compact_leaves.argtypes = [C.POINTER(LeafSource), C.POINTER(EmbedPoolConsts), vp, vp, vp]
    L.azk_nn_embed_fold.argtypes = [vp, i32, C.POINTER(EmbedFoldConsts), vp, i32, i32, i32, i32, vp, vp, vp]
    L.azk_nn_embed_fold_leaves.argtypes = [C.POINTER(LeafSource), C.POINTER(EmbedFoldConsts), vp, vp, vp]
    L.azk_nnx_embed_fold.argtypes = [vp, i32, C.POINTER(EmbedFoldConsts), vp, i32, i32, i32, i32, vp, vp, vp]
    L.azk_nnx_embed_fold_leaves.argtypes = [C.POINTER(LeafSource), C.POINTER(EmbedFoldConsts), vp, vp, vp]
    L.azk_begin_search_budget.argtypes = [vp, vp, i32, i32, vp]
    L.azk_search_unfinished.argtypes = [vp, vp, vp]
    L.azk_nn_tail_gemm.argtypes = [C.POINTER(TailGemm), vp]
    L.azk_nn_tail_gemm_lds.argtypes = [C.POINTER(TailGemm), vp]
    L.azk_nn_gemm_tok.argtypes = [C.POINTER(GemmTok), vp]
    L.azk_nn_attention_tok.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp]
    L.azk_nnx_embed_pool.argtypes = [vp, i32, C.POINTER(EmbedPoolXConsts), vp, i32, i32, i32, i32, vp, vp, vp]
    L.azk_nnx_embed_pool_leaves.argtypes = [C.POINTER(LeafSource), C.POINTER(EmbedPoolXConsts), vp, vp, vp]
    L.azk_nnx_gemm_h.argtypes = [C.POINTER(GemmH), vp]
    L.azk_nnx_gemm_h_lds.argtypes = [C.POINTER(GemmH), vp]
    L.azk_async_begin.argtypes = [vp, C.POINTER(AsyncConfig), vp]
    L.azk_async_begin_reuse.argtypes = [vp, C.POINTER(AsyncConfig), vp]
    L.azk_async_step.argtypes = [vp, vp, vp, i32, vp]
    L.azk_async_set_budget.argtypes = [vp, i32, i32, vp]
    L.azk_async_drain.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.azk_set_playout_cap.argtypes = [vp, f64, i32, u64, i64, vp]
    L.azk_begin_search_capped.argtypes = [vp, vp, i32, i32, i32, vp]
    L.azk_get_search_full.argtypes = [vp, vp, vp]
    L.azk_async_record_flags.argtypes = [vp, vp]
    L.azk_set_resign.argtypes = [vp, f64, i32, f64, u64, i64, vp]
    L.azk_advance_resign.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    L.azk_get_resigned.argtypes = [vp, vp, vp]
    L.azk_get_resign_stats.argtypes = [vp, vp, vp]
    L.azk_set_forced_playouts.argtypes = [vp, f64, vp]
    L.azk_root_policy_target.argtypes = [vp, vp, vp]
    L.azk_async_resign_flags.argtypes = [vp, vp]
    L.azk_set_surprise_weighting.argtypes = [vp, f64, u64, i64, vp]
    L.azk_clear_surprise_weighting.argtypes = [vp]
    L.azk_advance_keyed.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp]
    L.azk_get_surprise.argtypes = [vp, vp, vp, vp]
    L.azk_async_surprise_columns.argtypes = [vp, vp, vp]
    L.azk_set_gumbel_root.argtypes = [vp, i32, i32, f64, f64, vp]
    L.azk_clear_gumbel_root.argtypes = [vp]
    L.azk_gen_gumbel.argtypes = [vp, u64, i64, i32, vp, vp]
    L.azk_gen_gumbel_uniforms.argtypes = [vp, u64, i64, i32, vp, vp]
    L.azk_set_puct.argtypes = [vp, vp, i32, i32, f64, f64, vp]
    L.azk_clear_puct.argtypes = [vp]
    L.azk_set_solver.argtypes = [vp, vp]
    L.azk_clear_solver.argtypes = [vp]
    L.azk_get_solver_status.argtypes = [vp, vp, vp]
    L.azk_export_tree_status.argtypes = [vp, i32, i32, vp, vp]
    L.azk_get_solver_stats.argtypes = [vp, vp, vp]
    L.azk_debug_fill_solver_status.argtypes = [vp, i32, vp]
    L.azk_set_move_temperature.argtypes = [vp, vp, i32, vp, i32, i32, i32, f64, vp]
    L.azk_clear_move_temperature.argtypes = [vp]
    L.azk_get_move_temperature_stats.argtypes = [vp, vp, vp]
    L.azk_set_value_target.argtypes = [vp, f64, f64, vp]
    L.azk_clear_value_target.argtypes = [vp]
    L.azk_get_value_record.argtypes = [vp, vp, vp]
    L.azk_set_openings.argtypes = [vp, f64, i32, i32, u64, i64, vp]
    L.azk_clear_openings.argtypes = [vp]
    L.azk_open_pending.argtypes = [vp, i32, vp]
    L.azk_get_open_plies.argtypes = [vp, vp, vp]
    L.azk_get_opening_stats.argtypes = [vp, vp, vp]
    L.azk_get_opening_actions.argtypes = [vp, vp, vp]
    L.azk_get_leaf_flags.argtypes = [vp, vp, vp]
    L.azk_set_root_noise.argtypes = [vp, i32, f64, vp]
    L.azk_clear_root_noise.argtypes = [vp]
    L.azk_gen_root_noise.argtypes = [vp, u64, i64, i32, vp, vp, vp]
    L.azk_get_root_noise.argtypes = [vp, vp, vp]
    L.azk_set_kld_stop.argtypes = [vp, i32, f64, i32, vp]
    L.azk_clear_kld_stop.argtypes = [vp]
    L.azk_kld_checkpoint.argtypes = [vp, vp, vp]
    L.azk_get_search_sims.argtypes = [vp, vp, vp]
    L.azk_get_kld_rate.argtypes = [vp, vp, vp]
    L.azk_get_kld_stats.argtypes = [vp, vp, vp]
    L.azk_async_sims_column.argtypes = [vp, vp]
    L.azk_set_lead_stop.argtypes = [vp, i32, f64, i32, vp]
    L.azk_clear_lead_stop.argtypes = [vp]
    L.azk_get_lead.argtypes = [vp, vp, vp]
    L.azk_get_lead_stats.argtypes = [vp, vp, vp]
    L.azk_set_eval_symmetry.argtypes = [vp, i32, u64, vp]
    L.azk_get_leaf_symmetry.argtypes = [vp, vp, vp]
    L.azk_eval_symmetry_restore.argtypes = [vp, vp, vp, vp]
    L.azk_nn_ln_heads.argtypes = [vp, C.c_float, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.azk_nn_layernorm_rows.argtypes = [vp, vp, vp, C.c_float, vp, vp, i32, i32, vp, vp]
    L.azk_nn_heads_finalize.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.azk_nn_cls_pool.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]
    L.azk_nn_cls_attention.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, i32, vp]
    L.azk_nn_patch_embed.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, C.c_float, vp]
    for name in symbols:
        f = getattr(L, name)
        if name not in ("azk_last_error", "azk_destroy"):
            f.restype = i32
