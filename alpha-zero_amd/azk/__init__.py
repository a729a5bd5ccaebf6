"""azk - ctypes binding of libazk.so (include/azk.h), the MI355X-native self-play engine.

Host orchestration stays Python (as in the reference); everything on the hot path is a HIP kernel
behind the C ABI.  There is NO CPU fallback: if libazk.so is missing or no GPU is visible the
functions here raise.  PyTorch is used for device memory and streams only.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
LIB_PATH = os.path.join(_HERE, "libazk.so")

ABI_VERSION = 5           # include/azk.h AZK_ABI_VERSION the structure layouts below were written for

# every symbol include/azk.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "azk_abi_version", "azk_last_error", "azk_create", "azk_destroy", "azk_geometry", "azk_reset_games",
    "azk_set_positions", "azk_begin_search", "azk_step_select", "azk_step_expand_backup", "azk_step",
    "azk_root_stats", "azk_root_children", "azk_export_tree", "azk_advance", "azk_get_positions",
    "azk_get_counters", "azk_reset_counters", "azk_check_device_error", "azk_gen_noise",
    "azk_rules_legal_moves", "azk_rules_legal_mask", "azk_rules_apply_move", "azk_rules_undo_move",
    "azk_rules_check_winner", "azk_rules_canonical", "azk_softmax_rows",
    "azk_step_tree", "azk_step_gather", "azk_recycle_finished", "azk_nn_patch_embed", "azk_nn_cls_attention", "azk_nn_patch_embed_scores", "azk_nn_cls_pool", "azk_debug_stamps", "azk_debug_stamps_raw", "azk_emit_finished", "azk_clear_cache", "azk_nn_heads_finalize", "azk_nn_layernorm_rows",
    "azk_vanilla_set_rng", "azk_vanilla_get_rng", "azk_vanilla_search", "azk_nn_embed_pool",
    "azk_nn_ln_heads",
    "azk_leaf_source_of", "azk_nn_embed_pool_leaves", "azk_nn_embed_pool_compact", "azk_nn_embed_pool_compact_leaves",
    "azk_nn_embed_fold", "azk_nn_embed_fold_leaves", "azk_nnx_embed_fold", "azk_nnx_embed_fold_leaves",
    "azk_nn_tail_gemm", "azk_nn_tail_gemm_lds", "azk_nn_tail_lds_footprint", "azk_nn_embed_fold_grid", "azk_nn_gemm_tok", "azk_nn_attention_tok", "azk_begin_search_budget", "azk_search_unfinished",
    "azk_nnx_embed_pool", "azk_nnx_embed_pool_leaves", "azk_nnx_gemm_h", "azk_nnx_gemm_h_lds",
    "azk_async_begin", "azk_async_step", "azk_async_drain", "azk_async_set_budget", "azk_async_begin_reuse",
    "azk_set_playout_cap", "azk_begin_search_capped", "azk_get_search_full", "azk_async_record_flags",
    "azk_set_resign", "azk_advance_resign", "azk_get_resigned", "azk_get_resign_stats", "azk_async_resign_flags",
    "azk_set_forced_playouts", "azk_root_policy_target",
    "azk_set_eval_symmetry", "azk_get_leaf_symmetry", "azk_eval_symmetry_restore",
    "azk_emit_elements", "azk_replay_gather",
    "azk_set_surprise_weighting", "azk_clear_surprise_weighting", "azk_advance_keyed", "azk_get_surprise", "azk_async_surprise_columns",
    "azk_set_gumbel_root", "azk_clear_gumbel_root", "azk_gen_gumbel", "azk_gen_gumbel_uniforms",
    "azk_set_openings", "azk_clear_openings", "azk_open_pending", "azk_get_open_plies", "azk_get_opening_stats",
    "azk_get_opening_actions", "azk_get_leaf_flags",
    "azk_set_puct", "azk_clear_puct",
    "azk_set_move_temperature", "azk_clear_move_temperature", "azk_get_move_temperature_stats",
    "azk_set_value_target", "azk_clear_value_target", "azk_get_value_record",
    "azk_export_tree_quotients", "azk_debug_fill_quotients",
    "azk_set_solver", "azk_clear_solver", "azk_get_solver_status", "azk_export_tree_status", "azk_get_solver_stats",
    "azk_debug_fill_solver_status",
    "azk_set_root_noise", "azk_clear_root_noise", "azk_gen_root_noise", "azk_get_root_noise",
    "azk_set_kld_stop", "azk_clear_kld_stop", "azk_kld_checkpoint", "azk_get_search_sims", "azk_get_kld_rate", "azk_get_kld_stats",
    "azk_async_sims_column", "azk_set_lead_stop", "azk_clear_lead_stop", "azk_get_lead", "azk_get_lead_stats",
]


class AzkError(RuntimeError):
    pass


from . import structs  # noqa: E402
from .structs import (EMBED_FOLD_MAX_SLOTS, EMBED_FOLD_ROW, EMBED_POOL_COMPACT_MAX_SLOTS, GAME_ID, LEAF_BF16, LEAF_F32,  # noqa: E402,F401
                      AsyncConfig, Config, Counters, EmbedFoldConsts, EmbedPoolConsts, EmbedPoolXConsts, GemmH, GemmTok,
                      LeafSource, TailGemm)
from .packing import (GEMM_H_A_SCALE, GEMM_H_W_SCALE, pack_linear_weight, pack_linear_weight128, pack_linear_weight_h,  # noqa: E402,F401
                      packed_weight_col_sums, split_fp16)
from .replay import DeviceReplay  # noqa: E402,F401


def build(force=False, verbose=False):
    """Compile libazk.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "azk.h"))
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    cmd = ["make", "-C", _CSRC, "-j8"] + (["-B"] if force else [])      # one object per kernel family: they compile side by side
    r = subprocess.run(cmd, capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise AzkError("building libazk.so failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


_LIB = None


def lib():
    """Load libazk.so (no GPU needed to load; compute entry points need one)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise AzkError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(the HIP extension is required; there is no CPU fallback)")
    # PyTorch ships its own HIP runtime (libamdhip64.so.7 + libhsa-runtime64); it must be the process's only
    # one, so torch is imported before libazk.so is mapped and the soname resolves to the copy already loaded.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.azk_abi_version.restype = C.c_int32
    if L.azk_abi_version() != ABI_VERSION:
        raise AzkError(f"{LIB_PATH} speaks ABI version {L.azk_abi_version()}, this binding was written for {ABI_VERSION} "
                       "(include/azk.h AZK_ABI_VERSION): rebuild with __graft_entry__.build()")
    structs.declare(L, SYMBOLS)
    _LIB = L
    return L


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise AzkError("no GPU visible: the azk engine runs only on an MI355X (no CPU fallback)")
    return torch


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _np(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ok(rc, name):
    if rc != 0:
        raise AzkError(f"{name} failed ({rc})")


def board_elements(game, size=None):
    """The D4 elements (the emission's numbering: rot0, lr, tb, rot90, lr(rot90), tb(rot90), rot180, rot270) a game's geometry admits
    (include/azk.h azk_set_eval_symmetry): all eight on a square board with one action per cell, {0, 1, 2, 6} on a Gomoku board with
    rows != cols, {0, 1} for Connect4 (gravity)."""
    if game == "connect4":
        return (0, 1)
    rows, cols = (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size or 0), int(size or 0))
    return tuple(range(8)) if game == "tictactoe" or rows == cols else (0, 1, 2, 6)


def emit_mask(emit_symmetry, game, size=None):
    """emit_symmetry -> azk_config.emit_elements: None = 0 (off: the reference's emission), "board" = every element the geometry admits,
    "none" = the identity alone (mask 1: one tuple per ply), an iterable of elements = their bits.  Only the form is checked here (ValueError);
    which masks a geometry admits is azk_create's decision (selfplay.check_emit_symmetry says the same before an engine exists)."""
    if emit_symmetry is None:
        return 0
    if isinstance(emit_symmetry, str):
        if emit_symmetry == "board":
            return sum(1 << s for s in board_elements(game, size))
        if emit_symmetry == "none":
            return 1
        raise ValueError(f"emit_symmetry must be None, 'board', 'none' or an iterable of elements, not {emit_symmetry!r}")
    try:
        items = list(emit_symmetry)
        els = [int(s) for s in items]
        if not els or any(e != s for e, s in zip(els, items)) or any(not 0 <= e < 31 for e in els):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"emit_symmetry must be None, 'board', 'none' or an iterable of elements, not {emit_symmetry!r}")
    return sum(1 << s for s in set(els))


PUCT_TABLE_MAX = 65536                              # azk_set_puct's largest n_table
FPU_MODES = {"absolute": 1, "reduction": 2}


def puct_table(c_init, c_base, n=PUCT_TABLE_MAX):
    """AlphaZero's exploration rate as a table over the selecting node's visit count: math.log((1 + N + c_base) / c_base) + c_init for
    N = 0..n-1, in host float64 (the engine reads entry min(N, n - 1); it has no device log)."""
    c_init, c_base, n = float(c_init), float(c_base), int(n)
    if not 1 <= n <= PUCT_TABLE_MAX:
        raise ValueError(f"puct_table: n must lie in [1, {PUCT_TABLE_MAX}], not {n!r}")
    if not 0.0 < c_base < float("inf") or not 0.0 <= c_init < float("inf"):
        raise ValueError(f"puct_table: c_base must be finite and positive and c_init finite and not negative, not {(c_init, c_base)!r}")
    return np.array([math.log((1 + N + c_base) / c_base) + c_init for N in range(n)], np.float64)


def puct_setting(c, fpu=None):
    """(c, fpu) -> (c_table float64 [n], fpu_mode, fpu_tree, fpu_root), the arguments of azk_set_puct (include/azk.h).
    c: a number (that constant for every visit count), a TUPLE (c_init, c_base) (puct_table over the whole 65536 entries), or a list / array of
    table entries.  fpu: None (an unvisited child scores as the reference's), ("absolute", v_tree[, v_root]) or ("reduction", r_tree[, r_root]);
    the root's parameter defaults to the tree's.  Raises ValueError for what the engine refuses too."""
    try:
        if isinstance(c, bool):
            raise TypeError
        if isinstance(c, tuple) and len(c) == 2:
            table = puct_table(c[0], c[1])
        elif isinstance(c, (int, float, np.integer, np.floating)):
            table = np.array([float(c)], np.float64)
        else:
            table = np.ascontiguousarray([float(x) for x in c], np.float64)
    except TypeError:
        raise ValueError(f"puct: c must be a number, a tuple (c_init, c_base) or a list of table entries, not {c!r}")
    if not 1 <= table.size <= PUCT_TABLE_MAX:
        raise ValueError(f"puct: the table must have 1..{PUCT_TABLE_MAX} entries, not {table.size}")
    if not (np.isfinite(table).all() and (table >= 0.0).all()):
        raise ValueError("puct: every table entry must be finite and not negative")
    if fpu is None:
        return table, 0, 0.0, 0.0
    try:
        kind, f_tree = fpu[0], float(fpu[1])
        f_root = float(fpu[2]) if len(fpu) == 3 else f_tree
        if len(fpu) not in (2, 3) or kind not in FPU_MODES:
            raise ValueError
    except (TypeError, ValueError, IndexError, KeyError):
        raise ValueError(f"puct: fpu must be None, ('absolute', v_tree[, v_root]) or ('reduction', r_tree[, r_root]), not {fpu!r}")
    if not (math.isfinite(f_tree) and math.isfinite(f_root)):
        raise ValueError(f"puct: the FPU parameters must be finite, not {fpu!r}")
    if kind == "reduction" and (f_tree < 0.0 or f_root < 0.0):
        raise ValueError(f"puct: a reduction must not be negative, not {fpu!r}")
    return table, FPU_MODES[kind], f_tree, f_root


def _tau_schedule(tau, state_dim):
    """tau in one of move_temperature_setting's forms -> the per-ply list of float values (0.0 = greedy); the last holds for every later ply."""
    if isinstance(tau, bool):
        raise TypeError
    if isinstance(tau, (int, float, np.integer, np.floating)):
        return [float(tau)]
    if isinstance(tau, tuple) and len(tau) > 0 and isinstance(tau[0], str):
        kind, rest = tau[0], tau[1:]
        if kind == "until" and len(rest) == 2:
            t, n = float(rest[0]), int(rest[1])
            if n != rest[1] or n < 0:
                raise TypeError
            return [t] * min(n, int(state_dim)) + [0.0]
        if kind in ("halflife", "linear") and len(rest) in (2, 3):
            t0, span = float(rest[0]), float(rest[1])
            t_final = float(rest[2]) if len(rest) == 3 else 0.0
            if not (span > 0.0 and math.isfinite(span)):
                raise TypeError
            if kind == "halflife":
                return [t_final + (t0 - t_final) * 0.5 ** (p / span) for p in range(int(state_dim))]
            return [t0 + (t_final - t0) * (min(float(p), span) / span) for p in range(int(state_dim))]
        raise TypeError
    if isinstance(tau, (list, np.ndarray)) and len(tau) > 0:
        return [float(t) for t in tau]
    raise TypeError


def move_temperature_setting(tau, max_sims, state_dim, visit_offset=0, value_cutoff=None):
    """tau -> (row_of_ply int32 [n_plies], weights float64 [n_rows][max_sims + 1], visit_offset, value_cutoff), the arguments of
    azk_set_move_temperature (include/azk.h).  tau: a positive number (every ply), ("until", t, n_plies) (t for the first
    n_plies plies, then greedy), ("halflife", t0, halflife[, t_final]) (tau(p) = t_final + (t0 - t_final) * 0.5 ** (p / halflife) for
    p < state_dim), ("linear", t0, decay_plies[, t_final]) (tau(p) = t0 + (t_final - t0) * min(p, decay_plies) / decay_plies), t_final 0
    where it is left out, or a list of per-ply values whose last holds for every later ply.  A value of 0 is greedy (row -1); equal values share
    one row; a row is [math.pow(float(n), 1.0 / tau) for n in range(max_sims + 1)] in host float64 (the engine has no device pow).
    value_cutoff None (or negative) = no cutoff.  Raises ValueError for what the engine refuses too; where a row would overflow the engine's
    bound on a weight, DBL_MAX / (rows * columns), the message names the smallest admissible tau."""
    max_sims, state_dim = int(max_sims), int(state_dim)
    try:
        taus = _tau_schedule(tau, state_dim)
    except (TypeError, ValueError):
        raise ValueError("move_temperature: tau must be a positive number, ('until', t, n_plies), ('halflife', t0, halflife[, t_final]), "
                         f"('linear', t0, decay_plies[, t_final]) or a list of per-ply values, not {tau!r}")
    if max_sims < 1 or state_dim < 1:
        raise ValueError(f"move_temperature: max_sims and state_dim must be at least 1, not {(max_sims, state_dim)!r}")
    if not all(math.isfinite(t) and t >= 0.0 for t in taus):
        raise ValueError(f"move_temperature: every tau must be finite and not negative (0 = greedy), not {tau!r}")
    if isinstance(visit_offset, bool) or int(visit_offset) != visit_offset or int(visit_offset) < 0:
        raise ValueError(f"move_temperature: visit_offset must be an integer >= 0, not {visit_offset!r}")
    cutoff = -1.0 if value_cutoff is None else float(value_cutoff)
    if math.isnan(cutoff):
        raise ValueError("move_temperature: value_cutoff is NaN (None or a negative value means no cutoff)")
    distinct = []
    for t in taus:
        if t > 0.0 and t not in distinct:
            distinct.append(t)
    if not distinct:
        raise ValueError(f"move_temperature: no ply has a positive tau in {tau!r} - that is the engine without the option at sample_until 0")
    n_cols = max_sims + 1
    bound = sys.float_info.max / (len(distinct) * n_cols)
    tau_min = math.log(max_sims) / math.log(bound) if max_sims > 1 else 0.0
    rows = []
    for t in distinct:
        try:
            row = [math.pow(float(n), 1.0 / t) for n in range(n_cols)]
        except (OverflowError, ZeroDivisionError):
            row = [math.inf]
        if max(row) > bound:
            raise ValueError(f"move_temperature: tau = {t!r} overflows the table - {max_sims} ** (1 / tau) must stay below DBL_MAX / (rows * columns) = "
                             f"{bound:.6g}; the smallest admissible tau for {len(distinct)} row(s) of {n_cols} columns is {tau_min:.6g}")
        rows.append(row)
    row_of_ply = np.array([distinct.index(t) if t > 0.0 else -1 for t in taus], np.int32)
    return row_of_ply, np.ascontiguousarray(rows, np.float64), int(visit_offset), cutoff


class Engine:
    """G concurrent games + their search trees resident on one GPU (one engine per process / GPU)."""

    def __init__(self, game, n_games, max_sims, size=None, device=0, leaf_dtype="float32", arena_nodes=0, cache_entries=0,
                 cache_shared=False, leaves_per_step=1, tree_reuse=0, eval_symmetry=None, emit_symmetry=None):
        torch = _torch()
        self.torch = torch
        self.L = lib()
        self.game = game
        cfg = Config()
        cfg.game = GAME_ID[game]
        cfg.rows, cfg.cols = (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size or 0), int(size or 0))   # (rows, cols) or one side
        cfg.n_games, cfg.max_sims, cfg.device, cfg.arena_nodes = int(n_games), int(max_sims), int(device), int(arena_nodes)
        cfg.cache_entries = int(cache_entries)
        cfg.cache_shared = 1 if (cache_shared and cache_entries) else 0      # one table for all games (the reference's process-global MCTS.cache)
        self.cache_shared = bool(cfg.cache_shared)
        # OPT-IN virtual-loss expansion: K leaves in flight per game (changes search results; 1 = the reference's sequential search)
        self.K = max(1, int(leaves_per_step))
        cfg.leaves_per_step = self.K
        # OPT-IN tree reuse across moves (changes search results): 1 = carry (n_sims new simulations on the carried subtree), 2 = top-up
        # (only as many as bring the root back to n_sims visits; budget stepping only).  0 = a fresh root every move, the reference's search
        self.tree_reuse = int(tree_reuse)
        cfg.tree_reuse = self.tree_reuse
        # OPT-IN (state, pi, z) emission under a mask of D4 elements, on every geometry (azk.h azk_config.emit_elements):
        # None = the reference's emission, "board" = every element the geometry admits, "none" = one tuple per ply, or an iterable of elements
        cfg.emit_elements = emit_mask(emit_symmetry, game, size)
        cfg.leaf_dtype = LEAF_BF16 if leaf_dtype in ("bfloat16", "bf16", torch.bfloat16) else LEAF_F32
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        rc = self.L.azk_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise AzkError(f"azk_create failed ({rc}): {self.L.azk_last_error(None).decode()}")
        self.h = h
        vals = [C.c_int32() for _ in range(5)]
        self._chk(self.L.azk_geometry(self.h, *[C.byref(v) for v in vals]))
        self.planes, self.rows, self.cols, self.action_dim, self.state_dim = [v.value for v in vals]
        self.G, self.max_sims = int(n_games), int(max_sims)
        vals = [C.c_int32(), C.c_int32()]
        self._chk(self.L.azk_emit_elements(self.h, C.byref(vals[0]), C.byref(vals[1])))
        # the engine's emission mask (0 = off) and its tuples per ply from the third on (8 with the option off on a square board, 0 where
        # emission is refused): a finished game of p plies fills p <= 2 ? p : 2 + emit_group * (p - 2) ring slots
        self.emit_elements, self.emit_group = vals[0].value, vals[1].value
        tdt = torch.bfloat16 if cfg.leaf_dtype == LEAF_BF16 else torch.float32
        dev = self.device
        self.slots = self.G * self.K                # pending-leaf slots = capacity of one evaluator batch
        self.leaf_boards = torch.zeros((self.slots, self.planes, self.rows, self.cols), dtype=tdt, device=dev)
        self.n_leaf = torch.zeros(1, dtype=torch.int32, device=dev)
        self.pi = torch.zeros((self.G, self.action_dim), dtype=torch.float64, device=dev)
        self.q = torch.zeros(self.G, dtype=torch.float64, device=dev)
        self.root_visit = torch.zeros(self.G, dtype=torch.int32, device=dev)
        self.chosen = torch.zeros(self.G, dtype=torch.int32, device=dev)
        self.winner = torch.zeros(self.G, dtype=torch.int32, device=dev)
        self.done = torch.zeros(self.G, dtype=torch.int32, device=dev)
        self._noise = None
        self.playout_cap = None                     # (p_full, n_fast) once set_playout_cap has switched the option on
        self.resign = None                          # (v_resign, p_never, min_ply) once set_resign has switched the option on
        self.forced_playouts = None                 # k once set_forced_playouts has switched the option on
        self.gumbel_root = None                     # (m, n_sims, c_visit, c_scale) once set_gumbel_root has switched the option on
        self.openings = None                        # (p_open, max_plies, spread) once set_openings has switched the option on
        self.root_noise = None                      # ("legal" | "total", alpha) once set_root_noise has switched the option on
        self.puct = None                            # (c_table, fpu_mode, fpu_tree, fpu_root) once set_puct has switched the option on
        self.solver = False                         # True once set_solver has switched the option on
        self.move_temperature = None                # (row_of_ply, weights, visit_offset, value_cutoff) once set_move_temperature has switched the option on
        self.surprise_weight = None                 # lambda once set_surprise_weighting has switched the option on (0.0 is a live setting)
        self.value_target = None                    # (r, lam) once set_value_target has switched the option on (r = 0.0 is a live setting)
        self.kld_stop = None                        # (interval, min_gain, min_sims) once set_kld_stop has switched the option on
        self.lead_stop = None                       # (interval, factor, min_sims) once set_lead_stop has switched the option on
        self.cache_entries = int(cache_entries)
        # with the eval cache a step can have pending (cached) leaves to expand although no leaf went to the evaluator
        need = cache_entries or self.K > 1
        self._no_logits = torch.zeros((1, self.action_dim), dtype=torch.float32, device=dev) if need else None
        self._no_values = torch.zeros(1, dtype=torch.float32, device=dev) if need else None
        self.eval_symmetry = None                   # (mode, value) once set_eval_symmetry has switched the option on
        if eval_symmetry is not None:
            self.set_eval_symmetry(*eval_symmetry)

    def _chk(self, rc):
        if rc < 0:
            raise AzkError(f"libazk error {rc}: {self.L.azk_last_error(self.h).decode()}")
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.azk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----------------------------------------------------------------------------------
    def reset_games(self, first=0, count=None):
        self._chk(self.L.azk_reset_games(self.h, first, self.G - first if count is None else count, _stream()))

    def set_positions(self, cells, to_move, move_count, first=0):
        cells = np.ascontiguousarray(cells, np.int8).reshape(-1, self.rows * self.cols)
        tm = np.ascontiguousarray(to_move, np.int32)
        mc = np.ascontiguousarray(move_count, np.int32)
        self._chk(self.L.azk_set_positions(self.h, first, len(cells), _np(cells), _np(tm), _np(mc), _stream()))

    def get_positions(self):
        cells = np.empty((self.G, self.rows * self.cols), np.int8)
        tm = np.empty(self.G, np.int32)
        mc = np.empty(self.G, np.int32)
        self._chk(self.L.azk_get_positions(self.h, _np(cells), _np(tm), _np(mc), _stream()))
        return cells, tm, mc

    # ---- search ---------------------------------------------------------------------------------
    def begin_search(self, noise=None):
        """noise: float64 CUDA tensor [G, A] (np.random.dirichlet draws) or None (dirichlet=False)."""
        if noise is not None:
            assert noise.dtype == self.torch.float64 and noise.is_cuda and noise.is_contiguous()
            assert tuple(noise.shape) == (self.G, self.action_dim)
        self._noise = noise     # keep alive for the whole search
        self._chk(self.L.azk_begin_search(self.h, _p(noise), _stream()))

    def set_playout_cap(self, p_full, n_fast, seed=0, first_global_game=0):
        """OPT-IN playout-cap randomisation (azk_set_playout_cap): from now on every search is FULL (n_sims simulations) with probability
        p_full and FAST (n_fast simulations) otherwise, by a coin keyed (seed, first_global_game + g, move key); only the plies of full
        searches are emitted as (state, pi, z).  Searches then begin with begin_search_budget(..., move_index=...) (lock-step) or
        async_begin (which keys the coins by its own seed / first game).  n_fast = 0 switches it off."""
        self._chk(self.L.azk_set_playout_cap(self.h, float(p_full), int(n_fast), int(seed), int(first_global_game), _stream()))
        self.playout_cap = (float(p_full), int(n_fast)) if int(n_fast) else None
        if self.playout_cap and getattr(self, "_search_full", None) is None:
            self._search_full = self.torch.ones(self.G, dtype=self.torch.uint8, device=self.device)

    def search_full(self):
        """uint8 CUDA tensor [G]: 1 = the game's current search is a full one (azk_get_search_full; valid until the next call)."""
        if self.playout_cap is None:
            raise AzkError("search_full: no playout cap is set (set_playout_cap)")
        self._chk(self.L.azk_get_search_full(self.h, _p(self._search_full), _stream()))
        return self._search_full

    def set_openings(self, p_open, max_plies, spread=-1, seed=0, first_global_game=0):
        """OPT-IN random openings (azk_set_openings): from now on a game that starts in a slot is, with probability p_open,
        played forward 1..max_plies uniformly drawn legal plies inside the centred window of half-width `spread` (-1: the whole board) before
        its first search, by draws keyed (seed, first_global_game + g, move key of that search).  Lock-step drivers call open_pending(key)
        after the games were reset (key 0) and after recycle_finished (key = the next move index); the asynchronous movers open their games
        themselves.  Those plies are not emitted as (state, pi, z).  p_open = 0 is a live setting; clear_openings switches the option off."""
        self._chk(self.L.azk_set_openings(self.h, float(p_open), int(max_plies), int(spread), int(seed) & ((1 << 64) - 1), int(first_global_game),
                                          _stream()))
        self.openings = (float(p_open), int(max_plies), int(spread))
        if getattr(self, "_open_plies", None) is None:
            self._open_plies = self.torch.zeros(self.G, dtype=self.torch.int32, device=self.device)

    def clear_openings(self):
        """Random openings off (azk_clear_openings): the engine launches what it launched before."""
        self._chk(self.L.azk_clear_openings(self.h))
        self.openings = None

    def open_pending(self, key):
        """Open the games that have just started (azk_open_pending): key = the move index of the search that follows."""
        if self.openings is None:
            raise AzkError("open_pending: no openings are set (set_openings)")
        self._chk(self.L.azk_open_pending(self.h, int(key), _stream()))

    def open_plies(self):
        """int32 CUDA tensor [G]: the opening plies of each slot's current game, 0 = not opened (azk_get_open_plies; valid until the next call)."""
        if self.openings is None:
            raise AzkError("open_plies: no openings are set (set_openings)")
        self._chk(self.L.azk_get_open_plies(self.h, _p(self._open_plies), _stream()))
        return self._open_plies

    def opening_actions(self):
        """Per slot, the cells its current game's opening was played on, in order: a list of G lists (azk_get_opening_actions; host sync)."""
        if self.openings is None:
            raise AzkError("opening_actions: no openings are set (set_openings)")
        acts = self.torch.zeros((self.G, self.state_dim), dtype=self.torch.int16, device=self.device)
        self._chk(self.L.azk_get_opening_actions(self.h, _p(acts), _stream()))
        plies, acts = self.open_plies().cpu().numpy(), acts.cpu().numpy()
        return [[int(c) for c in acts[g, :plies[g]]] for g in range(self.G)]

    def leaf_flags(self):
        """uint8 CUDA tensor [G * K]: non-zero = the slot has a row in the evaluator batch of the step that has just selected, rows in
        ascending slot order (azk_get_leaf_flags; valid until the next call)."""
        if getattr(self, "_leaf_flags", None) is None:
            self._leaf_flags = self.torch.zeros(self.slots, dtype=self.torch.uint8, device=self.device)
        self._chk(self.L.azk_get_leaf_flags(self.h, _p(self._leaf_flags), _stream()))
        return self._leaf_flags

    def opening_stats(self):
        """[games opened, opening plies played, openings cut short] (host sync)."""
        if self.openings is None:
            raise AzkError("opening_stats: no openings are set (set_openings)")
        out = np.zeros(3, np.int64)
        self._chk(self.L.azk_get_opening_stats(self.h, _np(out), _stream()))
        return [int(x) for x in out]

    def set_resign(self, v_resign, p_never=0.0, min_ply=0, seed=0, first_global_game=0):
        """OPT-IN resignation (azk_set_resign): from now on, after a move that does not end the game, the side that has just moved concedes
        when the root's q (root_stats' q as it is: the outcome for the OPPONENT of the side to move, near +1 when the mover is lost) is
        >= v_resign and the game has at least min_ply plies.  A coin keyed (seed, first_global_game + g, move key of the game's first search)
        makes a share p_never of the games never-resign games, which are only marked.  Moves are then made with advance(..., move_index=...)
        (lock-step) or by the asynchronous movers (async_begin keys the coin by its own seed / first game).  v_resign = 0 switches it off."""
        self._chk(self.L.azk_set_resign(self.h, float(v_resign), int(min_ply), float(p_never), int(seed), int(first_global_game), _stream()))
        self.resign = (float(v_resign), float(p_never), int(min_ply)) if float(v_resign) != 0.0 else None
        if self.resign and getattr(self, "_resigned", None) is None:
            self._resigned = self.torch.zeros(self.G, dtype=self.torch.uint8, device=self.device)

    def resigned(self):
        """uint8 CUDA tensor [G]: 1 = the game's last move ended it by resignation (azk_get_resigned; valid until the next call)."""
        if self.resign is None:
            raise AzkError("resigned: no resignation is set (set_resign)")
        self._chk(self.L.azk_get_resigned(self.h, _p(self._resigned), _stream()))
        return self._resigned

    def resign_stats(self):
        """[games ended by resignation, never-resign games ended, of those marked, of those whose marked side did not lose] (host sync)."""
        if self.resign is None:
            raise AzkError("resign_stats: no resignation is set (set_resign)")
        out = np.zeros(4, np.int64)
        self._chk(self.L.azk_get_resign_stats(self.h, _np(out), _stream()))
        return [int(x) for x in out]

    def set_forced_playouts(self, k):
        """OPT-IN forced playouts and policy target pruning at the root (azk_set_forced_playouts; KataGo's k is 2): in every search with
        root noise - on a capped engine every FULL one - a root child with N >= 1 visits and mixed prior P is selected first while
        N * N < (k * P) * (root visits - 1), and the pi that advance / the asynchronous movers RECORD loses the visits only that floor
        explains (root_policy_target shows it).  The move, root_stats, q, resignation and tree reuse keep raw visits.  k = 0 switches it off."""
        self._chk(self.L.azk_set_forced_playouts(self.h, float(k), _stream()))
        self.forced_playouts = float(k) if float(k) != 0.0 else None

    def set_puct(self, c, fpu=None):
        """OPT-IN configurable PUCT (azk_set_puct): from now on every selection scores a child
        Q + c * P * sqrt(Np) / (N + 1), c = the table's word at the selecting node's visit count, and an unvisited child as the first-play
        urgency says.  c: a number, a tuple (c_init, c_base) (AlphaZero's log schedule, puct_table) or a list / array of table entries;
        fpu: None (the reference's: an unvisited child's Q counts 0), ("absolute", v_tree[, v_root]) or ("reduction", r_tree[, r_root]) - the
        selecting node's own value minus r * sqrt(prior mass of its visited children).  set_puct(1.0) searches the trees of an engine without
        the option.  Between searches only; not with forced playouts, a Gumbel root, leaves_per_step > 1 or vanilla_search.  clear_puct()
        switches it off."""
        table, mode, f_tree, f_root = puct_setting(c, fpu)
        self._chk(self.L.azk_set_puct(self.h, _np(table), int(table.size), mode, f_tree, f_root, _stream()))
        self.puct = (table, mode, f_tree, f_root)

    def clear_puct(self):
        """Configurable PUCT off (azk_clear_puct): the engine launches what it launched before."""
        self._chk(self.L.azk_clear_puct(self.h))
        self.puct = None

    def set_solver(self, on=True):
        """OPT-IN exact game-end proofs in the search (azk_set_solver): every node keeps a status - unknown, won, lost,
        draw for the player who moved into it - proven from terminal leaves up the path of the simulation that found them; the walk stops on
        proven nodes below the root and selection shuts out children proven lost.  Between searches only; not with forced playouts, a Gumbel
        root, configurable PUCT, tree reuse, leaves_per_step > 1 or vanilla_search.  set_solver(False) switches it off (azk_clear_solver)."""
        if on:
            self._chk(self.L.azk_set_solver(self.h, _stream()))
        else:
            self._chk(self.L.azk_clear_solver(self.h))
        self.solver = bool(on)

    def solver_status(self):
        """int8 [G]: every root's status as the side to move there sees it - 0 unknown, 1 wins, 2 loses, 3 draw (azk_get_solver_status)."""
        out = np.empty(self.G, np.int8)
        self._chk(self.L.azk_get_solver_status(self.h, _np(out), _stream()))
        return out

    def export_tree_status(self, game, cap=None):
        """uint8 [nodes]: the stored statuses (0 unknown, 1 won, 2 lost, 3 draw for the player who moved INTO the node) in export_tree's row order."""
        cap = cap or (1 + self.max_sims * self.rows * self.cols)
        out = np.empty(cap, np.uint8)
        n = self._chk(self.L.azk_export_tree_status(self.h, int(game), cap, _np(out), _stream()))
        return out[:min(n, cap)]

    def solver_stats(self):
        """The six counters since set_solver (azk_get_solver_stats): terminal leaves marked, nodes proven by one won child, nodes proven by
        all their children, simulations ended on a proven node with children, selections that shut a child out, roots that took a status."""
        out = np.zeros(6, np.int64)
        self._chk(self.L.azk_get_solver_stats(self.h, _np(out), _stream()))
        keys = ("terminal_marked", "proven_by_won_child", "proven_by_all_children", "stopped_on_proven", "selections_excluding", "roots_proven")
        return dict(zip(keys, (int(v) for v in out)))

    def fill_solver_status(self, byte):
        """Tests only: every byte of the status column becomes `byte`.  For engines whose trees are fresh roots."""
        self._chk(self.L.azk_debug_fill_solver_status(self.h, int(byte), _stream()))

    def set_move_temperature(self, row_of_ply, weights, visit_offset=0, value_cutoff=None):
        """OPT-IN move temperature (azk_set_move_temperature): from now on advance and the asynchronous movers ignore
        sample_until and pick the played child by the table - at a move of a game with mc plies, row r = row_of_ply[min(mc, len - 1)]; r < 0
        (or no uniforms) plays the first most-visited child b; otherwise child i weighs weights[r][max(0, N_i - visit_offset)], a child whose
        W / N lies more than value_cutoff below b's weighs 0, and the child is drawn from those weights as Node.sample_child draws from the
        counts.  move_temperature_setting builds the four arguments from a temperature schedule.  weights: float64 [n_rows][max_sims + 1].
        value_cutoff None or negative = no cutoff.  The recorded pi stays the raw visit distribution.  Between searches only; not with a Gumbel
        root or tree_reuse = 1.  clear_move_temperature() switches it off."""
        rows = np.ascontiguousarray(row_of_ply, np.int32).reshape(-1)
        wts = np.ascontiguousarray(weights, np.float64)
        if wts.ndim != 2:
            raise ValueError(f"set_move_temperature: weights must be [n_rows][max_sims + 1], not an array of shape {wts.shape!r}")
        cutoff = -1.0 if value_cutoff is None else float(value_cutoff)
        self._chk(self.L.azk_set_move_temperature(self.h, _np(rows), int(rows.size), _np(wts), int(wts.shape[0]), int(wts.shape[1]), int(visit_offset),
                                                  cutoff, _stream()))
        self.move_temperature = (rows, wts, int(visit_offset), cutoff)

    def clear_move_temperature(self):
        """Move temperature off (azk_clear_move_temperature): the engine launches what it launched before."""
        self._chk(self.L.azk_clear_move_temperature(self.h))
        self.move_temperature = None

    def move_temperature_stats(self):
        """[plies drawn by weight, of those not the most-visited child, children cut by the value cutoff, plies that fell back to the
        most-visited child because every weight was 0] since set_move_temperature (host sync)."""
        if self.move_temperature is None:
            raise AzkError("move_temperature_stats: no move temperature is set (set_move_temperature)")
        out = np.zeros(4, np.int64)
        self._chk(self.L.azk_get_move_temperature_stats(self.h, _np(out), _stream()))
        return [int(x) for x in out]

    def set_gumbel_root(self, m, n_sims, c_visit=50.0, c_scale=1.0):
        """OPT-IN Gumbel root search (azk_set_gumbel_root; Danihelka et al. 2022): every search of n_sims simulations
        samples m root actions by Gumbel-top-k, spreads its simulations over them by sequential halving, and advance / the asynchronous
        movers play the survivor and RECORD softmax(logits + sigma(completed Q)) (root_policy_target shows it).  The noise argument of
        begin_search / search / search_budget then carries Gumbel rows (gen_gumbel; zeros = the noise-free search), and advance ignores
        its uniforms.  root_stats, q, resignation and the counters keep raw visits."""
        self._chk(self.L.azk_set_gumbel_root(self.h, int(m), int(n_sims), float(c_visit), float(c_scale), _stream()))
        self.gumbel_root = (int(m), int(n_sims), float(c_visit), float(c_scale))

    def clear_gumbel_root(self):
        self._chk(self.L.azk_clear_gumbel_root(self.h))
        self.gumbel_root = None

    def gen_gumbel(self, seed, first_global_game, move_index, uniforms=False):
        """float64 CUDA tensor [G, A]: the games' Gumbel(0, 1) rows of (seed, first_global_game + g, move_index) (azk_gen_gumbel), or with
        uniforms=True the uniforms underneath them (azk_gen_gumbel_uniforms)."""
        rows = self.torch.empty((self.G, self.action_dim), dtype=self.torch.float64, device=self.device)
        fn = self.L.azk_gen_gumbel_uniforms if uniforms else self.L.azk_gen_gumbel
        self._chk(fn(self.h, int(seed), int(first_global_game), int(move_index), _p(rows), _stream()))
        return rows

    def set_surprise_weighting(self, lam, seed=0, first_global_game=0):
        """OPT-IN policy surprise weighting (azk_set_surprise_weighting): from now on every move records kl = KL(recorded pi ||
        the network's raw prior over the root's children) and a coin keyed (seed, first_global_game + g, move key), and a finished game's
        recorded ply i is emitted floor(w_i) + (coin_i < frac(w_i)) times, w_i = (1 - lam) + lam * n * kl_i / sum(kl) - n tuple groups per game
        in expectation, as without the option.  lam in [0, 1]; lam = 0 still records kl and coin and emits the option-off ring.  Moves are
        then made with advance(..., move_index=...) (lock-step) or by the asynchronous movers (async_begin keys the coin by its own seed /
        first game).  lam = None switches it off (azk_clear_surprise_weighting)."""
        if lam is None:
            self._chk(self.L.azk_clear_surprise_weighting(self.h))
            self.surprise_weight = None
            return
        self._chk(self.L.azk_set_surprise_weighting(self.h, float(lam), int(seed), int(first_global_game), _stream()))
        self.surprise_weight = float(lam)
        if getattr(self, "_surprise", None) is None:
            self._surprise = (self.torch.zeros(self.G, dtype=self.torch.float64, device=self.device),
                              self.torch.zeros(self.G, dtype=self.torch.float64, device=self.device))

    def surprise(self):
        """(kl, coin): float64 CUDA tensors [G], what each game's last move recorded (azk_get_surprise; valid until the next call)."""
        if self.surprise_weight is None:
            raise AzkError("surprise: no surprise weighting is set (set_surprise_weighting)")
        self._chk(self.L.azk_get_surprise(self.h, _p(self._surprise[0]), _p(self._surprise[1]), _stream()))
        return self._surprise

    def set_value_target(self, r, lam=0.0):
        """OPT-IN value targets (azk_set_value_target): from now on every move keeps the root's q = W / N beside its pi
        (value_record shows it) and emission - emit_finished, the asynchronous drain - writes t_i = (1 - r) * z_i + r * G_i in place of z_i,
        G the horizon-lam return over the game's own search values v_i = -q_i that ends in z:  G_{n-1} = (1 - lam) * v_{n-1} + lam * z_{n-1},
        G_i = (1 - lam) * v_i + lam * (-G_{i+1}).  r, lam in [0, 1]: (r, 0) is Leela's q-ratio, (1, lam) a TD(lambda) return; (0, lam) and
        (1, 1) write the option-off ring byte for byte.  States and pis do not change.  Not with a Gumbel root or leaves_per_step > 1;
        before async_begin.  r = None switches it off (azk_clear_value_target)."""
        if r is None:
            self._chk(self.L.azk_clear_value_target(self.h))
            self.value_target = None
            return
        self._chk(self.L.azk_set_value_target(self.h, float(r), float(lam), _stream()))
        self.value_target = (float(r), float(lam))

    def value_record(self):
        """float64 CUDA tensor [G, state_dim]: q of the plies of each slot's current game, as the movers kept them (azk_get_value_record);
        row g is valid up to the game's move count (entries before its first searched ply, and beyond its last, are older games' or 0)."""
        if self.value_target is None:
            raise AzkError("value_record: no value target is set (set_value_target)")
        out = self.torch.empty((self.G, self.state_dim), dtype=self.torch.float64, device=self.device)
        self._chk(self.L.azk_get_value_record(self.h, _p(out), _stream()))
        return out

    def set_eval_symmetry(self, mode, value=0):
        """OPT-IN evaluation under a board symmetry (azk_set_eval_symmetry): the evaluator sees every pending leaf turned by a D4 element
        and its logits row is turned back before the tree expands from it.  mode 1 (or "position"): the element is a hash of (seed = value,
        the leaf's position), so the evaluator stays a function of the position and cache modes, budget stepping, tree reuse and the
        asynchronous movers keep their bit-for-bit equivalences; mode 2 (or "fixed"): element `value` for every leaf; mode 0: off.  Between
        searches only (before async_begin)."""
        mode = {"off": 0, "position": 1, "fixed": 2}.get(mode, mode)
        self._chk(self.L.azk_set_eval_symmetry(self.h, int(mode), int(value), _stream()))
        self.eval_symmetry = (int(mode), int(value)) if int(mode) else None
        self._leaf_source = None                    # the cached struct holds the cells pointer of the mode it was made under
        if self.eval_symmetry and getattr(self, "_leaf_sym", None) is None:
            self._leaf_sym = self.torch.zeros(self.G, dtype=self.torch.uint8, device=self.device)

    def leaf_symmetry(self):
        """uint8 CUDA tensor [G]: the element each game's pending leaf is evaluated under (azk_get_leaf_symmetry; meaningful for the games
        whose leaf went to the evaluator in the last step; valid until the next call)."""
        if self.eval_symmetry is None:
            raise AzkError("leaf_symmetry: no evaluation symmetry is set (set_eval_symmetry)")
        self._chk(self.L.azk_get_leaf_symmetry(self.h, _p(self._leaf_sym), _stream()))
        return self._leaf_sym

    def restore_logits(self, logits, out=None):
        """The restore step alone (azk_eval_symmetry_restore): rows of `logits` (float32 [n, A], in the order of the last step's leaves) turned
        back into each position's frame, into `out` (default: a copy of logits) - rows that belong to no pending leaf are left alone."""
        if self.eval_symmetry is None:
            raise AzkError("restore_logits: no evaluation symmetry is set (set_eval_symmetry)")
        assert logits.dtype == self.torch.float32 and logits.is_cuda and logits.is_contiguous() and logits.shape[-1] == self.action_dim
        out = logits.clone() if out is None else out
        assert out.dtype == self.torch.float32 and out.is_contiguous() and out.shape == logits.shape and out.data_ptr() != logits.data_ptr()
        self._chk(self.L.azk_eval_symmetry_restore(self.h, _p(logits), _p(out), _stream()))
        return out

    def root_policy_target(self):
        """float64 CUDA tensor [G, A]: the pi the next advance would record for each game (azk_root_policy_target; valid until the next
        call).  With forced playouts off, or for a game whose search is a fast one, root_stats' pi bit for bit."""
        if getattr(self, "_pi_target", None) is None:
            self._pi_target = self.torch.empty((self.G, self.action_dim), dtype=self.torch.float64, device=self.device)
        self._chk(self.L.azk_root_policy_target(self.h, _p(self._pi_target), _stream()))
        return self._pi_target

    def set_kld_stop(self, interval, min_gain, min_sims=0):
        """OPT-IN adaptive search budgets (azk_set_kld_stop): from now on a search runs in segments of `interval` simulations
        and ends at the first checkpoint between two segments at which the KL divergence its root's visit distribution gained per simulation
        since the last checkpoint is below min_gain (not before it has run min_sims new simulations), or when its allowance is used up.  The
        lock-step search is search_budget (plain stepping is refused); the asynchronous movers judge their games themselves.  Not with a
        Gumbel root or leaves_per_step > 1; before async_begin and outside a search.  clear_kld_stop switches it off."""
        self._chk(self.L.azk_set_kld_stop(self.h, int(interval), float(min_gain), int(min_sims), _stream()))
        self.kld_stop = (int(interval), float(min_gain), int(min_sims))

    def clear_kld_stop(self):
        """Adaptive search budgets off (azk_clear_kld_stop): the engine launches what it launched before."""
        self._chk(self.L.azk_clear_kld_stop(self.h))
        self.kld_stop = None

    def set_lead_stop(self, interval, factor, min_sims=0):
        """OPT-IN adaptive search budgets, the lead rule (azk_set_lead_stop): from now on a search runs in segments of
        `interval` simulations and ends at the first checkpoint between two segments at which the most-visited root child leads the second
        by so much that  left < factor * (N1 - N2)  (not before it has run min_sims new simulations), at a root with a single child, or when
        its allowance is used up.  At factor 1 the first most-visited child is the full search's.  Driven like set_kld_stop, alone or beside
        it (one interval for both); the same refusals.  clear_lead_stop switches it off."""
        self._chk(self.L.azk_set_lead_stop(self.h, int(interval), float(factor), int(min_sims), _stream()))
        self.lead_stop = (int(interval), float(factor), int(min_sims))

    def clear_lead_stop(self):
        """The lead rule off (azk_clear_lead_stop): the engine launches what it launched before."""
        self._chk(self.L.azk_clear_lead_stop(self.h))
        self.lead_stop = None

    @property
    def adaptive(self):
        """Is a search of this engine cut into segments - is either rule of adaptive search budgets set?"""
        return self.kld_stop is not None or self.lead_stop is not None

    def lead(self):
        """int32 CUDA tensor [G][3]: N1, N2 and left at each game's last judged lead checkpoint (azk_get_lead; valid until the next call)."""
        if self.lead_stop is None:
            raise AzkError("lead: no lead rule is set (set_lead_stop)")
        if getattr(self, "_lead", None) is None:
            self._lead = self.torch.zeros((self.G, 3), dtype=self.torch.int32, device=self.device)
        self._chk(self.L.azk_get_lead(self.h, _p(self._lead), _stream()))
        return self._lead

    def lead_stats(self):
        """The five counters since set_lead_stop (azk_get_lead_stats): checkpoints judged, searches ended early, simulations those searches
        left unrun, forced-move ends, searches that ran their allowance."""
        if self.lead_stop is None:
            raise AzkError("lead_stats: no lead rule is set (set_lead_stop)")
        out = np.zeros(5, np.int64)
        self._chk(self.L.azk_get_lead_stats(self.h, _np(out), _stream()))
        return dict(judged=int(out[0]), ended_early=int(out[1]), sims_unrun=int(out[2]), forced=int(out[3]), ran_allowance=int(out[4]))

    def kld_checkpoint(self):
        """Judge every game whose segment is complete (azk_kld_checkpoint; host sync): returns how many games were released for another
        segment - 0: every search is over, move."""
        out = C.c_int32(0)
        self._chk(self.L.azk_kld_checkpoint(self.h, C.byref(out), _stream()))
        return int(out.value)

    def search_sims(self):
        """int32 CUDA tensor [G]: the new simulations each game's current or last-judged search has run (azk_get_search_sims; valid until
        the next call)."""
        if not self.adaptive:
            raise AzkError("search_sims: no adaptive search budget is set (set_kld_stop / set_lead_stop)")
        if getattr(self, "_search_sims", None) is None:
            self._search_sims = self.torch.zeros(self.G, dtype=self.torch.int32, device=self.device)
        self._chk(self.L.azk_get_search_sims(self.h, _p(self._search_sims), _stream()))
        return self._search_sims

    def kld_rate(self):
        """float64 CUDA tensor [G]: the rate of each game's last judged checkpoint (azk_get_kld_rate; valid until the next call)."""
        if self.kld_stop is None:
            raise AzkError("kld_rate: no adaptive search budget is set (set_kld_stop)")
        if getattr(self, "_kld_rate", None) is None:
            self._kld_rate = self.torch.zeros(self.G, dtype=self.torch.float64, device=self.device)
        self._chk(self.L.azk_get_kld_rate(self.h, _p(self._kld_rate), _stream()))
        return self._kld_rate

    def kld_stats(self):
        """The four counters since set_kld_stop (azk_get_kld_stats): checkpoints judged, searches ended early, simulations those searches
        left unrun, searches that ran their allowance."""
        if self.kld_stop is None:
            raise AzkError("kld_stats: no adaptive search budget is set (set_kld_stop)")
        out = np.zeros(4, np.int64)
        self._chk(self.L.azk_get_kld_stats(self.h, _np(out), _stream()))
        return dict(judged=int(out[0]), ended_early=int(out[1]), sims_unrun=int(out[2]), ran_allowance=int(out[3]))

    def begin_search_budget(self, noise, n_sims, per_launch=8, move_index=None):
        """begin_search + a simulation budget: afterwards every step lets a game run on inside the launch while its simulations
        need no evaluator (terminal leaves, eval-cache hits); step until unfinished() == 0, then step_expand_backup once.
        With a playout cap set, move_index (the coin's move key: the noise row's move_index) is required."""
        if noise is not None:
            assert noise.dtype == self.torch.float64 and noise.is_cuda and noise.is_contiguous()
            assert tuple(noise.shape) == (self.G, self.action_dim)
        assert n_sims <= self.max_sims
        self._noise = noise
        if self.playout_cap is not None:
            if move_index is None:
                raise AzkError("begin_search_budget: an engine with a playout cap needs move_index (the coin's move key)")
            self._chk(self.L.azk_begin_search_capped(self.h, _p(noise), int(n_sims), int(per_launch), int(move_index), _stream()))
            return
        self._chk(self.L.azk_begin_search_budget(self.h, _p(noise), int(n_sims), int(per_launch), _stream()))

    def unfinished(self):
        """Games that still owe simulations of their budget or whose last leaf awaits the evaluator (host sync)."""
        out = C.c_int32(0)
        self._chk(self.L.azk_search_unfinished(self.h, C.byref(out), _stream()))
        return int(out.value)

    def step(self, logits=None, values=None):
        """expand+backup the previous leaves (if logits given) and select the next; no host sync."""
        self._chk(self.L.azk_step(self.h, _p(logits), _p(values), _p(self.leaf_boards), _p(self.n_leaf), _stream()))

    def step_tree(self, logits=None, values=None):
        self._chk(self.L.azk_step_tree(self.h, _p(logits), _p(values), _stream()))

    def leaf_source(self):
        """The engine's pending-leaf arrays for azk_nn_embed_pool_leaves (the leaf count lands in self.n_leaf)."""
        if getattr(self, "_leaf_source", None) is None:
            src = LeafSource()
            self._chk(self.L.azk_leaf_source_of(self.h, _p(self.n_leaf), C.byref(src)))
            self._leaf_source = src
        return self._leaf_source

    def step_gather(self):
        self._chk(self.L.azk_step_gather(self.h, _p(self.leaf_boards), _p(self.n_leaf), _stream()))

    def recycle_finished(self, stats):
        """stats: int64 CUDA tensor [8] accumulating (games, plies, wins0, wins1, draws)."""
        assert stats.dtype == self.torch.int64 and stats.is_cuda and stats.numel() >= 8
        self._chk(self.L.azk_recycle_finished(self.h, _p(stats), _stream()))

    def emit_finished(self, replay):
        """Append the (state, pi, z) tuples of every just-finished game to a DeviceReplay; returns int64 [G] first indices (-1: not emitted)."""
        base = self.torch.empty(self.G, dtype=self.torch.int64, device=self.device)
        self._chk(self.L.azk_emit_finished(self.h, _p(replay.states), _p(replay.pis), _p(replay.zs), replay.capacity,
                                           _p(replay.cursor), _p(base), _stream()))
        return base

    def step_select(self):
        self._chk(self.L.azk_step_select(self.h, _p(self.leaf_boards), _p(self.n_leaf), _stream()))

    def step_expand_backup(self, logits, values):
        self._chk(self.L.azk_step_expand_backup(self.h, _p(logits), _p(values), _stream()))

    def evaluate_leaves(self, evaluator, n):
        """Eager stepping's hand-off: the evaluator over the n pending leaf boards (n = the synced n_leaf, > 0), its outputs as
        step / step_expand_backup take them - contiguous float32 logits [n, A] and values [n]."""
        logits, values = evaluator(self.leaf_boards[:n])
        logits = logits.to(self.torch.float32).contiguous()
        values = values.to(self.torch.float32).reshape(-1).contiguous()
        assert logits.shape == (n, self.action_dim) and values.shape[0] == n
        return logits, values

    def placeholder_rows(self):
        """(logits [1, A], values [1]) to pass to a step whose pending leaves all came from the eval cache (nothing reads them), or
        (None, None) on an engine that never has such a step."""
        return self._no_logits, self._no_values

    def search(self, evaluator, n_sims, noise=None):
        """MCTS.mcts for all G games: n_sims simulations each, one in flight per game.
        evaluator(boards[n,F,R,C]) -> (logits[n,A] float32, values[n] or [n,1] float32), on the GPU."""
        assert n_sims <= self.max_sims
        self.begin_search(noise)
        logits = values = None
        for _ in range(n_sims):
            self.step(logits, values)
            n = int(self.n_leaf.item())
            if n > 0:
                logits, values = self.evaluate_leaves(evaluator, n)
            elif self.cache_entries:
                logits, values = self._no_logits, self._no_values      # cache hits still need their expand + backup
            else:
                logits = values = None
        if logits is not None:
            self.step_expand_backup(logits, values)

    def search_budget(self, evaluator, n_sims, noise=None, per_launch=8, move_index=None):
        """The same search as `search` - bit-identical trees - with budget stepping: a game runs on inside a launch while its
        simulations need no evaluator, so n_sims simulations take about (share of simulations that miss the cache) * n_sims
        launches, each with a fuller evaluator batch.  Returns the number of launches.
        With adaptive search budgets set (set_kld_stop, set_lead_stop) the search runs segment by segment: when every game's segment is complete,
        kld_checkpoint judges the games, and the stepping goes on while it released one."""
        self.begin_search_budget(noise, n_sims, per_launch, move_index)
        launches = 0
        segments = 0
        while True:     # one round per segment of the search (adaptive search budgets, set_kld_stop); without the option there is one
            logits = values = None
            segments += 1
            while True:
                self.step(logits, values)
                launches += 1
                n = int(self.n_leaf.item())
                if n > 0:
                    logits, values = self.evaluate_leaves(evaluator, n)
                else:
                    logits, values = (self._no_logits, self._no_values) if self._no_logits is not None else (None, None)
                    if self.unfinished() == 0:
                        break
                assert launches <= 2 * n_sims + 8 * segments, "budget stepping does not terminate"
            if self.cache_entries and self.K == 1:
                self.step_expand_backup(self._no_logits, self._no_values)       # leaves served by the cache in the last launch
            if not self.adaptive or self.kld_checkpoint() == 0:             # every game at a checkpoint: released for another segment, or over
                break
            assert segments <= n_sims, "the checkpoints do not terminate"
        return launches

    # ---- asynchronous self-play (azk_async_*) -----------------------------------------------------
    def async_begin(self, n_sims, per_launch, sample_until, seed, first_global_game, alpha=0.03, dirichlet=True, recycle=True, record_capacity=0,
                    young_launch_us=0, reroot=False):
        """Every game starts its first search; from now on azk_async_step moves each game as soon as its own search is done.
        reroot=True (an engine with tree_reuse 1 | 2): azk_async_begin_reuse - a moved game is parked and re-rooted on the played child by the next drain.
        Returns (stats int64 [16] CUDA, records dict or None) - caller-visible tensors the engine writes (include/azk.h)."""
        torch = self.torch
        self.async_stats = torch.zeros(16, dtype=torch.int64, device=self.device)
        rec = None
        if record_capacity:
            rec = dict(meta=torch.zeros((record_capacity, 4), dtype=torch.int32, device=self.device),
                       q=torch.zeros(record_capacity, dtype=torch.float64, device=self.device),
                       pi=torch.zeros((record_capacity, self.action_dim), dtype=torch.float64, device=self.device))
            if self.playout_cap is not None:                  # the ring's kind column: 1 = the record's search was a full one
                rec["full"] = torch.ones(record_capacity, dtype=torch.uint8, device=self.device)
                self._chk(self.L.azk_async_record_flags(self.h, _p(rec["full"])))
            if self.resign is not None:                       # ... and its resignation column: 1 = the record's move conceded the game
                rec["resigned"] = torch.zeros(record_capacity, dtype=torch.uint8, device=self.device)
                self._chk(self.L.azk_async_resign_flags(self.h, _p(rec["resigned"])))
            if self.surprise_weight is not None:              # ... and its surprise columns: the record's kl and coin
                rec["kl"] = torch.zeros(record_capacity, dtype=torch.float64, device=self.device)
                rec["coin"] = torch.zeros(record_capacity, dtype=torch.float64, device=self.device)
                self._chk(self.L.azk_async_surprise_columns(self.h, _p(rec["kl"]), _p(rec["coin"])))
            if self.adaptive:                                 # ... and its sims column: the new simulations the record's search ran
                rec["sims"] = torch.zeros(record_capacity, dtype=torch.int32, device=self.device)
                self._chk(self.L.azk_async_sims_column(self.h, _p(rec["sims"])))
        self.async_records = rec
        c = AsyncConfig()
        c.n_sims, c.max_sims_per_launch, c.sample_until_move = int(n_sims), int(per_launch), int(min(sample_until, 1 << 30))
        c.dirichlet, c.recycle, c.seed, c.first_global_game, c.alpha = int(bool(dirichlet)), int(bool(recycle)), int(seed), int(first_global_game), float(alpha)
        c.stats_dev, c.record_capacity = self.async_stats.data_ptr(), int(record_capacity)
        c.young_launch_us = int(young_launch_us)      # > 0: another simulation inside a launch only while the launch is younger than this
        if rec is not None:
            c.rec_meta_dev, c.rec_q_dev, c.rec_pi_dev = rec["meta"].data_ptr(), rec["q"].data_ptr(), rec["pi"].data_ptr()
        self._chk((self.L.azk_async_begin_reuse if reroot else self.L.azk_async_begin)(self.h, C.byref(c), _stream()))
        return self.async_stats, rec

    def async_step(self, logits, values, phases=3):
        self._chk(self.L.azk_async_step(self.h, _p(logits), _p(values), int(phases), _stream()))

    def async_set_budget(self, n_sims, per_launch):
        self._chk(self.L.azk_async_set_budget(self.h, int(n_sims), int(per_launch), _stream()))

    def async_drain(self, replay=None):
        if replay is None:
            self._chk(self.L.azk_async_drain(self.h, None, None, None, 0, None, _stream()))
        else:
            self._chk(self.L.azk_async_drain(self.h, _p(replay.states), _p(replay.pis), _p(replay.zs), replay.capacity, _p(replay.cursor), _stream()))

    # ---- vanilla mode (model=None) ----------------------------------------------------------------
    def vanilla_set_rng(self, states, first=0):
        """states: uint32 [count, 625] = MT19937 key + position per game (np.random.get_state()[1:3])."""
        st = np.ascontiguousarray(states, np.uint32).reshape(-1, 625)
        self._chk(self.L.azk_vanilla_set_rng(self.h, first, len(st), _np(st), _stream()))

    def vanilla_get_rng(self, first=0, count=None):
        count = self.G - first if count is None else count
        st = np.empty((count, 625), np.uint32)
        self._chk(self.L.azk_vanilla_get_rng(self.h, first, count, _np(st), _stream()))
        return st

    def vanilla_search(self, n_sims, chunk=None):
        """MCTS.mcts(None, ...) for all G games: begin a search and run n_sims whole simulations (UCB1 walk, expansion,
        random rollout, backup) on the device; `chunk` bounds the simulations per launch."""
        assert n_sims <= self.max_sims
        self.begin_search(None)
        chunk = n_sims if not chunk else int(chunk)
        done = 0
        while done < n_sims:
            k = min(chunk, n_sims - done)
            self._chk(self.L.azk_vanilla_search(self.h, k, _stream()))
            done += k

    def root_stats(self):
        self._chk(self.L.azk_root_stats(self.h, _p(self.pi), _p(self.q), _p(self.root_visit), _stream()))
        return self.pi, self.q, self.root_visit

    def advance(self, uniforms=None, sample_until_move=0, move_index=None):
        """With resignation or surprise weighting set, move_index (the slots' move counter: the noise row's move_index) is required."""
        if uniforms is not None:
            assert uniforms.dtype == self.torch.float64 and uniforms.is_cuda and uniforms.numel() == self.G
        if self.surprise_weight is not None and move_index is not None:
            self._chk(self.L.azk_advance_keyed(self.h, _p(uniforms), int(sample_until_move), int(move_index), _p(self.chosen), _p(self.winner),
                                               _p(self.done), _stream()))
            return self.chosen, self.winner, self.done
        if self.resign is not None and move_index is not None:
            self._chk(self.L.azk_advance_resign(self.h, _p(uniforms), int(sample_until_move), int(move_index), _p(self.chosen), _p(self.winner),
                                                _p(self.done), _stream()))
            return self.chosen, self.winner, self.done
        self._chk(self.L.azk_advance(self.h, _p(uniforms), int(sample_until_move), _p(self.chosen), _p(self.winner),
                                     _p(self.done), _stream()))
        return self.chosen, self.winner, self.done

    def gen_noise(self, seed, first_global_game, move_index, alpha=0.03, want_noise=True, want_uniforms=True):
        torch = self.torch
        noise = torch.empty((self.G, self.action_dim), dtype=torch.float64, device=self.device) if want_noise else None
        uni = torch.empty(self.G, dtype=torch.float64, device=self.device) if want_uniforms else None
        self._chk(self.L.azk_gen_noise(self.h, int(seed), int(first_global_game), int(move_index), float(alpha),
                                       _p(noise), _p(uni), _stream()))
        return noise, uni

    def set_root_noise(self, mode, alpha):
        """OPT-IN root noise on the legal moves (azk_set_root_noise): from now on a search's Dirichlet row is drawn over the
        actions that are legal in the position the search starts from - the root's children - and is 0 elsewhere.  mode "legal": Gamma(alpha)
        per legal action (gen_noise's row restricted to them and renormalised); "total": Gamma(alpha / n) for n legal actions, so the row's total
        concentration is alpha whatever n is (KataGo: 10.83).  Lock-step drivers make the rows with gen_root_noise where they called gen_noise;
        the asynchronous movers make them themselves (alpha takes the place of async_begin's).  Not with a Gumbel root; before async_begin and
        outside a search.  clear_root_noise switches it off."""
        modes = {"legal": 1, "total": 2}
        if mode not in modes:
            raise AzkError(f"set_root_noise: mode must be 'legal' or 'total', not {mode!r}")
        self._chk(self.L.azk_set_root_noise(self.h, modes[mode], float(alpha), _stream()))
        self.root_noise = (mode, float(alpha))

    def clear_root_noise(self):
        """Root noise on the legal moves off (azk_clear_root_noise): the engine launches what it launched before."""
        self._chk(self.L.azk_clear_root_noise(self.h))
        self.root_noise = None

    def gen_root_noise(self, seed, first_global_game, move_index, want_noise=True, want_uniforms=True):
        """gen_noise's (rows, uniforms) with the rows drawn over each game's legal moves, from the engine's positions as they stand
        (azk_gen_root_noise): call it after open_pending / advance and before begin_search*.  The uniforms are gen_noise's bit for bit."""
        if self.root_noise is None:
            raise AzkError("gen_root_noise: no root noise is set (set_root_noise)")
        torch = self.torch
        noise = torch.empty((self.G, self.action_dim), dtype=torch.float64, device=self.device) if want_noise else None
        uni = torch.empty(self.G, dtype=torch.float64, device=self.device) if want_uniforms else None
        self._chk(self.L.azk_gen_root_noise(self.h, int(seed) & ((1 << 64) - 1), int(first_global_game), int(move_index), _p(noise), _p(uni), _stream()))
        return noise, uni

    def root_noise_rows(self):
        """float64 CUDA tensor [G, A]: the row each game's current search reads (azk_get_root_noise; an asynchronous engine: the row of the slot's
        move counter)."""
        if self.root_noise is None:
            raise AzkError("root_noise_rows: no root noise is set (set_root_noise)")
        rows = self.torch.empty((self.G, self.action_dim), dtype=self.torch.float64, device=self.device)
        self._chk(self.L.azk_get_root_noise(self.h, _p(rows), _stream()))
        return rows

    # ---- inspection -----------------------------------------------------------------------------
    def root_children(self, game):
        cap = self.rows * self.cols
        cells = np.empty(cap, np.int32); visits = np.empty(cap, np.int32)
        values = np.empty(cap, np.float64); priors = np.empty(cap, np.float64)
        n = self._chk(self.L.azk_root_children(self.h, int(game), cap, _np(cells), _np(visits), _np(values), _np(priors), _stream()))
        return dict(cell=cells[:n].copy(), visit=visits[:n].astype(np.int64), value=values[:n].copy(), prior=priors[:n].copy())

    def export_tree(self, game, cap=None, quotient=False):
        """The game's tree, DFS pre-order.  quotient=True adds the engine's quotient column (value / visit where visit > 0, bit for bit;
        unspecified where visit == 0)."""
        cap = cap or (1 + (2 if self.tree_reuse == 1 else 1) * self.max_sims * self.rows * self.cols)   # (a carry engine's default arena is twice the size)
        depth = np.empty(cap, np.int32); cell = np.empty(cap, np.int32); visit = np.empty(cap, np.int32)
        value = np.empty(cap, np.float64); prior = np.empty(cap, np.float64)
        if quotient:
            quot = np.empty(cap, np.float64)
            n = self._chk(self.L.azk_export_tree_quotients(self.h, int(game), cap, _np(depth), _np(cell), _np(visit), _np(value), _np(prior),
                                                           _np(quot), _stream()))
            n = min(n, cap)
            return dict(depth=depth[:n], cell=cell[:n], visit=visit[:n].astype(np.int64), value=value[:n], prior=prior[:n], quotient=quot[:n])
        n = self._chk(self.L.azk_export_tree(self.h, int(game), cap, _np(depth), _np(cell), _np(visit), _np(value), _np(prior), _stream()))
        n = min(n, cap)
        return dict(depth=depth[:n], cell=cell[:n], visit=visit[:n].astype(np.int64), value=value[:n], prior=prior[:n])

    def fill_quotients(self, byte):
        """Tests only: every byte of the quotient column becomes `byte` (0: zeros, 255: NaNs).  For engines whose trees are fresh roots."""
        self._chk(self.L.azk_debug_fill_quotients(self.h, int(byte), _stream()))

    def counters(self):
        c = Counters()
        self._chk(self.L.azk_get_counters(self.h, C.byref(c), _stream()))
        return c.as_dict()

    def reset_counters(self):
        self._chk(self.L.azk_reset_counters(self.h, _stream()))

    def clear_cache(self):
        """MCTS.cache.clear() - call when the evaluator's weights change."""
        self._chk(self.L.azk_clear_cache(self.h, _stream()))

    def check_error(self):
        rc = self.L.azk_check_device_error(self.h, _stream())
        if rc != 0:
            raise AzkError(f"device error {rc}: {self.L.azk_last_error(self.h).decode()}")


# ---- stateless board-rule kernels (Game statics) over float32 boards [n, F, R, C] on the GPU ------------
def _geom(game, size):
    gid = GAME_ID[game]
    if isinstance(size, (tuple, list)):          # (rows, cols) or one side, as Engine takes it
        return gid, int(size[0]), int(size[1])
    s = int(size or 0)
    return gid, s, s


def _rules_chk(rc):
    if rc != 0:
        raise AzkError(f"libazk rules error {rc}: {lib().azk_last_error(None).decode()}")


def rules_legal_moves(game, boards, size=None):
    """boards: float32 CUDA tensor [n,F,R,C] -> (moves int16 [n, R*C] in the reference's list order, counts int32 [n])."""
    torch = _torch()
    assert boards.is_cuda and boards.dtype == torch.float32 and boards.is_contiguous()
    n, rc = boards.shape[0], boards.shape[2] * boards.shape[3]
    moves = torch.full((n, rc), -1, dtype=torch.int16, device=boards.device)
    counts = torch.zeros(n, dtype=torch.int32, device=boards.device)
    _rules_chk(lib().azk_rules_legal_moves(*_geom(game, size), _p(boards), n, _p(moves), _p(counts), _stream()))
    return moves, counts


def rules_legal_mask(game, boards, action_dim, size=None):
    torch = _torch()
    assert boards.is_cuda and boards.dtype == torch.float32 and boards.is_contiguous()
    n = boards.shape[0]
    mask = torch.zeros((n, action_dim), dtype=torch.uint8, device=boards.device)
    _rules_chk(lib().azk_rules_legal_mask(*_geom(game, size), _p(boards), n, _p(mask), _stream()))
    return mask


def rules_apply_move(game, boards, players, cells, size=None):
    """in-place make_move on each board; returns next player int32 [n]."""
    torch = _torch()
    assert boards.is_cuda and boards.dtype == torch.float32 and boards.is_contiguous()
    n = boards.shape[0]
    players = players.to(torch.int32).contiguous(); cells = cells.to(torch.int32).contiguous()
    nxt = torch.zeros(n, dtype=torch.int32, device=boards.device)
    _rules_chk(lib().azk_rules_apply_move(*_geom(game, size), _p(boards), n, _p(players), _p(cells), _p(nxt), _stream()))
    return nxt


def rules_undo_move(game, boards, current_players, cells, size=None):
    torch = _torch()
    assert boards.is_cuda and boards.dtype == torch.float32 and boards.is_contiguous()
    n = boards.shape[0]
    cp = current_players.to(torch.int32).contiguous(); cells = cells.to(torch.int32).contiguous()
    _rules_chk(lib().azk_rules_undo_move(*_geom(game, size), _p(boards), n, _p(cp), _p(cells), _stream()))


def rules_check_winner(game, boards, players, cells, size=None):
    torch = _torch()
    assert boards.is_cuda and boards.dtype == torch.float32 and boards.is_contiguous()
    n = boards.shape[0]
    players = players.to(torch.int32).contiguous(); cells = cells.to(torch.int32).contiguous()
    out = torch.zeros(n, dtype=torch.int32, device=boards.device)
    _rules_chk(lib().azk_rules_check_winner(*_geom(game, size), _p(boards), n, _p(players), _p(cells), _p(out), _stream()))
    return out


def rules_canonical(game, boards, players, size=None):
    torch = _torch()
    assert boards.is_cuda and boards.dtype == torch.float32 and boards.is_contiguous()
    players = players.to(torch.int32).contiguous()
    out = torch.empty_like(boards)
    _rules_chk(lib().azk_rules_canonical(*_geom(game, size), _p(boards), boards.shape[0], _p(players), _p(out), _stream()))
    return out


def softmax_rows(logits):
    torch = _torch()
    logits = logits.to(torch.float32).contiguous()
    out = torch.empty_like(logits)
    _rules_chk(lib().azk_softmax_rows(_p(logits), logits.shape[0], logits.shape[1], _p(out), _stream()))
    return out


def nn_patch_embed(boards, wt, cpos, ln_w, ln_b, rows, cols, ksize, embed_dim, want_x=True, want_xhat=False, eps=1e-5,
                   x_out=None, xhat_out=None):
    """Token embedding on the matrix cores (azk_nn_patch_embed).  boards [n,C,R,Cc] bf16|f32 CUDA;
    wt [D,kp] bf16; cpos [T,D] f32.  Returns (x, xhat) bf16 [n,T,D] (None where not requested).
    x_out / xhat_out: buffers to write into (contiguous bf16 [n,T,D]) where that output is requested."""
    torch = _torch()
    assert boards.is_cuda and boards.is_contiguous() and boards.dtype in (torch.bfloat16, torch.float32)
    n, C = boards.shape[0], boards.shape[1]
    T = rows * cols + 1

    def out(want, buf):
        if not want:
            return None
        if buf is None:
            return torch.empty((n, T, embed_dim), dtype=torch.bfloat16, device=boards.device)
        assert buf.shape == (n, T, embed_dim) and buf.dtype == torch.bfloat16 and buf.is_contiguous()
        return buf
    x, xh = out(want_x, x_out), out(want_xhat, xhat_out)
    rc = lib().azk_nn_patch_embed(_p(boards), 1 if boards.dtype == torch.float32 else 0, _p(wt), _p(cpos), _p(ln_w), _p(ln_b),
                                  _p(x), _p(xh), n, C, rows, cols, ksize, wt.shape[1], embed_dim, float(eps), _stream())
    _ok(rc, "azk_nn_patch_embed")
    return x, xh


def nn_cls_attention(xhat, m, c, num_heads):
    """z[b,h,:] = sum_t softmax_t(xhat[b,t,:] . m[.,h,:] + c[.,h]) * xhat[b,t,:]  (azk_nn_cls_attention).
    xhat bf16 [n,T,D]; m f32 [H,D] (shared) or [n,H,D]; c f32 [H] or [n,H].  Returns z bf16 [n,H,D]."""
    torch = _torch()
    assert xhat.is_cuda and xhat.dtype == torch.bfloat16 and xhat.is_contiguous()
    n, T, D = xhat.shape
    per_board = 1 if m.dim() == 3 else 0
    m = m.to(torch.float32).contiguous(); c = c.to(torch.float32).contiguous()
    z = torch.empty((n, num_heads, D), dtype=torch.bfloat16, device=xhat.device)
    rc = lib().azk_nn_cls_attention(_p(xhat), _p(m), _p(c), per_board, _p(z), n, T, D, num_heads, _stream())
    _ok(rc, "azk_nn_cls_attention")
    return z


def nn_embed_scores_pool(boards, wt_ext, cpos, score_cpos, score_msum, c, rows, cols, ksize, embed_dim, num_heads, eps=1e-5,
                         count=None, timers=None):
    """Depth-1 folded cls attention in two launches: azk_nn_patch_embed_scores (normalised tokens + per-token head scores,
    the scores as 16 extra MFMA output columns: wt_ext [D+16, kp]) then azk_nn_cls_pool (softmax + weighted token sum).
    Returns z bf16 [n, H, D]."""
    if timers is not None:
        timers[0].start()
    xh, sc = nn_patch_embed_scores(boards, wt_ext, cpos, score_cpos, score_msum, rows, cols, ksize, embed_dim, num_heads, eps=eps,
                                   count=count)
    if timers is not None:
        timers[0].stop()
        timers[1].start()
    z = nn_cls_pool(xh, sc, c, num_heads, count=count)
    if timers is not None:
        timers[1].stop()
    return z


def nn_patch_embed_scores(boards, wt_ext, cpos, score_cpos, score_msum, rows, cols, ksize, embed_dim, num_heads, eps=1e-5,
                          count=None, xhat=None, scores=None):
    """k_embed's score variant (azk_nn_patch_embed_scores): the normalised tokens without the LayerNorm affine, and per token the
    folded head scores rstd (x . m'_h - mean msum[h]), the x . m'_h as 16 extra MFMA output columns (wt_ext [D+16, kp] bf16,
    score_cpos [T, 16] f32 their per-token additive term, score_msum [16] f32).  Returns (xhat bf16 [n, T, D], scores f32
    [n, H, Tp]), Tp = T rounded up to 16; with a device-side count the rows past it are not written.  xhat / scores: buffers to
    write into (contiguous, of those shapes)."""
    torch = _torch()
    assert boards.is_cuda and boards.is_contiguous() and boards.dtype in (torch.bfloat16, torch.float32)
    assert wt_ext.dtype == torch.bfloat16 and wt_ext.is_contiguous() and wt_ext.shape[0] == embed_dim + 16
    n, C = boards.shape[0], boards.shape[1]
    T = rows * cols + 1
    Tp = (T + 15) // 16 * 16
    assert cpos.numel() == T * embed_dim and score_cpos.numel() == T * 16 and score_msum.numel() == 16
    xh = torch.empty((n, T, embed_dim), dtype=torch.bfloat16, device=boards.device) if xhat is None else xhat
    sc = torch.empty((n, num_heads, Tp), dtype=torch.float32, device=boards.device) if scores is None else scores
    assert xh.shape == (n, T, embed_dim) and xh.dtype == torch.bfloat16 and xh.is_contiguous()
    assert sc.shape == (n, num_heads, Tp) and sc.dtype == torch.float32 and sc.is_contiguous()
    rc = lib().azk_nn_patch_embed_scores(_p(boards), 1 if boards.dtype == torch.float32 else 0, _p(wt_ext), _p(cpos), None, None,
                                         _p(xh), _p(score_cpos), _p(score_msum), _p(sc), num_heads, n, C, rows, cols, ksize,
                                         wt_ext.shape[1], embed_dim, float(eps), _p(count), _stream())
    _ok(rc, "azk_nn_patch_embed_scores")
    return xh, sc


def nn_cls_pool(xhat, scores, c, num_heads, count=None, z=None):
    """k_cls_pool (azk_nn_cls_pool): z[b, h, :] = sum_t softmax_t(scores[b, h, :T] + c[h])[t] xhat[b, t, :].  xhat bf16 [n, T, D];
    scores f32 [n, H, Tp] (Tp = T rounded up to 16; the entries from T on are not read); c f32 [H].  Returns z bf16 [n, H, D];
    with a device-side count the boards past it are not written.  z: a buffer to write into."""
    torch = _torch()
    assert xhat.is_cuda and xhat.dtype == torch.bfloat16 and xhat.is_contiguous()
    n, T, D = xhat.shape
    Tp = (T + 15) // 16 * 16
    assert scores.dtype == torch.float32 and scores.is_contiguous() and scores.shape == (n, num_heads, Tp)
    assert c.dtype == torch.float32 and c.is_contiguous() and c.numel() == num_heads
    # with a device-side count the rows past it are never written; every later op is row-wise, so they cannot leak
    if z is None:
        z = torch.empty((n, num_heads, D), dtype=torch.bfloat16, device=xhat.device)
    assert z.shape == (n, num_heads, D) and z.dtype == torch.bfloat16 and z.is_contiguous()
    rc = lib().azk_nn_cls_pool(_p(xhat), _p(scores), _p(c), _p(z), n, T, D, num_heads, _p(count), _stream())
    _ok(rc, "azk_nn_cls_pool")
    return z


def nn_embed_pool(boards, wt_ext, cpos_frag, score_frag, score_msum, score_ref, rows, cols, ksize, embed_dim, num_heads,
                  eps=1e-5, count=None, timers=None):
    """Depth-1 folded cls attention in ONE launch (azk_nn_embed_pool): boards -> z bf16 [n, H, D]; tokens never reach HBM.
    cpos_frag / score_frag: per-token constants padded to whole 16-token tiles, in accumulator order (include/azk.h);
    score_ref: [16] static softmax reference per head or None (running maximum)."""
    torch = _torch()
    assert boards.is_cuda and boards.is_contiguous() and boards.dtype in (torch.bfloat16, torch.float32)
    Tp = (rows * cols + 1 + 15) // 16 * 16
    assert cpos_frag.numel() == Tp * embed_dim and score_frag.numel() == Tp * 16 and cpos_frag.is_contiguous() and score_frag.is_contiguous()
    n, C = boards.shape[0], boards.shape[1]
    z = torch.empty((n, num_heads, embed_dim), dtype=torch.bfloat16, device=boards.device)
    fn = lib().azk_nn_embed_pool
    args = (_p(boards), 1 if boards.dtype == torch.float32 else 0, _p(wt_ext), _p(cpos_frag), _p(score_frag), _p(score_msum),
            _p(score_ref), _p(z), num_heads, n, C, rows, cols, ksize, wt_ext.shape[1], embed_dim, float(eps), _p(count), _stream())
    if timers is not None:          # everything is marshalled already: the events bracket the launch alone
        timers[0].start()
    rc = fn(*args)
    if timers is not None:
        timers[0].stop()
    _ok(rc, "azk_nn_embed_pool")
    return z


def nn_embed_pool_leaves(src, wt_ext, cpos_frag, score_frag, score_msum, score_ref, ksize, embed_dim, num_heads, eps=1e-5,
                         timers=None):
    """nn_embed_pool over an engine's pending leaves (LeafSource) instead of a compacted board batch: z bf16 [G, H, D],
    rows [0, n_leaf) valid; also writes the engine's leaf slots and the leaf count (no azk_step_gather needed)."""
    torch = _torch()
    z = torch.empty((src.n_games, num_heads, embed_dim), dtype=torch.bfloat16, device=wt_ext.device)
    fn = lib().azk_nn_embed_pool_leaves
    args = (C.byref(src), _p(wt_ext), _p(cpos_frag), _p(score_frag), _p(score_msum), _p(score_ref), _p(z), num_heads, ksize,
            wt_ext.shape[1], embed_dim, float(eps), _stream())
    if timers is not None:
        timers[0].start()
    rc = fn(*args)
    if timers is not None:
        timers[0].stop()
    _ok(rc, "azk_nn_embed_pool_leaves")
    return z


class _Tables:
    """Base of the three table holders: self.t (dict of device tensors, kept alive) and self.c (their ctypes descriptor)."""
    work_stats = None

    def enable_work_stats(self):
        """Device counters [boards evaluated, 16-token tiles evaluated] (int64 [2]), bumped by every launch from now on."""
        if self.work_stats is None:
            self.work_stats = _torch().zeros(2, dtype=_torch().int64, device=self.t["score_tok"].device)
            self.c.work_stats = self.work_stats.data_ptr()
        return self.work_stats


def _embed(symbol, dtype, width, tables, sched, timers, boards=None, rows=0, cols=0, count=None, src=None, exact=False):
    """The call every compacting embedding kernel shares (azk_nn_embed_pool_compact, azk_nn_embed_fold, azk_nnx_embed_fold,
    azk_nnx_embed_pool and their _leaves forms): boards [n, C, R, Cc] bf16 / f32, or an engine's pending leaves (src: LeafSource),
    -> rows [n or slots, H, width] of `dtype`.  exact: the tables must be the float32-accurate ones."""
    torch = _torch()
    assert not exact or tables.exact
    if src is None:
        assert boards.is_cuda and boards.is_contiguous() and boards.dtype in (torch.bfloat16, torch.float32)
        assert rows * cols + 1 == tables.tokens and sched.dtype == torch.int32 and sched.numel() >= 2
        n, Cc = boards.shape[0], boards.shape[1]
        out = torch.empty((n, tables.num_heads, width), dtype=getattr(torch, dtype), device=boards.device)
        args = (_p(boards), 1 if boards.dtype == torch.float32 else 0, C.byref(tables.c), _p(out), n, Cc, rows, cols, _p(count), _p(sched), _stream())
    else:
        symbol += "_leaves"
        assert src.rows * src.cols + 1 == tables.tokens and sched.dtype == torch.int32 and sched.numel() >= 2
        out = torch.empty((src.n_games, tables.num_heads, width), dtype=getattr(torch, dtype), device=sched.device)
        args = (C.byref(src), C.byref(tables.c), _p(out), _p(sched), _stream())
    fn = getattr(lib(), symbol)
    if timers is not None:          # everything is marshalled already: the events bracket the launch alone
        timers[0].start()
    rc = fn(*args)
    if timers is not None:
        timers[0].stop()
    _ok(rc, symbol)
    return out


class EmbedPoolTables(_Tables):
    """The tables of azk_nn_embed_pool_compact, kept alive together with their ctypes descriptor.
    t: dict of CUDA tensors (wt_ext bf16 [D+16, kp]; cpos_tok f32 [T+1, D]; score_tok, wconst_tok f32 [T+1, 16]; xnconst_tok bf16
    [T+1, D]; z_all f32 [4, 8, 64, 4]; l_all, score_msum, score_ref f32 [16])."""

    def __init__(self, t, num_heads, ksize, embed_dim, eps=1e-5):
        torch = _torch()
        self.t = {k: v.contiguous() for k, v in t.items()}
        T1 = self.t["cpos_tok"].shape[0]
        for k, (shape, dt) in dict(cpos_tok=((T1, embed_dim), torch.float32), score_tok=((T1, 16), torch.float32),
                                   wconst_tok=((T1, 16), torch.float32), xnconst_tok=((T1, embed_dim), torch.bfloat16),
                                   z_all=((4, 8, 64, 4), torch.float32), l_all=((16,), torch.float32), score_msum=((16,), torch.float32),
                                   score_ref=((16,), torch.float32)).items():
            assert tuple(self.t[k].shape) == shape and self.t[k].dtype == dt and self.t[k].is_cuda, k
        assert self.t["wt_ext"].dtype == torch.bfloat16 and self.t["wt_ext"].shape[0] == embed_dim + 16 and embed_dim == 512
        # MFMA fragment order [33 column tiles][kp/32][64 lanes][8] (include/azk.h)
        w = self.t["wt_ext"]
        kp = w.shape[1]
        ct, l = torch.arange(33, device=w.device)[:, None], torch.arange(64, device=w.device)[None, :]
        col = torch.where(ct < 32, 128 * (ct >> 3) + 8 * (l & 15) + (ct & 7), 512 + (l & 15))           # [33, 64]
        kidx = (32 * torch.arange(kp // 32, device=w.device)[:, None, None] + 8 * (l[0] >> 4)[None, :, None]
                + torch.arange(8, device=w.device)[None, None, :])                                      # [KS, 64, 8]
        self.t["wt_frag"] = w[col[:, None, :, None], kidx[None]].contiguous()                           # [33, KS, 64, 8]
        self.tokens, self.num_heads, self.embed_dim = T1 - 1, num_heads, embed_dim
        self.c = EmbedPoolConsts(*[self.t[k].data_ptr() for k in ("wt_frag", "cpos_tok", "score_tok", "wconst_tok", "xnconst_tok", "z_all",
                                                                 "l_all", "score_msum", "score_ref")],
                                 num_heads, ksize, self.t["wt_ext"].shape[1], embed_dim, float(eps), None)


def new_sched(device):
    """The work-queue words of the compacting kernel: int32 [2], zero; one buffer per stream that may run it concurrently."""
    return _torch().zeros(2, dtype=_torch().int32, device=device)


def nn_embed_pool_compact(boards, tables, rows, cols, sched, count=None, timers=None):
    """azk_nn_embed_pool_compact: boards [n, C, R, Cc] bf16 / f32 -> z bf16 [n, H, D], evaluating only the tokens a stone can reach."""
    return _embed("azk_nn_embed_pool_compact", "bfloat16", tables.embed_dim, tables, sched, timers, boards, rows, cols, count)


def nn_embed_pool_compact_leaves(src, tables, sched, timers=None):
    """azk_nn_embed_pool_compact over an engine's pending leaves (LeafSource): z bf16 [G, H, D], rows [0, n_leaf) valid."""
    return _embed("azk_nn_embed_pool_compact", "bfloat16", tables.embed_dim, tables, sched, timers, src=src)


class EmbedFoldTables(_Tables):
    """Tables of azk_nn_embed_fold and the weight of the batched GEMM that follows it, from PolicyValueNet.fold_u's float64 operands
    (r: G [64, 64], ext [64, 16], U2 [T, 64], nt [T], sct [T, H], Dtab [T, 512], M [512, 64], rstdc [T], ref [H], wc [T, H], uall [512],
    lall [H]); kept alive with the ctypes descriptor.  `weight`: H blocks of [64][EMBED_FOLD_ROW] in azk_nn_tail_gemm's packing."""

    def __init__(self, r, num_heads, ksize, embed_dim, device, eps=1e-5, exact=False):
        """exact: the tables of azk_nnx_embed_fold (float32 rows, 1 / L in one slot) and the weight in azk_nnx_gemm_h's (hi, lo) planes."""
        torch = _torch()
        self.exact = bool(exact)
        assert embed_dim == 512 and embed_dim // num_heads == 64
        H, D = num_heads, embed_dim
        dev = torch.device(device)
        T = r["U2"].shape[0]
        assert T + 3 <= 256 and r["G"].shape == (64, 64)
        # power-of-two scales that put the largest entry's hi term near 2^10: hi and lo both normal fp16 for entries down to ~1e-7 of it
        sc = lambda t: 2.0 ** (10 - math.ceil(math.log2(max(float(t.abs().max()), 1e-30))))
        gs, es = sc(r["G"]), sc(r["ext"])

        def frags(mat, scale, ncol):                    # mat [64 k, 16 ncol columns] -> [2 (hi, lo)][ncol][2 k-steps][64 lanes][8]
            hi, lo = split_fp16(mat.to(dev), scale)
            l = torch.arange(64, device=dev)
            col = 16 * torch.arange(ncol, device=dev)[:, None] + (l & 15)[None, :]                                      # [ncol, 64]
            kidx = 32 * torch.arange(2, device=dev)[:, None, None] + 8 * (l >> 4)[None, :, None] + torch.arange(8, device=dev)[None, None, :]   # [2, 64, 8]
            pick = lambda m_: m_[kidx[None], col[:, None, :, None]]                                                     # [ncol, 2, 64, 8]
            return torch.stack([pick(hi), pick(lo)]).contiguous()
        t = {}
        t["g_frag"] = frags(r["G"], gs, 4)              # element [term][q][s][l][i] = G[32 s + 8 (l>>4) + i][16 q + (l&15)] (G is symmetric)
        t["e_frag"] = frags(r["ext"], es, 1)
        f32 = lambda x: x.to(dev, torch.float32).contiguous()
        u2 = torch.zeros(T + 1, 64, dtype=torch.float64, device=dev)
        u2[:T] = r["U2"].to(dev)
        t["u2_tok"] = f32(u2)
        st = torch.zeros(T + 1, 16, dtype=torch.float64, device=dev)
        st[:T, :H], st[:T, 15] = r["sct"].to(dev), r["nt"].to(dev)
        st[T, :H], st[T, 15] = -1e30, float(D)
        t["score_tok"] = f32(st)
        wct = torch.zeros(T + 1, 16, dtype=torch.float64, device=dev)
        wct[:T, :H], wct[:T, 15] = r["wc"].to(dev), r["rstdc"].to(dev)
        wct[T, 15] = 1.0
        t["wconst_tok"] = f32(wct)
        la = torch.zeros(16, dtype=torch.float64, device=dev)
        la[:H] = r["lall"].to(dev)
        t["l_all"] = f32(la)
        ref = torch.full((16,), 1e30, dtype=torch.float64, device=dev)
        ref[:H] = r["ref"].to(dev)
        t["score_ref"] = f32(ref)
        t["inv_scales"] = torch.tensor([1.0 / gs, 1.0 / es], dtype=torch.float32, device=dev)
        self.t = t
        # the GEMM weight: per head [64 outputs][EMBED_FOLD_ROW]: D_t (t < T), U_all as bf16 hi at T and T + 1, its remainder at T + 2,
        # M_h at [256, 320)
        W = torch.zeros(H, 64, EMBED_FOLD_ROW, dtype=torch.float64, device=dev)
        W[:, :, :T] = r["Dtab"].to(dev).view(T, H, 64).permute(1, 2, 0)
        ua = r["uall"].to(dev).view(H, 64)
        ua_hi = ua.to(torch.bfloat16).double()
        if exact:
            W[:, :, T] = ua                                                  # (float32 rows carry 1 / L in one slot, the planes U_all in full)
        else:
            W[:, :, T], W[:, :, T + 1], W[:, :, T + 2] = ua_hi, ua_hi, ua - ua_hi
        W[:, :, 256:320] = r["M"].to(dev).view(H, 64, 64)
        self.weight_f64 = W
        if exact:
            t["weight"] = torch.stack([pack_linear_weight_h(W[h])[0] for h in range(H)]).contiguous()
        else:
            t["weight"] = torch.cat([pack_linear_weight(W[h].float()).reshape(-1) for h in range(H)])  # (in .t: promoted in place with the tables)
        self.weight = t["weight"]
        self.tokens, self.num_heads, self.embed_dim = T, H, D
        self.c = EmbedFoldConsts(*[t[k].data_ptr() for k in ("g_frag", "e_frag", "u2_tok", "score_tok", "wconst_tok", "l_all", "score_ref",
                                                             "inv_scales")], H, ksize, D, float(eps), None)


def nn_embed_fold(boards, tables, rows, cols, sched, count=None, timers=None):
    """azk_nn_embed_fold: boards [n, C, R, Cc] bf16 / f32 -> bf16 [n, H, EMBED_FOLD_ROW] (token weights / L, 1 / L, pooled patch / L)."""
    return _embed("azk_nn_embed_fold", "bfloat16", EMBED_FOLD_ROW, tables, sched, timers, boards, rows, cols, count)


def nn_embed_fold_leaves(src, tables, sched, timers=None):
    """azk_nn_embed_fold over an engine's pending leaves (LeafSource): bf16 [G, H, EMBED_FOLD_ROW], rows [0, n_leaf) valid."""
    return _embed("azk_nn_embed_fold", "bfloat16", EMBED_FOLD_ROW, tables, sched, timers, src=src)


def nnx_embed_fold(boards, tables, rows, cols, sched, count=None, timers=None):
    """azk_nnx_embed_fold: boards [n, C, R, Cc] bf16 / f32 -> float32 [n, H, EMBED_FOLD_ROW] (token weights / L, 1 / L, pooled patch / L)."""
    return _embed("azk_nnx_embed_fold", "float32", EMBED_FOLD_ROW, tables, sched, timers, boards, rows, cols, count, exact=True)


def nnx_embed_fold_leaves(src, tables, sched, timers=None):
    """azk_nnx_embed_fold over an engine's pending leaves (LeafSource): float32 [G, H, EMBED_FOLD_ROW], rows [0, n_leaf) valid."""
    return _embed("azk_nnx_embed_fold", "float32", EMBED_FOLD_ROW, tables, sched, timers, src=src, exact=True)


TAIL_BF16, TAIL_GELU, TAIL_RESID, TAIL_HEADS = 0, 1, 2, 3


def nn_tail_gemm(a, w_packed, n_out, k, epilogue=TAIL_BF16, nbatch=1, a_batch_stride=0, bias=None, out=None, resid=None,
                 a_stats=None, stats_out=None, logits=None, values=None, action_dim=0, count=None, eps=1e-5, col_sums=None, lds=False):
    """One link of the cls-row tail (azk_nn_tail_gemm): a bf16 [m, lda] x packed weights -> out bf16 [m, nbatch * n_out] (or the
    heads' float32 logits / values).  a_stats [m, groups, 2]: A is LayerNorm(a) (affine folded by the caller), its row statistics
    coming from the producer's stats_out."""
    torch = _torch()
    assert a.dtype == torch.bfloat16 and a.stride(-1) == 1 and a.dim() == 2
    d = TailGemm()
    d.a_bf16, d.lda, d.a_batch_stride, d.w_packed = a.data_ptr(), a.stride(0), int(a_batch_stride), w_packed.data_ptr()
    d.m, d.n_out, d.k, d.nbatch = a.shape[0], int(n_out), int(k), int(nbatch)
    d.n_valid = count.data_ptr() if count is not None else None
    d.bias = bias.data_ptr() if bias is not None else None
    d.layernorm_a, d.epilogue, d.ln_eps = (1 if a_stats is not None else 0), int(epilogue), float(eps)
    if a_stats is not None:
        assert a_stats.dtype == torch.float32 and a_stats.dim() == 3 and a_stats.shape[2] == 2 and a_stats.is_contiguous()
        d.a_stats, d.a_stats_groups = a_stats.data_ptr(), a_stats.shape[1]
    if stats_out is not None:
        assert stats_out.dtype == torch.float32 and tuple(stats_out.shape) == (a.shape[0], nbatch * n_out // 64, 2) and stats_out.is_contiguous()
        d.stats_out = stats_out.data_ptr()
    if out is not None:
        assert out.dtype == torch.bfloat16 and out.stride(-1) == 1
        d.out_bf16, d.ldo = out.data_ptr(), out.stride(0)
    if resid is not None:
        d.resid_bf16, d.ldr = resid.data_ptr(), resid.stride(0)
    if logits is not None:
        assert logits.dtype == torch.float32 and values.dtype == torch.float32 and logits.is_contiguous()
        d.logits_out, d.values_out, d.action_dim = logits.data_ptr(), values.data_ptr(), int(action_dim)
    if col_sums is not None:
        assert col_sums.dtype == torch.float32 and col_sums.is_contiguous() and col_sums.numel() >= nbatch * n_out
        d.a_col_sums = col_sums.data_ptr()
    rc = (lib().azk_nn_tail_gemm_lds if lds else lib().azk_nn_tail_gemm)(C.byref(d), _stream())
    if rc != 0:
        raise AzkError(f"azk_nn_tail_gemm{'_lds' if lds else ''} failed ({rc})")


TOK_BF16, TOK_GELU, TOK_RESID, TOK_F32 = 0, 1, 2, 4


def nn_gemm_tok(a, w_packed, n_out, epilogue=TOK_BF16, bias=None, out=None, resid=None, count=None):
    """out[m][n_out] = a[m][k] W^T (+ bias) through an epilogue (azk_nn_gemm_tok, csrc/azk_block.hip).  a: bf16 [m, k] (row stride
    a.stride(0)); w_packed: pack_linear_weight128(W); n_out: the padded output width (a multiple of 128); out: bf16 (float32 for
    TOK_F32) [m, >= n_out], allocated when None; resid: bf16 [m, >= n_out] for TOK_RESID."""
    torch = _torch()
    assert a.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1 and n_out % 128 == 0
    m, k = a.shape
    if out is None:
        out = torch.empty((m, n_out), dtype=torch.float32 if epilogue == TOK_F32 else torch.bfloat16, device=a.device)
    assert out.stride(1) == 1 and out.dtype == (torch.float32 if epilogue == TOK_F32 else torch.bfloat16)
    d = GemmTok()
    d.a_bf16, d.lda, d.w_packed, d.m, d.n_out, d.k = a.data_ptr(), a.stride(0), w_packed.data_ptr(), m, int(n_out), k
    d.n_valid = count.data_ptr() if count is not None else None
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() >= n_out
        d.bias = bias.data_ptr()
    d.epilogue, d.out, d.ldo = int(epilogue), out.data_ptr(), out.stride(0)
    if resid is not None:
        assert resid.dtype == torch.bfloat16 and resid.stride(1) == 1
        d.resid_bf16, d.ldr = resid.data_ptr(), resid.stride(0)
    rc = lib().azk_nn_gemm_tok(C.byref(d), _stream())
    _ok(rc, "azk_nn_gemm_tok")
    return out


def nn_attention_tok(qkv, n_boards, tokens, embed_dim, num_heads, out=None, count=None):
    """softmax(q k^T / sqrt(dh)) v over all tokens of every board (azk_nn_attention_tok).  qkv: bf16 [n_boards * tokens, 3 embed_dim]."""
    torch = _torch()
    assert qkv.dtype == torch.bfloat16 and qkv.is_contiguous() and qkv.shape == (n_boards * tokens, 3 * embed_dim)
    if out is None:
        out = torch.empty((n_boards * tokens, embed_dim), dtype=torch.bfloat16, device=qkv.device)
    assert out.is_contiguous() and out.dtype == torch.bfloat16
    rc = lib().azk_nn_attention_tok(_p(qkv), _p(out), int(n_boards), int(tokens), int(embed_dim), int(num_heads), _p(count), _stream())
    _ok(rc, "azk_nn_attention_tok")
    return out


def nn_heads_finalize(heads, action_dim, logits_out, values_out, count=None):
    """heads bf16 [n, ld] (merged policy/value GEMM) -> logits_out f32 [n, A], values_out f32 [n] = tanh(raw), one launch."""
    torch = _torch()
    assert heads.dtype == torch.bfloat16 and heads.is_contiguous() and logits_out.dtype == torch.float32 and values_out.dtype == torch.float32
    rc = lib().azk_nn_heads_finalize(_p(heads), heads.shape[1], int(action_dim), heads.shape[0], _p(logits_out), _p(values_out),
                                     _p(count), _stream())
    _ok(rc, "azk_nn_heads_finalize")


def nn_layernorm_rows(x, w, b, eps=1e-5, add_bias=None, count=None):
    """LayerNorm over the rows of bf16 x [n, D] -> new bf16 tensor; with add_bias, x becomes x + add_bias in place."""
    torch = _torch()
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and w.dtype == torch.float32 and b.dtype == torch.float32
    y = torch.empty_like(x)
    rc = lib().azk_nn_layernorm_rows(_p(x), _p(w), _p(b), float(eps), _p(y), _p(add_bias), x.shape[0], x.shape[1], _p(count), _stream())
    _ok(rc, "azk_nn_layernorm_rows")
    return y


def mt_state_from_numpy(state=None):
    """np.random.get_state() (or a RandomState's) -> the uint32[625] an engine game takes (key + position)."""
    st = np.random.get_state() if state is None else state
    assert st[0] == "MT19937"
    out = np.empty(625, np.uint32)
    out[:624] = st[1]
    out[624] = st[2]
    return out


def mt_state_to_numpy(words, template=None):
    """uint32[625] read back from the engine -> a tuple for np.random.set_state (Gaussian cache fields from `template`)."""
    t = np.random.get_state() if template is None else template
    return ("MT19937", np.asarray(words[:624], np.uint32), int(words[624]), t[3], t[4])


def nn_ln_heads(x, w_packed, bias, action_dim, logits_out, values_out, eps=1e-5, count=None):
    """Final LayerNorm + merged policy/value head + finalize in one launch: x bf16 [n, D] -> logits f32 [n, A], values f32 [n]."""
    torch = _torch()
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    n, d = x.shape
    rc = lib().azk_nn_ln_heads(_p(x), float(eps), _p(w_packed), _p(bias), n, d, bias.numel(), int(action_dim),
                               _p(logits_out), _p(values_out), _p(count), _stream())
    _ok(rc, "azk_nn_ln_heads")


# ---- fp32-accurate network path (csrc/azk_nnx.hip) ----------------------------------------------------------------------
class EmbedPoolXTables(_Tables):
    """Tables of azk_nnx_embed_pool, kept alive with their ctypes descriptor.  t: dict of CUDA tensors - wt_ext float64 [D+16, kp] (conv
    weight, folded score rows, mean row); cpos_tok, xnconst_tok f32 [T+1, D]; score_tok, wconst_tok f32 [T+1, 16]; z_all f32 [16, D]
    (head-major, converted to accumulator order here); l_all, score_msum, score_ref f32 [16]."""

    WT_SCALE = 4096.0      # weights (|w| < 0.2 here) x 2^12: hi and lo fp16 terms both in the normal range down to |w| ~ 6e-5
    WC_SCALE, XNC_SCALE = 64.0, 16.0     # constant tokens' softmax weights (in (0, 1]) and normalised rows (|x| < 23) as two fp16 terms each

    def __init__(self, t, num_heads, ksize, embed_dim, eps=1e-5):
        torch = _torch()
        assert embed_dim == 512
        dev = t["cpos_tok"].device
        self.t = {k: v.contiguous() for k, v in t.items() if k not in ("wt_ext", "z_all")}      # (z_all is rebuilt below from the split constant terms)
        T1 = self.t["cpos_tok"].shape[0]
        for k, shape in dict(cpos_tok=(T1, embed_dim), xnconst_tok=(T1, embed_dim), score_tok=(T1, 16), wconst_tok=(T1, 16), l_all=(16,),
                             score_msum=(16,), score_ref=(16,)).items():
            assert tuple(self.t[k].shape) == shape and self.t[k].dtype == torch.float32 and self.t[k].is_cuda, k
        w = t["wt_ext"].double()
        assert w.shape[0] == embed_dim + 16 and w.shape[1] % 32 == 0 and float(w.abs().max()) * self.WT_SCALE < 60000.0
        kp = w.shape[1]
        hi, lo = split_fp16(w, self.WT_SCALE)
        ct, l = torch.arange(33, device=dev)[:, None], torch.arange(64, device=dev)[None, :]
        col = torch.where(ct < 32, 64 * (ct >> 2) + 4 * (l & 15) + (ct & 3), 512 + (l & 15))                 # [33, 64]
        kidx = (32 * torch.arange(kp // 32, device=dev)[:, None, None] + 8 * (l[0] >> 4)[None, :, None]
                + torch.arange(8, device=dev)[None, None, :])                                             # [KS, 64, 8]
        fh, fl = hi[col[:, None, :, None], kidx[None]], lo[col[:, None, :, None], kidx[None]]              # [33, KS, 64, 8]
        self.t["wt_frag"] = torch.stack([fh, fl], dim=2).contiguous()                                      # [33, KS, 2, 64, 8]
        # the constant tokens' part of the weighted token sum runs on v_mfma_f32_16x16x32_f16 with both operands as (hi, lo) fp16
        # pairs (all four partial products in two instructions): -wconst * WC_SCALE per (token, head) as one uint32 (hi | lo << 16),
        # xnconst * XNC_SCALE per (token, 4 columns) as 16 bytes (hi0..hi3, lo0..lo3); the accumulators then run in units of
        # POOL_SCALE = WC_SCALE * XNC_SCALE (the kernel scales the stone-touched tokens' weights by it, z_all comes pre-scaled)
        wc, xnc = self.t["wconst_tok"].double(), self.t["xnconst_tok"].double()
        assert float(wc.max()) <= 1.0 + 1e-6 and float(xnc.abs().max()) * self.XNC_SCALE < 60000.0
        wh, wl = split_fp16(-wc, self.WC_SCALE)
        self.t["wconst_h16"] = (wh.view(torch.int16).to(torch.int32) & 0xffff | (wl.view(torch.int16).to(torch.int32) << 16)).contiguous()
        xh, xl = split_fp16(xnc, self.XNC_SCALE)
        self.t["xnconst_h16"] = torch.cat([xh.view(T1, embed_dim // 4, 4), xl.view(T1, embed_dim // 4, 4)], dim=2).contiguous()   # [T+1, 128, 8] fp16
        self.pool_scale = self.WC_SCALE * self.XNC_SCALE
        wc_eff = -(wh.double() + wl.double()) / self.WC_SCALE                # what the kernel subtracts per dirty token ...
        xnc_eff = (xh.double() + xl.double()) / self.XNC_SCALE
        zall = (wc_eff.t() @ xnc_eff) * self.pool_scale                      # ... so the sum over ALL tokens uses the same terms
        # z_all [16 heads, D] -> accumulator order [g][q][lane = 16 l4 + l15][j]: head 4 l4 + j, column 64 g + 4 l15 + q
        za = zall.float().view(4, 4, 8, 16, 4)                                # [l4, j, g, l15, q]
        self.t["z_all"] = za.permute(2, 4, 0, 3, 1).reshape(8, 4, 64, 4).contiguous()
        self.tokens, self.num_heads, self.embed_dim = T1 - 1, num_heads, embed_dim
        self.c = EmbedPoolXConsts(*[self.t[k].data_ptr() for k in ("wt_frag", "cpos_tok", "score_tok", "wconst_tok", "xnconst_h16", "z_all",
                                                                  "l_all", "score_msum", "score_ref")],
                                  num_heads, ksize, kp, embed_dim, float(eps), float(self.WT_SCALE), None,
                                  self.t["wconst_h16"].data_ptr(), float(self.pool_scale))


def nnx_embed_pool(boards, tables, rows, cols, sched, count=None, timers=None):
    """azk_nnx_embed_pool: boards [n, C, R, Cc] bf16 / f32 (values 0 / 1) -> z float32 [n, H, 512]."""
    return _embed("azk_nnx_embed_pool", "float32", tables.embed_dim, tables, sched, timers, boards, rows, cols, count)


def nnx_embed_pool_leaves(src, tables, sched, timers=None):
    """azk_nnx_embed_pool over an engine's pending leaves (LeafSource): z float32 [slots, H, 512], rows [0, n_leaf) valid."""
    return _embed("azk_nnx_embed_pool", "float32", tables.embed_dim, tables, sched, timers, src=src)


def nnx_gemm_h(a, w_packed, n_out, k, epilogue=TAIL_BF16, nbatch=1, a_batch_stride=0, bias=None, col_sums=None, out=None, out_f32=None,
               resid=None, a_stats=None, stats_out=None, logits=None, values=None, action_dim=0, count=None, eps=1e-5, lds=False, overflow=None):
    """One link of the fp32-accurate tail on fp16 (hi, lo) planes (azk_nnx_gemm_h).  a: a float32 tensor [m, lda] (split on the fly)
    or a (hi, lo) pair of fp16 tensors; out: a (hi, lo) pair of fp16 tensors [m, nbatch * n_out] and / or out_f32."""
    torch = _torch()
    d = GemmH()
    if isinstance(a, (tuple, list)):
        ah, al = a
        assert ah.dtype == torch.float16 and al.dtype == torch.float16 and ah.stride(1) == 1 and ah.stride(0) == al.stride(0)
        d.a_hi, d.a_lo, d.lda, m = ah.data_ptr(), al.data_ptr(), ah.stride(0), ah.shape[0]
    else:
        assert a.dtype == torch.float32 and a.stride(1) == 1
        d.a_f32, d.lda, m = a.data_ptr(), a.stride(0), a.shape[0]
    d.a_batch_stride, d.w_packed = int(a_batch_stride), w_packed.data_ptr()
    d.m, d.n_out, d.k, d.nbatch = m, int(n_out), int(k), int(nbatch)
    d.n_valid = count.data_ptr() if count is not None else None
    d.bias = bias.data_ptr() if bias is not None else None
    d.col_sums = col_sums.data_ptr() if col_sums is not None else None
    d.layernorm_a, d.epilogue, d.ln_eps = (1 if a_stats is not None else 0), int(epilogue), float(eps)
    d.a_scale, d.w_scale = GEMM_H_A_SCALE, GEMM_H_W_SCALE
    d.a_stats = a_stats.data_ptr() if a_stats is not None else None
    d.stats_out = stats_out.data_ptr() if stats_out is not None else None
    if out is not None:
        oh, ol = out
        assert oh.dtype == torch.float16 and ol.dtype == torch.float16 and oh.stride(1) == 1 and oh.stride(0) == ol.stride(0)
        d.out_hi, d.out_lo, d.ldo = oh.data_ptr(), ol.data_ptr(), oh.stride(0)
    if out_f32 is not None:
        assert out_f32.dtype == torch.float32 and out_f32.stride(1) == 1 and (out is None or out_f32.stride(0) == out[0].stride(0))
        d.out_f32, d.ldo = out_f32.data_ptr(), out_f32.stride(0)
    if resid is not None:
        assert resid.dtype == torch.float32 and resid.stride(1) == 1
        d.resid_f32, d.ldr = resid.data_ptr(), resid.stride(0)
    if logits is not None:
        d.logits_out, d.values_out, d.action_dim = logits.data_ptr(), values.data_ptr(), int(action_dim)
    if overflow is not None:
        assert overflow.dtype == torch.int32 and overflow.numel() >= 1
        d.overflow_flag = overflow.data_ptr()
    rc = (lib().azk_nnx_gemm_h_lds if lds else lib().azk_nnx_gemm_h)(C.byref(d), _stream())
    if rc != 0:
        raise AzkError(f"azk_nnx_gemm_h{'_lds' if lds else ''} failed ({rc})")
