"""train.py of the reference (train.py:8-123) with its names and signatures, on the batched engine.

    collect_data(Game, model, buffer, iterations, mcts_iter, display=False)   train.py:54-83
    save_data_to_buffer(Game, buffer, data, full=None, elements=None, copies=None, first_ply=0)   train.py:30-49
    rotate_data / flip_data                                                   train.py:8-27
    train(model, batch_size, buffer, train_iterations, lr, device, augment=None)   train.py:85-123

`buffer` is anything with the reference's ReplayBuffer interface (add / sample / size) - the reference's own class or
azk.DeviceReplay.  With a DeviceReplay, collect_data plays all `iterations` games as ONE lock-step batch and the engine
emits the (state, pi, z) tuples on the device (azk_emit_finished); with a host buffer the games still run as one batch and
the tuples are appended through save_data_to_buffer exactly as the reference does it, game by game.
`model`: pvnet.PolicyValueNet (or, for collect_data, any callable tensor[n,F,R,C] -> (logits[n,A], value[n,1])).
"""
import numpy as np


def rotate_data(board, policy, k=0):
    """train.py:8-15: np.rot90 on the board planes and on the policy reshaped to the board."""
    rows, cols = board.shape[-2], board.shape[-1]
    return np.rot90(board, k=k, axes=(1, 2)), np.rot90(policy.reshape(rows, cols), k=k).reshape(-1)


def flip_data(board, policy, mode="lr"):
    """train.py:17-27: left-right / top-bottom flips of the planes and of the policy."""
    rows, cols = board.shape[-2], board.shape[-1]
    p = policy.reshape(rows, cols)
    if mode == "lr":
        return np.flip(board, axis=2), np.fliplr(p).reshape(-1)
    return np.flip(board, axis=1), np.flipud(p).reshape(-1)


def element_source_map(s, rows, cols):
    """int array [rows * cols]: the image of a board under D4 element s of the emission's order (0 rot0, 1 lr, 2 tb, 3 rot90, 4 lr(rot90),
    5 tb(rot90), 6 rot180, 7 rot270; np.rot90 is counter-clockwise) is flat[element_source_map] - numpy's own flips applied to the indices."""
    idx = np.arange(rows * cols).reshape(rows, cols)
    r90 = (lambda a: np.rot90(a, k=1))
    img = [lambda a: a, np.fliplr, np.flipud, r90, lambda a: np.fliplr(r90(a)), lambda a: np.flipud(r90(a)),
           lambda a: np.rot90(a, k=2), lambda a: np.rot90(a, k=3)][s](idx)
    if img.shape != (rows, cols):
        raise ValueError(f"element {s} transposes: a {rows} x {cols} board does not admit it")
    return np.ascontiguousarray(img).reshape(-1)


def element_image(board, policy, s):
    """(board, policy) under element s: every plane turned; the policy turned with the cells where there is one action per cell, mirrored
    under element 1 where there is one per column (Connect4: only elements 0 and 1 keep gravity)."""
    planes, rows, cols = board.shape
    src = element_source_map(s, rows, cols)
    b = np.ascontiguousarray(board.reshape(planes, rows * cols)[:, src].reshape(planes, rows, cols))
    policy = np.asarray(policy)
    if len(policy) == rows * cols:
        return b, policy[src].copy()
    if s not in (0, 1):
        raise ValueError(f"element {s}: a policy of {len(policy)} column actions admits elements 0 and 1 only")
    return b, (policy[::-1].copy() if s == 1 else policy.copy())


def _add_group(Game, buffer, canon, policy, target, i, elements):
    """One position's tuples: once for positions 0 and 1, else the reference's eight images, or one per element."""
    if i < 2:
        buffer.add(canon, policy, target)
        return
    if elements is not None:
        for s in elements:
            b, p = element_image(np.asarray(canon), policy, s)
            buffer.add(b, p, target)
        return
    for r in range(4):
        b, p = rotate_data(canon, policy, k=r)
        buffer.add(b, p, target)
        if r < 2:
            for mode in ("lr", "tb"):
                fb, fp = flip_data(b, p, mode)
                buffer.add(fb, fp, target)


def save_data_to_buffer(Game, buffer, data, full=None, elements=None, copies=None, first_ply=0, values=None):
    """train.py:30-49: z = +reward for the winner's positions, -reward for the loser's; canonical boards; positions 0 and 1
    once, every later position with its 8 dihedral images in the reference's order.  full (playout cap, SelfPlayResult.full): one flag
    per position; the positions of fast searches are left out, the others keep the group they would have had.  elements (OPT-IN; None:
    the reference's code path): a tuple of D4 elements, ascending - every later position once per element instead (element_image), on any
    board and for Connect4's column actions: what an engine created with that emit_symmetry puts into a DeviceReplay.  copies (OPT-IN surprise
    weighting; None: once each): one count per position (selfplay.surprise_copies) - the position's whole group is added that many times, copy
    after copy, what an engine with surprise weighting puts into a DeviceReplay; a position with 0 copies is left out.  first_ply (OPT-IN random
    openings, SelfPlayResult.open_plies; 0: the reference's code path): boards[0] is the game's position at ply first_ply - the plies of its
    opening had no search and are not in `data` - so the side to move starts at first_ply & 1 and the once-or-group rule goes by the absolute
    ply first_ply + i: what an engine with openings puts into a DeviceReplay.  values (OPT-IN value targets; None: the reference's code path):
    one float64 target per position (selfplay.value_targets) that replaces [+-reward] in every tuple of the position - each image, each copy:
    what an engine with value targets puts into a DeviceReplay, which keeps it as float32."""
    boards, actions, policies, qs, winner, reward = data
    current = int(first_ply) & 1
    for i in range(len(boards)):
        target = [reward] if current == winner else [-reward]
        if values is not None:
            target = [float(values[i])]
        canon = Game.get_canonical_board(boards[i], current)
        current = 1 - current
        if full is not None and not full[i]:
            continue
        for _ in range(1 if copies is None else int(copies[i])):
            _add_group(Game, buffer, canon, policies[i], target, int(first_ply) + i, elements)


def collect_data(Game, model, buffer, iterations, mcts_iter, display=False, seed=None, batched=True, playout_cap=None, resign=None,
                 forced_playouts=None, eval_symmetry=None, emit_symmetry=None, surprise_weight=None, gumbel_root=None, openings=None, puct=None,
                 move_temperature=None, value_target=None, solver=None, root_noise=None, kld_stop=None, lead_stop=None):
    """train.py:54-83: `iterations` self-play games of Game with `model` into `buffer`; returns [first, second, draw] counts.
    batched=False plays the games one after the other through Game().self_play and save_data_to_buffer exactly as the
    reference does (global np.random stream: a seeded caller gets the reference's buffer); the default plays them as one
    engine batch with the engine's own counter-based RNG.  playout_cap = (p_full, n_fast) (OPT-IN, batched only; selfplay.check_playout_cap):
    fast searches choose their move and are not stored, in a DeviceReplay and in a host buffer alike.  resign = (v_resign, p_never[, min_ply])
    (OPT-IN, batched only; selfplay.check_resign): a game may end by resignation; its winner is the side that did not concede, and both
    buffer kinds get the positions played with z by that winner.  forced_playouts = k (OPT-IN, batched only; selfplay.check_forced_playouts):
    forced playouts at the root; both buffer kinds get the pruned pi of every stored position.  eval_symmetry = True | ("fixed", s) (OPT-IN,
    batched only; selfplay.check_eval_symmetry): every leaf is evaluated in an orientation keyed by (seed, its position), or in the one given.
    emit_symmetry = "board" | "none" | elements (OPT-IN, batched only; selfplay.check_emit_symmetry): every position from the third on is stored
    once per element of the mask, on every board - Connect4 and non-square Gomoku included; both buffer kinds get the same tuples.
    surprise_weight = lambda (OPT-IN, batched only; selfplay.check_surprise_weight): every stored position is stored as often as its policy
    surprise weight says (selfplay.surprise_copies); both buffer kinds get the same tuples.  gumbel_root = (m, c_visit, c_scale) (OPT-IN,
    batched only; selfplay.check_gumbel_root): every search is a Gumbel root search of mcts_iter simulations; both buffer kinds get
    softmax(logits + sigma(completed Q)) as the pi of every stored position.  openings = (p_open, max_plies, spread) (OPT-IN, batched only;
    selfplay.check_openings): a game starts, with probability p_open, from a position a few drawn plies in; neither buffer kind gets those plies.
    puct = (c, fpu) (OPT-IN, batched only; selfplay.check_puct): every search selects with the exploration rate c and the first-play urgency fpu.
    move_temperature (OPT-IN, batched only; selfplay.check_move_temperature): a schedule tau or dict(tau=, visit_offset=, value_cutoff=) picks
    every move; both buffer kinds still get the raw visit distribution as pi.  value_target = r | (r, lam) (OPT-IN, batched only;
    selfplay.check_value_target): the z of every stored position is (1 - r) * z + r * G, G the horizon-lam return over the game's search
    values (selfplay.value_targets); both buffer kinds get the same targets, and the trainer's mse loss takes them as they are.
    solver = True (OPT-IN, batched only; selfplay.check_solver): every search keeps exact game-end proofs; what is stored does not change shape.
    root_noise = ("legal", alpha) | ("total", alpha_total) (OPT-IN, batched only; selfplay.check_root_noise): every search's Dirichlet row is drawn
    over the legal moves of the position it starts from; what is stored does not change shape.  kld_stop = (interval, min_gain[, min_sims])
    (OPT-IN, batched only; selfplay.check_kld_stop): a search ends at the first checkpoint at which its root's visit distribution gained less
    than min_gain of KL divergence per simulation; what is stored does not change shape.  lead_stop = (interval, factor[, min_sims]) (OPT-IN,
    batched only; selfplay.check_lead_stop): a search ends once the simulations left are fewer than factor * (the most-visited root child's lead
    over the second); what is stored does not change shape."""
    from azk import DeviceReplay
    from selfplay import (check_emit_symmetry, check_surprise_weight, check_value_target, mask_elements, self_play_batch, surprise_copies,
                          value_targets)
    lam = check_surprise_weight(surprise_weight, model)
    vtg = check_value_target(value_target, model)
    if not batched:
        for name, value in (("surprise_weight", lam), ("emit_symmetry", emit_symmetry), ("playout_cap", playout_cap), ("resign", resign),
                            ("forced_playouts", forced_playouts), ("gumbel_root", gumbel_root), ("openings", openings), ("puct", puct),
                            ("move_temperature", move_temperature), ("value_target", vtg), ("solver", solver or None), ("root_noise", root_noise),
                            ("kld_stop", kld_stop), ("lead_stop", lead_stop),
                            ("eval_symmetry", None if eval_symmetry is False else eval_symmetry)):
            if value is not None:
                raise ValueError(f"collect_data: {name} needs the batched engine (batched=True)")
        results = [0, 0, 0]
        for _ in range(iterations):
            game = Game()
            boards, actions, pis, qs, winner = game.self_play(model, mcts_iter, display)
            results[2 if winner == -1 else winner] += 1
            save_data_to_buffer(Game, buffer, (boards, actions, pis, qs, winner, 0 if winner == -1 else 1))
        return results
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 31 - 1))
    on_device = isinstance(buffer, DeviceReplay)
    leaf_dtype = "bfloat16" if getattr(model, "dtype", None) is not None and str(model.dtype).endswith("bfloat16") else "float32"
    res = self_play_batch(Game.engine_name, model, iterations, mcts_iter, size=Game._size(), seed=seed, leaf_dtype=leaf_dtype,
                          replay=buffer if on_device else None, playout_cap=playout_cap, resign=resign, forced_playouts=forced_playouts,
                          eval_symmetry=eval_symmetry, emit_symmetry=emit_symmetry, surprise_weight=surprise_weight, gumbel_root=gumbel_root,
                          openings=openings, puct=puct, move_temperature=move_temperature, value_target=value_target, solver=solver,
                          root_noise=root_noise, kld_stop=kld_stop, lead_stop=lead_stop)
    emit = check_emit_symmetry(emit_symmetry, Game.engine_name, Game._size())
    results = [0, 0, 0]
    for r in res:
        results[2 if r.winner == -1 else r.winner] += 1
        if not on_device:
            reward = 0 if r.winner == -1 else 1
            full = r.full if playout_cap is not None else None
            save_data_to_buffer(Game, buffer, (r.boards, r.actions, r.pis, r.qs, r.winner, reward), full=full,
                                elements=mask_elements(emit) if emit else None,
                                copies=surprise_copies(r.kl, r.coin, lam, full) if lam is not None else None, first_ply=r.open_plies,
                                values=value_targets(r.qs, r.winner, r.open_plies, *vtg) if vtg is not None else None)
        if display:
            Game.display_board(r.boards[-1])
    return results


def train(model, batch_size, buffer, train_iterations, lr, device, augment=None):
    """train.py:85-123 for a pvnet.PolicyValueNet: a fresh Adam, `train_iterations` sampled batches, the reference's loss;
    the network's weights are updated in place; returns (loss, policy_loss, value_loss, l2) of the last iteration.  augment (OPT-IN; None:
    buffer.sample(batch_size) as ever) goes to buffer.sample(batch_size, augment=augment) - azk.DeviceReplay turns every drawn row by a D4
    element of its own."""
    import torch
    from trainer import Trainer
    tr = Trainer(model.cfg, model.state_dict(), device=device)

    def batches():
        for _ in range(train_iterations):
            s, p, z = buffer.sample(batch_size) if augment is None else buffer.sample(batch_size, augment=augment)
            yield s, p.to(torch.float32), z.reshape(-1, 1)
    dist = torch.distributed if torch.distributed.is_available() and torch.distributed.is_initialized() else None
    out = tr.train(batches(), lr, dist=dist)
    model.load_state_dict(tr.state_dict())
    return out
