"""Arena on the batched engine: test.compete / test.compare (test.py:60-140).

compete: two agents alternate by side to move (model1 plays player 0); every move is a fresh-root search with the
mover's model and iteration count (Dirichlet noise on, as Game.mcts's default); the move is sampled from the visit
distribution while move_count < 20 when `sampling`, else the first most-visited child; returns the winner.
compare: `iterations` games, the best model plays first in the first half and second in the second half; draws score
0.5 each; optional early stopping at 55 %.  All games of a half run as one lock-step batch; the early-stopping rule
is then applied to the outcomes in game order, which yields exactly what the sequential loop would return.
"""
import numpy as np

from selfplay import self_play_batch


def _game_name(game, size):
    """`game`: an engine name ("gomoku", ...) or one of the facade's Game classes (games.Gomoku, ...), as test.py passes it."""
    if isinstance(game, str):
        return game, size
    return game.engine_name, (game._size() if size is None else size)


def compete_batch(game, model1, model2, n_games, model1_mcts_iter=50, model2_mcts_iter=50, sampling=False, size=None,
                  seed=0, first_global_game=0, device=0, leaf_dtype="float32", noise_fn=None, uniform_fn=None, cache_entries=0,
                  openings=None, openings_first_game=None, puct=None, move_temperature=None, solver=None, lead_stop=None):
    """n_games independent test.compete games at once -> (winners int array in {0, 1, -1}, final boards).

    cache_entries > 0 turns on the per-game eval cache, which - like the reference's process-global MCTS.cache (mcts.py:7,
    38-44: keyed by the position alone) - is shared by BOTH models: whichever model evaluated a position first also answers
    for the other.  That reproduces the reference's compete games exactly as long as no entry is evicted (direct-mapped
    table: size it well above the positions a game visits); with 0 every model evaluates its own positions.

    openings = (max_plies, spread) (OPT-IN, selfplay.check_openings with p_open = 1): every game starts from a drawn position - 1..max_plies
    plies inside the centred window - keyed (seed, (openings_first_game or first_global_game) + game, move 0); player 0 is still model1,
    whoever is to move first; both models then search the same number of iterations and neither may be None (ValueError).

    puct = (c, fpu) (OPT-IN, selfplay.check_puct): BOTH sides search under the same exploration rate and first-play urgency - the setting is
    the arena's, not a model's; neither model may be None (ValueError).

    move_temperature (OPT-IN, selfplay.check_move_temperature): a schedule tau or dict(tau=, visit_offset=, value_cutoff=) - BOTH sides pick
    their moves by it, and it replaces what `sampling` would do (sampling is then not looked at).

    solver = True (OPT-IN, selfplay.check_solver): BOTH sides search with exact game-end proofs (Engine.set_solver) - a side that has seen a
    forced win plays it; each result's root_status holds the movers' proven statuses.  Neither model may be None (ValueError).

    lead_stop = (interval, factor[, min_sims]) (OPT-IN, selfplay.check_lead_stop): BOTH sides end a search once the simulations left are fewer
    than factor * (the most-visited root child's lead over the second); the interval lies in 1 .. the larger of the two
    iteration counts.  With sampling off and factor 1 the games are the option-off games move for move, for fewer simulations; each result's
    sims holds the simulations every search ran.  Neither model may be None (ValueError)."""
    game, size = _game_name(game, size)
    opn = _arena_openings(openings)
    res = self_play_batch(game, (model1, model2), n_games, (model1_mcts_iter, model2_mcts_iter), size=size, seed=seed,
                          first_global_game=first_global_game, device=device, leaf_dtype=leaf_dtype,
                          noise_fn=noise_fn, uniform_fn=uniform_fn, sample_until=20 if sampling else 0, cache_entries=cache_entries,
                          openings=opn, openings_first_game=openings_first_game, puct=puct, move_temperature=move_temperature, solver=solver,
                          lead_stop=lead_stop)
    winners = np.array([r.winner for r in res], np.int64)
    return winners, res


def _arena_openings(openings):
    """(max_plies, spread) -> the runners' (1.0, max_plies, spread), or None."""
    if openings is None:
        return None
    try:
        max_plies, spread = openings
    except (TypeError, ValueError):
        raise ValueError(f"openings must be (max_plies, spread), not {openings!r}")
    return (1.0, max_plies, spread)


def compete(Game, model1, model2, model1_mcts_iter=50, model2_mcts_iter=50, sampling=False, display=False):
    """test.compete (test.py:60-105) for ONE game, as the reference runs it: the facade's primitives, one search per move,
    np.random.dirichlet / np.random.choice / np.random.randint from the global stream where the reference draws them, and
    one eval cache shared by both models (MCTS.cache).  Returns (winner, final board).  Use compete_batch for throughput."""
    from ai import Node
    game = Game()
    player, move_count = 0, 0
    while True:
        if display:
            Game.display_board(game.board)
        root = Node(None, None, player, move_count)
        if player == 0:
            Game.mcts(model1, game.board, root, model1_mcts_iter)
        else:
            Game.mcts(model2, game.board, root, model2_mcts_iter)
        child = root.sample_child(Game) if (sampling and move_count < 20) else root.max_visit_child()
        player = Game.make_move(game.board, player, child.prevAction)
        move_count += 1
        winner = Game.check_winner(game.board, root.currentPlayer, child.prevAction)
        if winner != -1:
            return winner, game.board
        if move_count == Game.state_dim:
            return -1, game.board


def score_like_reference(winners_first_half, winners_second_half, iterations, early_stopping):
    """test.compare's bookkeeping (test.py:107-140) over outcomes given in game order.
    Returns 1 / 0 on an early stop (accepted / rejected) else the contender's win rate."""
    win_count = [0, 0, 0]                                      # best model's, contender's, draws
    outcomes = list(winners_first_half) + list(winners_second_half)
    for i, winner in enumerate(outcomes):
        first = i < iterations // 2
        if winner == 0:
            win_count[0 if first else 1] += 1
        elif winner == 1:
            win_count[1 if first else 0] += 1
        else:
            win_count[0] += 0.5
            win_count[1] += 0.5
            win_count[2] += 1
        if early_stopping:
            if win_count[1] >= int(iterations * 0.55):
                return 1
            if win_count[1] + (iterations - (i + 1)) < int(iterations * 0.55):
                return 0
    return win_count[1] / iterations


def compare_sequential(Game, best_model, contender_model, best_model_mcts_iter, contender_model_mcts_iter, iterations, sampling,
                       early_stopping, winners_out=None):
    """test.compare exactly as the reference runs it (test.py:107-140): the games one after the other through `compete` (global
    np.random stream, MCTS.cache kept across the games and shared by both models), the models swap sides at half time, the
    early-stopping rule is applied after every game (so it also decides how many games are played).  Returns 1 / 0 on an
    early stop, else the contender's win rate.  `winners_out` (a list) receives each game's winner."""
    win_count = [0, 0, 0]                                      # best model's, contender's, draws
    for i in range(iterations):
        first = i < iterations // 2
        winner, _ = compete(Game, best_model if first else contender_model, contender_model if first else best_model,
                            best_model_mcts_iter if first else contender_model_mcts_iter,
                            contender_model_mcts_iter if first else best_model_mcts_iter, sampling=sampling)
        if winners_out is not None:
            winners_out.append(int(winner))
        if winner == 0:
            win_count[0 if first else 1] += 1
        elif winner == 1:
            win_count[1 if first else 0] += 1
        else:
            win_count[0] += 0.5
            win_count[1] += 0.5
            win_count[2] += 1
        if early_stopping:
            if win_count[1] >= int(iterations * 0.55):
                return 1
            if win_count[1] + (iterations - (i + 1)) < int(iterations * 0.55):
                return 0
    return win_count[1] / iterations


def compare(game, best_model, contender_model, best_model_mcts_iter, contender_model_mcts_iter, iterations, sampling,
            early_stopping, size=None, seed=0, device=0, leaf_dtype="float32", openings=None, puct=None, move_temperature=None, solver=None,
            lead_stop=None):
    """test.compare(Game, best_model, contender_model, best_iter, contender_iter, iterations, sampling, early_stopping)
    (test.py:107-140) with all games of a half played at once; a model of None plays vanilla MCTS (main.py:76).
    (compare_sequential is the game-by-game form that reproduces the reference's RNG stream and cache history.)
    openings = (max_plies, spread) (OPT-IN): every game starts from a drawn position and the openings have a first game index of their own,
    the same for both halves - game i of the second half starts from the position game i of the first half started from, with the models
    swapped, so each opening is played with both colours.  An odd `iterations` has no such pairs and is refused (ValueError).
    puct = (c, fpu) (OPT-IN, selfplay.check_puct): both models search under that exploration rate and first-play urgency in both halves.
    move_temperature (OPT-IN, selfplay.check_move_temperature): both models pick their moves by that schedule in both halves, in place of
    what `sampling` would do.
    solver = True (OPT-IN, selfplay.check_solver): both models search with exact game-end proofs in both halves.
    lead_stop = (interval, factor[, min_sims]) (OPT-IN, selfplay.check_lead_stop): both models' searches end under the lead rule in both halves."""
    game, size = _game_name(game, size)
    if lead_stop is not None:
        from selfplay import check_lead_stop
        check_lead_stop(lead_stop, (best_model_mcts_iter, contender_model_mcts_iter), (best_model, contender_model))
    if solver:
        from selfplay import check_solver
        check_solver(solver, (best_model, contender_model), puct=puct)
    if move_temperature is not None:
        from selfplay import check_move_temperature
        check_move_temperature(move_temperature, (best_model_mcts_iter, contender_model_mcts_iter), game, size)
    if puct is not None:
        from selfplay import check_puct
        check_puct(puct, (best_model, contender_model))
    if openings is not None:
        from selfplay import check_openings
        check_openings(_arena_openings(openings), game, size, (best_model, contender_model))
        if iterations % 2:
            raise ValueError(f"compare: openings pair game i of the first half with game i of the second - iterations must be even, not {iterations!r}")
    half = iterations // 2
    w1, _ = compete_batch(game, best_model, contender_model, half, best_model_mcts_iter, contender_model_mcts_iter,
                          sampling, size, seed, 0, device, leaf_dtype, openings=openings, openings_first_game=0, puct=puct,
                          move_temperature=move_temperature, solver=solver, lead_stop=lead_stop) if half else (np.zeros(0, np.int64), None)
    w2, _ = compete_batch(game, contender_model, best_model, iterations - half, contender_model_mcts_iter,
                          best_model_mcts_iter, sampling, size, seed, half, device, leaf_dtype, openings=openings, openings_first_game=0, puct=puct,
                          move_temperature=move_temperature, solver=solver, lead_stop=lead_stop)
    return score_like_reference(w1, w2, iterations, early_stopping)
