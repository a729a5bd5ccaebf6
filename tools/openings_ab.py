#!/usr/bin/env python3
"""Same-box A/B of random openings (azk_set_openings) inside the asynchronous movers at the headline workload: Gomoku
15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries, and the pre-roll of
tools/tree_reuse_ab.py.

    python3 tools/openings_ab.py [--out profiles/openings_ab.json] [--p-open 0.5] [--max-plies 8] [--spread 2]

Lines: 1 asynchronous off, 2 asynchronous with the openings; the pair is run --rounds times, alternated.  Then two diversity lines (3 off, 4
on): the lock-step graph runner plays the first games of the G slots for ten plies and counts the distinct boards among them at their first
searched ply and at ply 10 - the figure the option exists for.  Then two children under `rocprofv3 --kernel-trace --stats`, runs of their
own (5 off, 6 on), for k_async_restart per launch off and on and k_open_pending per launch.  One child process per line, one after the
other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per timed line: ms per G moves and moves/s, games/s
with the mean plies of finished games (opening plies included), the drain's time per call (HIP events around azk_async_drain), recorded
tuples per second and the option's three counts.  There is no speed bar.  What the option does to the strength of a trained network is not
measured here.
"""
import argparse
import json
import sys

import ab_common as ab

LINES = [("async off", False), ("async openings", True)]
DIVERSITY = {3: ("diversity off", False), 4: ("diversity openings", True)}
TRACED = {5: False, 6: True}
PLY = 10


def option(args, on):
    return (args.p_open, args.max_plies, args.spread) if on else None


def worker(args):
    from selfplay import KernelTimer
    name, on = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, openings=option(args, on))
    drain_events = []
    ab.bracket_calls(runner.eng, "async_drain", drain_events, lambda *a, **k: kt.enabled)
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    moves = max(1, d["moves"])
    print(json.dumps(dict(fields, line=args.line, name=name, openings=list(option(args, on)) if on else None,
                          recorded_tuples_per_s=d["tuples"] / dt, drains=d["drains"],
                          openings_opened_plies_cut=runner.eng.opening_stats() if on else None,
                          **ab.leaf_fields(c, moves), **ab.drain_fields(drain_events, dt))))


def diversity(args):
    """The first games of the G slots on the lock-step graph runner: distinct boards at the first searched ply and at ply PLY."""
    import numpy as np
    from selfplay import SelfPlayRunner
    name, on = DIVERSITY[args.line]
    chosen = []
    runner = SelfPlayRunner("gomoku", ab.headline_net(args), args.games, args.sims,
                            on_records=lambda mv, base, pi, q, ch, w, d: chosen.append(ch.numpy().copy()),
                            **ab.headline_options(args, None, recycle=False, use_graph=True, budget_stepping=True, per_launch=8, openings=option(args, on)))
    cells, to_move, mc = runner.eng.get_positions()
    boards, plies = cells.copy(), mc.copy()
    first = len({b.tobytes() for b in boards})
    at_ply = [None] * args.games
    for g in range(args.games):
        if plies[g] == PLY:
            at_ply[g] = boards[g].tobytes()
    for _ in range(PLY):
        runner.play_move()
        for g, c in enumerate(chosen[-1]):
            if c >= 0 and at_ply[g] is None:
                boards[g, c] = 1 + (plies[g] & 1)
                plies[g] += 1
                if plies[g] == PLY:
                    at_ply[g] = boards[g].tobytes()
    runner.check_error()
    reached = [b for b in at_ply if b is not None]
    print(json.dumps(dict(line=args.line, name=name, games=args.games, sims=args.sims, size=args.size, openings=list(option(args, on)) if on else None,
                          distinct_boards_at_first_searched_ply=first, games_that_reached_ply_10=len(reached),
                          distinct_boards_at_ply_10=len(set(reached)), mean_open_plies=float(np.mean(mc)))))


def traced(args):
    """A short run, off or on, for the profiler: a few drains' worth of restarts."""
    from selfplay import KernelTimer
    runner = ab.async_runner(args, KernelTimer(stride=args.timer_stride), ab.device_replay(args), openings=option(args, TRACED[args.line]))
    ab.preroll(runner, args)
    for _ in range(args.steps):
        runner.play_move()
    runner.finish()
    runner.check_error()


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line")
    ap.add_argument("--rounds", type=int, default=2)
    ab.add_common_args(ap, "games", "sims", "size")
    ap.add_argument("--p-open", type=float, default=0.5)
    ap.add_argument("--max-plies", type=int, default=8)
    ap.add_argument("--spread", type=int, default=2)
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("openings_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return traced(args) if args.line in TRACED else diversity(args) if args.line in DIVERSITY else worker(args)
    forwarded = ("games", "sims", "size", "p_open", "max_plies", "spread", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries",
                 "replay_capacity", "per_launch", "steps_per_graph", "timer_stride")
    status, rows = ab.collect_lines(__file__, args, [1, 2], forwarded, rounds=args.rounds)
    if status != 0:
        return status
    status, div = ab.collect_lines(__file__, args, sorted(DIVERSITY), forwarded)
    if status != 0:
        return status
    kernels = {}
    for line, on in sorted(TRACED.items()):
        status, kernels["openings" if on else "off"] = ab.traced_kernels(ab.child_cmd(__file__, args, "--line", line, forwarded), 2 * args.timeout,
                                                                          f"kernel trace {line}", ("k_open_pending", "k_async_restart"))
        if status != 0:
            return status
    summary = {LINES[i - 1][0]: {k: ab.mean_of(rows, i, k) for k in ("ms_per_G_moves", "drain_us_per_call", "mean_plies_of_finished_games")}
               for i in (1, 2)}
    ab.write_doc(args.out, what="random openings inside the asynchronous movers at the headline workload, one box, one process after the other, the "
                 "pair alternated (tools/openings_ab.py); times are measured, the diversity lines count distinct boards among the G slots' "
                 "first games, the kernel times come from a rocprofv3 --kernel-trace --stats run of their own; the strength of a network "
                 "trained on opened games is not measured", lines=rows, means=summary, diversity=div, kernels_us_per_launch=kernels)
    print(json.dumps(dict(means=summary, kernels=kernels)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
