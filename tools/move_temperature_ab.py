#!/usr/bin/env python3
"""Same-box A/B of the move temperature (azk_set_move_temperature) inside the asynchronous movers at the headline workload:
Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries, and the pre-roll of
tools/tree_reuse_ab.py.

    python3 tools/move_temperature_ab.py [--out profiles/move_temperature_ab.json] [--t0 1.0] [--halflife 10] [--t-final 0.1]
                                         [--visit-offset 1] [--value-cutoff 0.2] [--no-trace]

Lines: 1 asynchronous off (the reference's rule: in proportion to the visits for 8 plies, then the most-visited child), 2 asynchronous with
tau(p) = t_final + (t0 - t_final) * 0.5 ** (p / halflife), a visit offset and a value cutoff.  Line 2 plays OTHER games (it samples on every
ply), so the pair describes the option at this workload - the mover's own cost is the k_move_async line.  The two are run --rounds times,
alternated.  Then two children under `rocprofv3 --kernel-trace --stats`, runs of their own (3 off, 4 on), for k_move_async per launch.  One
child process per line, one after the other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing
more is started on the GPU).  Per timed line: ms per G moves, the option's four counters over the timed window,
the plies of finished games, the eval cache's hit share.  There is no speed bar.  What a schedule does to the strength of a network trained
on its games is not measured here.
"""
import argparse
import json
import sys

import ab_common as ab

LINES = [("async off", False), ("async move temperature", True)]
TRACED = {3: False, 4: True}


def option(args, on):
    if not on:
        return None
    return dict(tau=("halflife", args.t0, args.halflife, args.t_final), visit_offset=args.visit_offset, value_cutoff=args.value_cutoff)


def worker(args):
    from selfplay import KernelTimer
    name, on = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, move_temperature=option(args, on))
    ab.preroll(runner, args)
    runner.finish()
    before = runner.move_temperature_stats() if on else None      # (the pre-roll's cheap searches are not the workload: the window's own counts)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    stats = [b - a for a, b in zip(before, runner.move_temperature_stats())] if on else None
    print(json.dumps(dict(fields, line=args.line, name=name, move_temperature=repr(option(args, on)), move_temperature_stats=stats,
                          not_most_visited_share=None if not on else stats[1] / max(1, stats[0]), **ab.leaf_fields(c, max(1, d["moves"])))))


def traced(args):
    """A short run for the profiler."""
    from selfplay import KernelTimer
    runner = ab.async_runner(args, KernelTimer(stride=args.timer_stride), ab.device_replay(args), move_temperature=option(args, TRACED[args.line]))
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
    ap.add_argument("--t0", type=float, default=1.0)
    ap.add_argument("--halflife", type=float, default=10.0)
    ap.add_argument("--t-final", type=float, default=0.1)
    ap.add_argument("--visit-offset", type=int, default=1)
    ap.add_argument("--value-cutoff", type=float, default=0.2)
    ap.add_argument("--no-trace", action="store_true", help="leave the two profiler runs out")
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("move_temperature_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return traced(args) if args.line in TRACED else worker(args)
    forwarded = ("games", "sims", "size", "t0", "halflife", "t_final", "visit_offset", "value_cutoff", "steps", "warmup", "preroll_cheap",
                 "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph", "timer_stride")
    status, rows = ab.collect_lines(__file__, args, [1, 2], forwarded, rounds=args.rounds)
    if status != 0:
        return status
    kernels = {}
    for line, on in ([] if args.no_trace else sorted(TRACED.items())):
        status, kernels["on" if on else "off"] = ab.traced_kernels(ab.child_cmd(__file__, args, "--line", line, forwarded), 2 * args.timeout,
                                                                    f"kernel trace {line}", ("k_move_async",))
        if status != 0:
            return status
    keys = ("ms_per_G_moves", "mean_plies_of_finished_games", "cache_hit_share", "leaves_evaluated_per_move", "not_most_visited_share")
    summary = {LINES[i - 1][0]: {k: ab.mean_of(rows, i, k) for k in keys} for i in (1, 2)}
    ab.write_doc(args.out, what="the move temperature inside the asynchronous movers at the headline workload, one box, one process after the other, "
                 "the two lines alternated (tools/move_temperature_ab.py); 'on' samples on every ply and so plays other games than 'off': the pair "
                 "describes the option, k_move_async per launch (rocprofv3 --kernel-trace --stats runs of their own) is the mover's cost; the four "
                 "counters cover the timed window; the strength of a network trained on either line's games is not measured",
                 lines=rows, means=summary, kernels_us_per_launch=kernels)
    print(json.dumps(dict(means=summary, kernels=kernels)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
