#!/usr/bin/env python3
"""Same-box A/B of root noise on the legal moves (azk_set_root_noise) inside the asynchronous movers at the headline
workload: Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries, and the
pre-roll of tools/tree_reuse_ab.py.

    python3 tools/root_noise_ab.py [--out profiles/root_noise_ab.json] [--rounds 2]

Lines: 1 off (rows over the whole action vector, alpha 0.03, made a search ahead), 2 ("legal", 0.03), 3 ("total", 10.83), run --rounds
times, alternated.  Then, per line, a child that DESCRIBES the searches from move records (4-6: fresh games, no pre-roll, --describe-moves
moves per slot): the top root child's share of a search's visits, and the distinct boards among the slots' first games after each of the
first three searched plies.  Then two children under `rocprofv3 --kernel-trace --stats`, runs of their own (7 legal, 8 total), for
k_root_noise_due per launch - the kernel the option puts into the step chain.  One child process per line, one after the other on the same
GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per timed line: ms per G
moves, k_tree per launch (HIP events), leaves evaluated per move, the cache-hit share, the plies of finished games.  The three lines are
DIFFERENT searches - the noise reaches the root's children with 100 % of its mass instead of about 1 % - so their figures are descriptions:
no target is set for them.  What either mode does to the strength of a trained network is not measured here.
"""
import argparse
import json
import sys

import ab_common as ab

LINES = [("async off", None), ("async legal 0.03", ("legal", 0.03)), ("async total 10.83", ("total", 10.83))]
DESCRIBED = {4: 0, 5: 1, 6: 2}
TRACED = {7: 1, 8: 2}


def worker(args):
    from selfplay import KernelTimer
    name, rn = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, root_noise=rn)
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    print(json.dumps(dict(fields, line=args.line, name=name, root_noise=rn, **ab.leaf_fields(c, max(1, d["moves"])))))


def describe(args):
    """Fresh games, move records on: what the searches of the first plies look like."""
    import numpy as np
    from selfplay import KernelTimer
    name, rn = LINES[DESCRIBED[args.line]]
    first, top = {}, []

    def on(meta, q, pi):
        top.extend(np.asarray(pi).max(axis=1).tolist())
        for g, mv, cell, _ in np.asarray(meta).tolist():
            if mv < 3:
                first[(g, mv)] = cell
    runner = ab.async_runner(args, KernelTimer(stride=args.timer_stride), None, root_noise=rn, on_records=on)
    for _ in range(args.describe_moves):
        runner.play_move()
    runner.finish()
    runner.check_error()
    boards = []
    for ply in range(3):                                          # a board after ply + 1 searched plies: the cells of either colour, as sets
        seen = {(frozenset(first[(g, m)] for m in range(0, ply + 1, 2)), frozenset(first[(g, m)] for m in range(1, ply + 1, 2)))
                for g in range(args.games) if all((g, m) in first for m in range(ply + 1))}
        boards.append(len(seen))
    print(json.dumps(dict(line=args.line, name=name, root_noise=rn, searches_recorded=len(top), top_child_share_of_visits=float(np.mean(top)),
                          distinct_boards_after_plies_1_2_3=boards, first_games=args.games)))


def traced(args):
    """A short run for the profiler."""
    from selfplay import KernelTimer
    runner = ab.async_runner(args, KernelTimer(stride=args.timer_stride), ab.device_replay(args), root_noise=LINES[TRACED[args.line]][1])
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
    ap.add_argument("--describe-moves", type=int, default=6, help="moves per slot of the describing children")
    ap.add_argument("--no-trace", action="store_true", help="leave the two profiler runs out")
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("root_noise_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return traced(args) if args.line in TRACED else describe(args) if args.line in DESCRIBED else worker(args)
    forwarded = ("games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
                 "steps_per_graph", "timer_stride", "describe_moves")
    status, rows = ab.collect_lines(__file__, args, [1, 2, 3], forwarded, rounds=args.rounds)
    if status != 0:
        return status
    status, described = ab.collect_lines(__file__, args, sorted(DESCRIBED), forwarded)
    if status != 0:
        return status
    kernels = {}
    for line, i in ([] if args.no_trace else sorted(TRACED.items())):
        status, kernels[LINES[i][0]] = ab.traced_kernels(ab.child_cmd(__file__, args, "--line", line, forwarded), 2 * args.timeout,
                                                         f"kernel trace {line}", ("k_root_noise_due", "k_tree", "k_move_async"))
        if status != 0:
            return status
    keys = ("ms_per_G_moves", "k_tree_us_per_launch", "cache_hit_share", "leaves_evaluated_per_move", "mean_plies_of_finished_games")
    summary = {LINES[i - 1][0]: {k: ab.mean_of(rows, i, k) for k in keys} for i in (1, 2, 3)}
    ab.write_doc(args.out, what="root noise on the legal moves inside the asynchronous movers at the headline workload, one box, one process after the "
                 "other, the three lines alternated (tools/root_noise_ab.py); the lines are different searches and are described, not priced "
                 "against each other; the describing lines play fresh games with move records on; the kernel times come from rocprofv3 "
                 "--kernel-trace --stats runs of their own; the strength of a network trained under either mode is not measured",
                 lines=rows, means=summary, described=described, kernels_us_per_launch=kernels)
    print(json.dumps(dict(means=summary, described=described, kernels=kernels)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
