#!/usr/bin/env python3
"""Same-box A/B of exact game-end proofs in the search (azk_set_solver) inside the asynchronous movers at the headline
workload: Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries, and the
pre-roll of tools/tree_reuse_ab.py.

    python3 tools/solver_ab.py [--out profiles/solver_ab.json] [--rounds 2]

Lines: 1 asynchronous off, 2 asynchronous with the solver on, run --rounds times, alternated.  Then two children under `rocprofv3
--kernel-trace --stats`, runs of their own (3 off, 4 on), for k_tree per launch.  One child process per line, one after the other on the same
GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per timed line: ms per G
moves, k_tree per launch (HIP events, every timer_stride-th launch), the six solver counters per move, the terminal and cache-hit shares,
leaves evaluated per move, the plies of finished games, and the share of searches whose root took a status (the counters do not keep the
simulation at which it did).  The solver is ANOTHER search wherever something is proven: its line is a description, and there is no speed
bar - the time a decided root could save lies in ending its search early, which the movers do not do yet.  What the option does to the
strength of a trained network is not measured here.
"""
import argparse
import json
import sys

import ab_common as ab

LINES = [("async off", False), ("async solver", True)]
TRACED = {3: False, 4: True}


def worker(args):
    from selfplay import KernelTimer
    name, on = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, solver=on or None)
    ab.preroll(runner, args)
    before = runner.solver_stats() if on else {}
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    moves = max(1, d["moves"])
    after = runner.solver_stats() if on else {}
    per_move = {k + "_per_move": (after[k] - before[k]) / moves for k in after}
    decided = (after["roots_proven"] - before["roots_proven"]) / max(1, d["searches"]) if on else None
    print(json.dumps(dict(fields, line=args.line, name=name, solver=on, terminal_share=c["terminal_sims"] / max(1, c["sims"]),
                          mean_walk_depth=c["trace_nodes"] / max(1, c["sims"]), share_of_searches_with_a_decided_root=decided,
                          **per_move, **ab.leaf_fields(c, moves))))


def traced(args):
    """A short run for the profiler."""
    from selfplay import KernelTimer
    runner = ab.async_runner(args, KernelTimer(stride=args.timer_stride), ab.device_replay(args), solver=TRACED[args.line] or None)
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
    ap.add_argument("--no-trace", action="store_true", help="leave the two profiler runs out")
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("solver_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return traced(args) if args.line in TRACED else worker(args)
    forwarded = ("games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
                 "steps_per_graph", "timer_stride")
    status, rows = ab.collect_lines(__file__, args, [1, 2], forwarded, rounds=args.rounds)
    if status != 0:
        return status
    kernels = {}
    for line, on in ([] if args.no_trace else sorted(TRACED.items())):
        status, kernels["on" if on else "off"] = ab.traced_kernels(ab.child_cmd(__file__, args, "--line", line, forwarded), 2 * args.timeout,
                                                                   f"kernel trace {line}", ("k_tree",))
        if status != 0:
            return status
    keys = ("ms_per_G_moves", "k_tree_us_per_launch", "terminal_share", "cache_hit_share", "leaves_evaluated_per_move", "mean_plies_of_finished_games",
            "mean_walk_depth", "share_of_searches_with_a_decided_root") + tuple(k + "_per_move" for k in
                                                                               ("terminal_marked", "proven_by_won_child", "proven_by_all_children",
                                                                                "stopped_on_proven", "selections_excluding", "roots_proven"))
    summary = {LINES[i - 1][0]: {k: ab.mean_of(rows, i, k) for k in keys} for i in (1, 2)}
    ab.write_doc(args.out, what="exact game-end proofs (the solver) inside the asynchronous movers at the headline workload, one box, one process after "
                 "the other, the two lines alternated (tools/solver_ab.py); the solver's line is another search wherever something is proven and is "
                 "described, not priced; the kernel times come from rocprofv3 --kernel-trace --stats runs of their own; the counters do not keep "
                 "the simulation at which a root was decided; the strength of a network searched or trained under the option is not measured",
                 lines=rows, means=summary, kernels_us_per_launch=kernels)
    print(json.dumps(dict(means=summary, kernels=kernels)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
