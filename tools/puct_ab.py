#!/usr/bin/env python3
"""Same-box A/B of configurable PUCT (azk_set_puct) inside the asynchronous movers at the headline workload: Gomoku 15x15,
2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries, and the pre-roll of
tools/tree_reuse_ab.py.

    python3 tools/puct_ab.py [--out profiles/puct_ab.json] [--c-init 1.25] [--c-base 19652] [--fpu-reduction 0.3] [--fpu-root 0.0]

Lines: 1 asynchronous off, 2 asynchronous with set_puct(1.0) - the trees are those of line 1, so the workload is the same and the difference
is what the sibling kernels' extra per-level work costs - and 3 asynchronous with AlphaZero's schedule and a first-play-urgency reduction,
which is ANOTHER search (deeper, narrower): its line is a description, not a cost.  The three are run --rounds times, alternated.  Then
three children under `rocprofv3 --kernel-trace --stats`, runs of their own (4 off, 5 c = 1, 6 the schedule), for k_tree per launch.  One child
process per line, one after the other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is
started on the GPU).  Per timed line: ms per G moves, k_tree per launch (HIP events, every timer_stride-th launch), the mean walk depth
(trace nodes per simulation), leaves evaluated per move, the eval cache's hit share and the plies of finished games.  There is no speed bar.
What either setting does to the strength of a trained network is not measured here.
"""
import argparse
import json
import sys

import ab_common as ab

LINES = [("async off", "off"), ("async puct c=1", "one"), ("async puct schedule+fpu", "schedule")]
TRACED = {4: "off", 5: "one", 6: "schedule"}


def option(args, which):
    if which == "off":
        return None
    if which == "one":
        return (1.0, None)
    return ((args.c_init, args.c_base), ("reduction", args.fpu_reduction, args.fpu_root))


def worker(args):
    from selfplay import KernelTimer
    name, which = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, puct=option(args, which))
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    moves = max(1, d["moves"])
    print(json.dumps(dict(fields, line=args.line, name=name, puct=repr(option(args, which)),
                          mean_walk_depth=c["trace_nodes"] / max(1, c["sims"]), edges_scanned_per_sim=c["edges_scanned"] / max(1, c["sims"]),
                          terminal_share=c["terminal_sims"] / max(1, c["sims"]), **ab.leaf_fields(c, moves))))


def traced(args):
    """A short run for the profiler."""
    from selfplay import KernelTimer
    runner = ab.async_runner(args, KernelTimer(stride=args.timer_stride), ab.device_replay(args), puct=option(args, TRACED[args.line]))
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
    ap.add_argument("--c-init", type=float, default=1.25)
    ap.add_argument("--c-base", type=float, default=19652.0)
    ap.add_argument("--fpu-reduction", type=float, default=0.3)
    ap.add_argument("--fpu-root", type=float, default=0.0)
    ap.add_argument("--no-trace", action="store_true", help="leave the three profiler runs out")
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("puct_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return traced(args) if args.line in TRACED else worker(args)
    forwarded = ("games", "sims", "size", "c_init", "c_base", "fpu_reduction", "fpu_root", "steps", "warmup", "preroll_cheap", "preroll_full",
                 "cache_entries", "replay_capacity", "per_launch", "steps_per_graph", "timer_stride")
    status, rows = ab.collect_lines(__file__, args, [1, 2, 3], forwarded, rounds=args.rounds)
    if status != 0:
        return status
    kernels = {}
    for line, which in ([] if args.no_trace else sorted(TRACED.items())):
        status, kernels[which] = ab.traced_kernels(ab.child_cmd(__file__, args, "--line", line, forwarded), 2 * args.timeout,
                                                   f"kernel trace {line}", ("k_tree",))
        if status != 0:
            return status
    keys = ("ms_per_G_moves", "k_tree_us_per_launch", "mean_walk_depth", "leaves_evaluated_per_move", "cache_hit_share", "mean_plies_of_finished_games")
    summary = {LINES[i - 1][0]: {k: ab.mean_of(rows, i, k) for k in keys} for i in (1, 2, 3)}
    ab.write_doc(args.out, what="configurable PUCT inside the asynchronous movers at the headline workload, one box, one process after the other, the "
                 "three lines alternated (tools/puct_ab.py); 'off' against 'c=1' is one workload (identical trees) and prices the sibling kernels' "
                 "per-level work, 'schedule+fpu' is another search and is described, not priced; the kernel times come from rocprofv3 "
                 "--kernel-trace --stats runs of their own; the strength of a network searched or trained under either setting is not measured",
                 lines=rows, means=summary, kernels_us_per_launch=kernels)
    print(json.dumps(dict(means=summary, kernels=kernels)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
