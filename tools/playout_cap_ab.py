#!/usr/bin/env python3
"""Same-box A/B of playout-cap randomisation (azk_set_playout_cap) inside the asynchronous movers at the headline
workload: Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries,
and the pre-roll of tools/tree_reuse_ab.py.

    python3 tools/playout_cap_ab.py [--out profiles/playout_cap_ab.json] [--p-full 0.25] [--n-fast 100]

Lines: 1 asynchronous off, 2 asynchronous with the cap, 3 asynchronous top-up, 4 asynchronous top-up with the cap.  One child process
per line, one after the other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is
started on the GPU).  Per line: ms per G moves and moves/s, games/s with the mean plies, simulations and tree launches per move, the
share of full searches, recorded (state, pi, z) tuples per second (the replay ring's cursor), k_tree's mean time per launch (HIP events
around sampled eager launches) and the drain's share of the time (HIP events around azk_async_drain).  There is no speed bar.  The one
derived expectation: tree launches per G moves follow the mean simulations per move - p_full * n_sims + (1 - p_full) * n_fast of the
800 without reuse.
"""
import argparse
import json
import sys

import ab_common as ab

# (name, tree reuse mode, playout cap on)
LINES = [("async off", 0, False), ("async cap", 0, True), ("async top-up", 2, False), ("async top-up cap", 2, True)]


def worker(args):
    from selfplay import KernelTimer
    name, mode, capped = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    cap = (args.p_full, args.n_fast) if capped else None
    runner = ab.async_runner(args, kt, replay, reroot=mode, playout_cap=cap)
    drain_events = []
    ab.bracket_calls(runner.eng, "async_drain", drain_events, lambda *a, **k: kt.enabled)
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    moves = max(1, d["moves"])
    expected = args.p_full * args.sims + (1.0 - args.p_full) * args.n_fast if capped else float(args.sims)
    print(json.dumps(dict(fields, line=args.line, name=name, tree_reuse=mode, playout_cap=list(cap) if cap else None,
                          derived_sims_per_move_without_reuse=expected,
                          full_share_of_searches=(d["full"] / max(1, d["full"] + d["fast"])) if capped else 1.0,
                          recorded_tuples_per_s=d["tuples"] / dt, roots_reused_share=c["roots_reused"] / moves, drains=d["drains"],
                          **ab.leaf_fields(c, moves), **ab.drain_fields(drain_events, dt))))


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line")
    ap.add_argument("--lines", default="1,2,3,4")
    ab.add_common_args(ap, "games", "sims", "size")
    ap.add_argument("--p-full", type=float, default=0.25)
    ap.add_argument("--n-fast", type=int, default=100)
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout", steps_per_graph=8,
                       help=dict(steps_per_graph="steps between two drains (tree_reuse_async_ab.json: 8 is the best top-up line)"))
    ap.add_argument("--out", default=ab.out_path("playout_cap_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    return ab.run_lines(__file__, args, [int(x) for x in args.lines.split(",")],
                        ("games", "sims", "size", "p_full", "n_fast", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries",
                         "replay_capacity", "per_launch", "steps_per_graph", "timer_stride"),
                        "playout-cap randomisation inside the asynchronous movers at the headline workload, one box, one process after the other "
                        "(tools/playout_cap_ab.py); moves/s and games/s are measured, derived_sims_per_move_without_reuse is arithmetic on the options",
                        args.out)


if __name__ == "__main__":
    sys.exit(main())
