#!/usr/bin/env python3
"""Same-box A/B of forced playouts and policy target pruning (azk_set_forced_playouts) inside the asynchronous movers at the
headline workload: Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768
entries, and the pre-roll of tools/tree_reuse_ab.py.

    python3 tools/forced_playouts_ab.py [--out profiles/forced_playouts_ab.json] [--k 2]

Lines: 1 asynchronous off, 2 asynchronous with forced playouts (k).  One child process per line, one after the other on the same GPU,
each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per line: ms per G moves
and moves/s, games/s with the mean plies of the games that finished, k_tree's mean time per launch (HIP events around sampled eager
launches), and from the device counters (azk_counters, no restatement involved) the share of root selections that took a forced child and
the share of the recorded visits that pruning removed.  There is no speed bar: the option changes the search, so games last another
number of plies and moves/s of the two lines are not one workload - ms per G moves and k_tree us per launch are the comparable figures.
"""
import argparse
import json
import sys

import ab_common as ab

# (name, forced playouts on)
LINES = [("async off", False), ("async forced playouts", True)]


def worker(args):
    from selfplay import KernelTimer
    name, forced = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, forced_playouts=args.k if forced else None)
    drain_events = []
    ab.bracket_calls(runner.eng, "async_drain", drain_events, lambda *a, **k: kt.enabled)
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    moves = max(1, d["moves"])
    print(json.dumps(dict(fields, line=args.line, name=name, forced_playouts=args.k if forced else 0.0,
                          forced_share_of_root_selections=c["forced_selections"] / max(1, c["sims"]),
                          pruned_share_of_recorded_visits=c["visits_pruned"] / max(1, c["visits_before_pruning"]),
                          recorded_tuples_per_s=d["tuples"] / dt, drains=d["drains"],
                          **ab.leaf_fields(c, moves), **ab.drain_fields(drain_events, dt))))


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line")
    ap.add_argument("--lines", default="1,2")
    ab.add_common_args(ap, "games", "sims", "size")
    ap.add_argument("--k", type=float, default=2.0, help="forced playouts' k of line 2 (KataGo: 2)")
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("forced_playouts_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    return ab.run_lines(__file__, args, [int(x) for x in args.lines.split(",")],
                        ("games", "sims", "size", "k", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity",
                         "per_launch", "steps_per_graph", "timer_stride"),
                        "forced playouts and policy target pruning inside the asynchronous movers at the headline workload, one box, one process after "
                        "the other (tools/forced_playouts_ab.py); every figure is measured, the two shares come from the device counters",
                        args.out)


if __name__ == "__main__":
    sys.exit(main())
