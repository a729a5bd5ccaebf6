#!/usr/bin/env python3
"""Same-box A/B of tree reuse inside the asynchronous movers (azk_async_begin_reuse) at the headline workload:
Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries, and the
pre-roll of tools/tree_reuse_ab.py.

    python3 tools/tree_reuse_async_ab.py [--out profiles/tree_reuse_async_ab.json]

Lines: 1 lock-step off, 2 lock-step top-up (the baselines, SelfPlayRunner), 3 asynchronous off, 4-6 asynchronous top-up at
steps_per_graph 8 / 16 / 32 (a parked game waits for the drain that follows its move: half of steps_per_graph steps on average),
7 asynchronous carry at 32.  One child process per line, one after the other on the same GPU, each under its own time limit; the
first one that fails ends the run (nothing more is started on the GPU).  Per line: ms per G moves and moves/s, simulations, tree
launches and evaluator leaves per move, the share of roots reused and the nodes carried per re-root, games/s with the mean plies
(NOT comparable across modes: reuse changes how long games last), k_tree's mean time per launch (HIP events around sampled eager
launches) and, for the asynchronous lines, the drain's time per call (HIP events around azk_async_drain) with the games it re-rooted.
There is no speed bar: the record says whether asynchronous top-up beats the two lock-step lines in moves/s.
"""
import argparse
import json
import sys

import ab_common as ab

# (name, asynchronous, tree reuse mode, steps per graph)
LINES = [("lock-step off", False, 0, 32), ("lock-step top-up", False, 2, 32), ("async off", True, 0, 32),
         ("async top-up spg 8", True, 2, 8), ("async top-up spg 16", True, 2, 16), ("async top-up spg 32", True, 2, 32),
         ("async carry spg 32", True, 1, 32)]


def worker(args):
    from selfplay import KernelTimer, SelfPlayRunner
    name, is_async, mode, spg = LINES[args.line - 1]
    kt = KernelTimer(stride=args.timer_stride)
    drain_events = []
    if is_async:
        runner = ab.async_runner(args, kt, None, reroot=mode, steps_per_graph=spg)
        ab.bracket_calls(runner.eng, "async_drain", drain_events, lambda *a, **k: kt.enabled)
    else:
        runner = SelfPlayRunner("gomoku", ab.headline_net(args), args.games, args.sims, use_graph=True, n_split=1, tree_reuse=mode,
                                **ab.headline_options(args, kt, steps_per_graph=spg))
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, None, args, args.steps)
    moves = max(1, d["moves"])
    out = dict(fields, line=args.line, name=name, asynchronous=is_async, tree_reuse=mode, per_launch=args.per_launch if is_async else None,
               roots_reused_share=c["roots_reused"] / moves, nodes_carried_per_reroot=c["nodes_carried"] / max(1, c["roots_reused"]),
               **ab.leaf_fields(c, moves))
    if is_async:
        # searches begun = re-roots (carried or fallback) + restarts of finished games; engines without reuse begin them in the move kernel
        out.update(drains=d["drains"], games_rerooted_per_drain=(d["searches"] - d["games"]) / max(1, d["drains"]) if mode else 0.0,
                   **ab.drain_fields(drain_events, dt))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line")
    ap.add_argument("--lines", default="1,2,3,4,5,6,7")
    ab.add_common_args(ap, "games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "per_launch", "timer_stride",
                       "timeout", help=dict(per_launch="asynchronous lines: most simulations a game runs inside one tree launch"))
    ap.add_argument("--out", default=ab.out_path("tree_reuse_async_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    status, rows = ab.collect_lines(__file__, args, [int(x) for x in args.lines.split(",")],
                                    ("games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "per_launch",
                                     "timer_stride"))
    if status != 0:
        return status
    base = {r["line"]: r["moves_per_s"] for r in rows}
    best = max((r for r in rows if r["asynchronous"] and r["tree_reuse"] == 2), key=lambda r: r["moves_per_s"], default=None)
    ab.write_doc(args.out, what="tree reuse inside the asynchronous movers against the lock-step runners at the headline workload, one box, one process "
                                "after the other (tools/tree_reuse_async_ab.py); games/s are not comparable across modes",
                 best_async_top_up=None if best is None else best["name"],
                 async_top_up_beats_lockstep_off=None if best is None or 1 not in base else best["moves_per_s"] > base[1],
                 async_top_up_beats_lockstep_top_up=None if best is None or 2 not in base else best["moves_per_s"] > base[2],
                 lines=rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
