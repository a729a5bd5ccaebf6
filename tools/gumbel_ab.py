#!/usr/bin/env python3
"""Same-box report of the Gumbel root search (azk_set_gumbel_root) inside the asynchronous movers at the headline workload:
Gomoku 15x15, 2 048 games, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries.

    python3 tools/gumbel_ab.py [--out profiles/gumbel_root_ab.json] [--m 16 --c-visit 50 --c-scale 1]

Lines: 1 option off at 800 simulations, 2 option off at 64, 3 Gumbel root (m, c_visit, c_scale) at 64.  One child process per line, one after
the other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per
line: ms per G moves, k_tree's and k_move_async's mean time per launch (HIP events around sampled eager launches), the drain's time per call,
the movers' share of the wall time (k_move_async in every step + the drains), and leaves evaluated per move from the device counters.  A
Gumbel search's budget is fixed (its halving table is built for it), so the 64-simulation lines run their pre-roll at 64 simulations; line 1
has the cheap pre-roll of the other tools.  Nothing here has a bar: the option changes the search, so the lines are not one workload.
"""
import argparse
import json
import sys

import ab_common as ab

# (name, simulations: "long" | "short", Gumbel root on)
LINES = [("off, long search", "long", False), ("off, short search", "short", False), ("gumbel root, short search", "short", True)]


def worker(args):
    from selfplay import KernelTimer
    name, kind, gumbel = LINES[args.line - 1]
    sims = args.sims if kind == "long" else args.sims_short
    steps = args.steps if kind == "long" else args.steps_short
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, sims=sims, gumbel_root=(args.m, args.c_visit, args.c_scale) if gumbel else None)
    drain_events, movers = [], KernelTimer()                    # (movers: a store for the pairs, and robust_mean_ms over them)
    ab.bracket_calls(runner.eng, "async_drain", drain_events, lambda *a, **k: kt.enabled)
    # phases == 2 alone: the movers of a sampled eager step
    ab.bracket_calls(runner.eng, "async_step", movers.pairs, lambda logits, values, phases=3: kt.enabled and phases == 2)
    # line 1: the cheap pre-roll of the other tools; a short search is cheap (and a Gumbel budget fixed): the whole pre-roll at its own budget
    ab.preroll(runner, args, cheap=kind == "long")
    dt, d, c, fields = ab.timed_window(runner, replay, args, steps)
    mover_ms, _, mover_samples = movers.robust_mean_ms()
    mover_us = None if mover_ms is None else 1e3 * mover_ms
    drain_s = 1e-3 * ab.events_ms(drain_events)
    print(json.dumps(dict(fields, line=args.line, name=name, gumbel_root=[args.m, args.c_visit, args.c_scale] if gumbel else None,
                          recorded_tuples_per_s=d["tuples"] / dt, k_move_async_us_per_launch=mover_us, k_move_async_samples=mover_samples,
                          drains=d["drains"], drain_us_per_call=1e6 * drain_s / max(1, len(drain_events)),
                          movers_share_of_time=None if mover_us is None else (1e-6 * mover_us * d["launches"] + drain_s) / dt,
                          **ab.leaf_fields(c, max(1, d["moves"])))))


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line")
    ap.add_argument("--lines", default="1,2,3")
    ab.add_common_args(ap, "games", "sims", help=dict(sims="simulations of line 1"))
    ap.add_argument("--sims-short", type=int, default=64, help="simulations of lines 2 and 3")
    ab.add_common_args(ap, "size")
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--c-visit", type=float, default=50.0)
    ap.add_argument("--c-scale", type=float, default=1.0)
    ab.add_common_args(ap, "steps", help=dict(steps="timed moves per slot of line 1"))
    ap.add_argument("--steps-short", type=int, default=200, help="timed moves per slot of lines 2 and 3")
    ab.add_common_args(ap, "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout", timer_stride=64)
    ap.add_argument("--out", default=ab.out_path("gumbel_root_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    return ab.run_lines(__file__, args, [int(x) for x in args.lines.split(",")],
                        ("games", "sims", "sims_short", "size", "m", "c_visit", "c_scale", "steps", "steps_short", "warmup", "preroll_cheap",
                         "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph", "timer_stride"),
                        "Gumbel root search inside the asynchronous movers at the headline workload, one box, one process after the other "
                        "(tools/gumbel_ab.py); every figure is measured; the strength of a network trained on these targets is not",
                        args.out)


if __name__ == "__main__":
    sys.exit(main())
