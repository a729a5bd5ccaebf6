#!/usr/bin/env python3
"""Same-box A/B of evaluation under a position-keyed board symmetry (azk_set_eval_symmetry) inside the asynchronous movers at
the headline workload: Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768
entries, and the pre-roll of tools/tree_reuse_ab.py.

    python3 tools/eval_symmetry_ab.py [--out profiles/eval_symmetry_ab.json] [--rounds 2]

Lines: 1 asynchronous off, 2 asynchronous with eval_symmetry=True, ALTERNATED `--rounds` times (off, on, off, on, ...).  One child process per
line, one after the other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on
the GPU).  Per line: ms per G moves and moves/s, k_tree's mean time per launch (HIP events around sampled eager launches), and from the device
counters leaves evaluated per move and the eval-cache hit share.  Then ONE more child, line 2 for a few steps under
`rocprofv3 --kernel-trace --stats` with a time limit of its own: the per-launch time of the two kernels the option adds (k_sym_leaves,
k_sym_logits) and of k_tree beside them, from the profiler's per-kernel statistics (that run's own timings are not reported: it is traced).
"""
import argparse
import json
import sys

import ab_common as ab

# (name, eval symmetry on)
LINES = [("async off", False), ("async eval symmetry", True)]
FORWARDED = ("games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
             "steps_per_graph", "timer_stride")


def worker(args):
    from selfplay import KernelTimer
    name, sym = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, eval_symmetry=True if sym else None)
    drain_events = []
    ab.bracket_calls(runner.eng, "async_drain", drain_events, lambda *a, **k: kt.enabled)
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    print(json.dumps(dict(fields, line=args.line, name=name, eval_symmetry=bool(sym), recorded_tuples_per_s=d["tuples"] / dt, drains=d["drains"],
                          **ab.leaf_fields(c, max(1, d["moves"])), **ab.drain_fields(drain_events, dt))))


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line", "games", "sims", "size")
    ap.add_argument("--rounds", type=int, default=2, help="how often the pair of lines is run, alternated")
    ap.add_argument("--trace-steps", type=int, default=3, help="timed steps of the traced run (0: no traced run)")
    ap.add_argument("--trace-timeout", type=int, default=300, help="seconds for the traced run")
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("eval_symmetry_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    status, rows = ab.collect_lines(__file__, args, (1, 2), FORWARDED, rounds=args.rounds)
    if status != 0:
        return status
    kernels = None
    if args.trace_steps > 0:
        child = ab.child_cmd(__file__, args, "--line", 2, FORWARDED, steps=args.trace_steps, warmup=1, preroll_cheap=32, preroll_full=2)
        status, kernels = ab.traced_kernels(child, args.trace_timeout, "traced run", ("k_sym_leaves", "k_sym_logits", "k_tree", "k_move_async"))
        if status != 0:
            return status
        print(json.dumps(kernels), flush=True)
    summary = {k: dict(off=ab.mean_of(rows, 1, k), on=ab.mean_of(rows, 2, k))
               for k in ("ms_per_G_moves", "leaves_evaluated_per_move", "cache_hit_share", "k_tree_us_per_launch", "tree_launches_per_G_moves",
                         "mean_plies_of_finished_games")}
    ab.write_doc(args.out, what="evaluation under a position-keyed board symmetry inside the asynchronous movers at the headline workload, one box, one "
                                "process after the other, off and on alternated (tools/eval_symmetry_ab.py); every figure is measured; kernels_traced "
                                "comes from a separate short run of the 'on' line under rocprofv3 --kernel-trace --stats",
                 lines=rows, mean_of_rounds=summary, kernels_traced=kernels)
    return 0


if __name__ == "__main__":
    sys.exit(main())
