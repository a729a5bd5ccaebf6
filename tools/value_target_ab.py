#!/usr/bin/env python3
"""Same-box A/B of value targets (azk_set_value_target) inside the asynchronous movers at the headline workload with a
replay ring attached: Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768
entries, and the pre-roll of tools/tree_reuse_ab.py.

    python3 tools/value_target_ab.py [--out profiles/value_target_ab.json] [--r 0.5] [--lam 0.9] [--rounds 2] [--no-trace]

Lines: 1 asynchronous off, 2 asynchronous with value targets (r, lam), alternated `rounds` times.  One child process per line, one after the
other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per line: ms
per G moves (G = 2 048: ms per 2 048 moves), tuples emitted per finished ply, the drain's time per call, and over the ring as the timed window
left it the mean and the largest |z| and the share of rows whose z is not +-1 or 0 (off: none).  The option changes neither searches nor games,
so the two lines are one workload and ms per G moves compares directly.  Then each line runs once more, short, under
`rocprofv3 --kernel-trace --stats` (a run of its own each): the per-launch time of k_move_async, k_emit_alloc and k_emit_tuples.  There is no
speed bar.  What the targets do to the strength of a trained network is not measured here.
"""
import argparse
import json
import sys

import ab_common as ab

# (name, value targets on)
LINES = [("async off", False), ("async value targets", True)]
FORWARDED = ("games", "sims", "size", "r", "lam", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
             "steps_per_graph", "timer_stride")


def ring_fields(replay):
    z = replay.zs[:replay.size()].double()
    if z.numel() == 0:
        return dict(ring_rows=0)
    soft = ((z != 0.0) & (z.abs() != 1.0)).double().mean()
    return dict(ring_rows=int(z.numel()), ring_mean_abs_z=float(z.abs().mean()), ring_max_abs_z=float(z.abs().max()), ring_share_soft_z=float(soft))


def worker(args):
    from selfplay import KernelTimer
    name, on = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = ab.async_runner(args, kt, replay, value_target=(args.r, args.lam) if on else None)
    drain_events = []
    ab.bracket_calls(runner.eng, "async_drain", drain_events, lambda *a, **k: kt.enabled)
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    print(json.dumps(dict(fields, line=args.line, name=name, value_target=[args.r, args.lam] if on else None,
                          tuples_per_finished_ply=d["tuples"] / max(1, d["plies"]), finished_plies=d["plies"], tuples=d["tuples"], drains=d["drains"],
                          **ab.drain_fields(drain_events, dt), **ring_fields(replay))))


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line")
    ap.add_argument("--rounds", type=int, default=2, help="off / on pairs, alternated")
    ab.add_common_args(ap, "games", "sims", "size")
    ap.add_argument("--r", type=float, default=0.5, help="weight of the search-based part in line 2")
    ap.add_argument("--lam", type=float, default=0.9, help="its horizon")
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch", "steps_per_graph",
                       "timer_stride", "timeout")
    ap.add_argument("--no-trace", action="store_true", help="leave the two profiler runs out")
    ap.add_argument("--trace-steps", type=int, default=4, help="steps of the two traced runs")
    ap.add_argument("--trace-timeout", type=int, default=240)
    ap.add_argument("--out", default=ab.out_path("value_target_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    status, rows = ab.collect_lines(__file__, args, (1, 2), FORWARDED, rounds=args.rounds)
    if status != 0:
        return status
    traced = None
    if not args.no_trace and args.trace_steps > 0:
        traced = {}
        for line in (1, 2):
            child = ab.child_cmd(__file__, args, "--line", line, FORWARDED, steps=args.trace_steps, warmup=1, preroll_cheap=32, preroll_full=2)
            status, kernels = ab.traced_kernels(child, args.trace_timeout, f"traced run of line {line}", ("k_move_async", "k_emit_alloc", "k_emit_tuples"))
            if status != 0:
                return status
            traced[LINES[line - 1][0]] = kernels
            print(json.dumps({LINES[line - 1][0]: kernels}), flush=True)
    summary = {k: dict(off=ab.mean_of(rows, 1, k), on=ab.mean_of(rows, 2, k))
               for k in ("ms_per_G_moves", "tuples_per_finished_ply", "mean_plies_of_finished_games", "drain_us_per_call", "ring_mean_abs_z",
                         "ring_share_soft_z")}
    ab.write_doc(args.out, what="value targets inside the asynchronous movers at the headline workload with a replay ring attached, one box, one process "
                                "after the other, off and on alternated (tools/value_target_ab.py); every figure is measured; kernels_traced comes from a "
                                "separate short run of each line under rocprofv3 --kernel-trace --stats; what the targets do to the strength of a trained "
                                "network is not measured",
                 lines=rows, mean_of_rounds=summary, kernels_traced=traced)
    print(json.dumps(dict(mean_of_rounds=summary, kernels_traced=traced)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
