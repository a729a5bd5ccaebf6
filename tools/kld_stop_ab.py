#!/usr/bin/env python3
"""Same-box A/B of adaptive search budgets (azk_set_kld_stop) inside the asynchronous movers at the headline workload:
Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries, plain and with
top-up re-rooting (reroot=2).

    python3 tools/kld_stop_ab.py [--out profiles/kld_stop_ab.json] [--rounds 2] [--interval 100] [--gains 1e-5,1e-4,1e-3]

First a child that DESCRIBES the rates (line 0): the movers run with a threshold that never fires and the last judged rate of every game is
read after each of --describe-moves moves per slot; the deciles are printed.  Without --gains the three thresholds are then taken a decade
apart around the decade of the median rate.  Lines, per mode (plain: 1-4, reroot=2: 5-8): off, then interval --interval at the three
thresholds, run --rounds times, alternated.  Then two children under `rocprofv3 --kernel-trace --stats`, runs of their own (9 plain off, 10
plain at the middle threshold), for k_move_async per launch - the kernel the judge lives in.  One child process per line, one after the other
on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per timed line: ms
per G moves, mean simulations per search, the share of searches ended early, leaves evaluated per move, the cache-hit share, the plies of
finished games.  Every line's pre-roll runs at its own budget (the option fixes n_sims for the run).  The lines are DIFFERENT searches - a
search that ends early moves on fewer visits - so their figures are descriptions: no target is set for them.  What the rule does to the
strength of a trained network is not measured here.
"""
import argparse
import json
import math
import sys

import ab_common as ab

NEVER = 1e-300
MODES = [("async", 0), ("async reroot=2", 2)]
TRACED = {9: "off", 10: "middle"}


def line_setting(args, line):
    """(name, reroot, kld_stop) of a timed line: four lines per mode - off and the three thresholds."""
    mode, k = divmod(line - 1, 4)
    name, reroot = MODES[mode]
    gains = [float(x) for x in args.gains.split(",")]
    if k == 0:
        return name + " off", reroot, None
    return f"{name} I={args.interval} gain={gains[k - 1]:g}", reroot, (args.interval, gains[k - 1], args.min_sims)


def runner_for(args, kt, replay, reroot, kld):
    opts = dict(kld_stop=kld)
    if reroot:
        opts.update(reroot=reroot, arena_nodes=args.arena_nodes)
    return ab.async_runner(args, kt, replay, **opts)


def worker(args):
    from selfplay import KernelTimer
    name, reroot, kld = line_setting(args, args.line)
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = runner_for(args, kt, replay, reroot, kld)
    ab.preroll(runner, args, cheap=False)
    before = runner.kld_stats() if kld else None
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    extra = dict(share_ended_early=None, sims_unrun_per_search=None)
    if kld:
        after = runner.kld_stats()
        over = (after["ended_early"] - before["ended_early"]) + (after["ran_allowance"] - before["ran_allowance"])
        extra = dict(share_ended_early=(after["ended_early"] - before["ended_early"]) / max(1, over),
                     sims_unrun_per_search=(after["sims_unrun"] - before["sims_unrun"]) / max(1, over))
    print(json.dumps(dict(fields, line=args.line, name=name, reroot=reroot, kld_stop=kld, **extra, **ab.leaf_fields(c, max(1, d["moves"])))))


def describe(args):
    """The rate distribution: a threshold that never fires, the games' last judged rates after every move."""
    import numpy as np
    from selfplay import KernelTimer
    runner = runner_for(args, KernelTimer(stride=args.timer_stride), None, 0, (args.interval, NEVER, 0))
    rates = []
    for _ in range(args.describe_moves):
        runner.play_move()
        runner.finish()
        r = runner.eng.kld_rate().cpu().numpy()
        rates.extend(r[r > 0.0].tolist())
    runner.check_error()
    q = np.quantile(np.asarray(rates), [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]).tolist()
    print(json.dumps(dict(line=0, name="rates, threshold never fires", interval=args.interval, rates_read=len(rates), deciles=q, median=q[4],
                          note="the last judged rate of every game after each move: late checkpoints of long searches weigh most")))


def traced(args):
    """A short run for the profiler."""
    from selfplay import KernelTimer
    gains = [float(x) for x in args.gains.split(",")]
    kld = None if TRACED[args.line] == "off" else (args.interval, gains[1], args.min_sims)
    runner = runner_for(args, KernelTimer(stride=args.timer_stride), ab.device_replay(args), 0, kld)
    ab.preroll(runner, args, cheap=False)
    for _ in range(args.steps):
        runner.play_move()
    runner.finish()
    runner.check_error()


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--interval", type=int, default=100)
    ap.add_argument("--min-sims", type=int, default=0)
    ap.add_argument("--gains", default="", help="three thresholds, comma separated; default: a decade apart around the decade of the median rate")
    ap.add_argument("--describe-moves", type=int, default=4, help="moves per slot of the describing child")
    ap.add_argument("--arena-nodes", type=int, default=0, help="reroot lines: nodes per game (0: the engine's default)")
    ap.add_argument("--no-trace", action="store_true", help="leave the two profiler runs out")
    ab.add_common_args(ap, "games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
                       "steps_per_graph", "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("kld_stop_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return traced(args) if args.line in TRACED else describe(args) if args.line == 0 else worker(args)
    forwarded = ["games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
                 "steps_per_graph", "timer_stride", "interval", "min_sims", "describe_moves", "arena_nodes"]
    status, described = ab.collect_lines(__file__, args, [0], forwarded)
    if status != 0:
        return status
    if not args.gains:
        mid = 10.0 ** round(math.log10(described[0]["median"]))
        args.gains = ",".join(f"{g:g}" for g in (mid / 10.0, mid, mid * 10.0))
    forwarded.append("gains")
    lines = list(range(1, 4 * len(MODES) + 1))
    status, rows = ab.collect_lines(__file__, args, lines, forwarded, rounds=args.rounds)
    if status != 0:
        return status
    kernels = {}
    for line in ([] if args.no_trace else sorted(TRACED)):
        status, kernels[f"async {TRACED[line]}"] = ab.traced_kernels(ab.child_cmd(__file__, args, "--line", line, forwarded), 2 * args.timeout,
                                                                     f"kernel trace {line}", ("k_move_async", "k_tree", "k_kld_arm"))
        if status != 0:
            return status
    keys = ("ms_per_G_moves", "sims_per_move", "share_ended_early", "leaves_evaluated_per_move", "cache_hit_share", "mean_plies_of_finished_games",
            "k_tree_us_per_launch")
    summary = {line_setting(args, i)[0]: {k: ab.mean_of(rows, i, k) for k in keys} for i in lines}
    ab.write_doc(args.out, what="adaptive search budgets inside the asynchronous movers at the headline workload, plain and with top-up re-rooting, one "
                 "box, one process after the other, the lines alternated (tools/kld_stop_ab.py); the thresholds were taken from the described rate "
                 "distribution; the lines are different searches and are described, not priced against each other; every pre-roll runs at the "
                 "line's own budget; the kernel times come from rocprofv3 --kernel-trace --stats runs of their own; the strength of a network "
                 "trained under the rule is not measured", rates=described, gains=args.gains, lines=rows, means=summary, kernels_us_per_launch=kernels)
    print(json.dumps(dict(rates=described, means=summary, kernels=kernels)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
