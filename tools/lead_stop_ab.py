#!/usr/bin/env python3
"""Same-box A/B of adaptive search budgets' lead rule (azk_set_lead_stop) inside the asynchronous movers at the headline
workload: Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries, plain and
with top-up re-rooting (reroot=2).

    python3 tools/lead_stop_ab.py [--out profiles/lead_stop_ab.json] [--rounds 2] [--interval 100] [--factors 1,1.33,2]

Lines, per mode (plain: 1-4, reroot=2: 5-8): off, then interval --interval at the three factors, run --rounds times, alternated.  Line 9, run
once: plain, the first factor at --short-interval.  Then two children under `rocprofv3 --kernel-trace --stats`, runs of their own (10 plain
off, 11 plain at the first factor), for k_move_async per launch - the kernel the judge lives in.  One child process per line, one after the
other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per timed
line: ms per G moves, mean simulations per search, the share of searches ended early, forced-move ends, leaves evaluated per move, the
cache-hit share, the plies of finished games.  Every line's pre-roll runs at its own budget (the option fixes n_sims for the run).  The lines
are DIFFERENT searches - a search that ends early moves on fewer visits, and these moves are sampled from them for the first plies of a game -
except where moves are greedy: there factor 1 plays the option-off move.  So the figures are descriptions: no target is set for them.  What
any factor does to the strength of a trained network is not measured here.
"""
import argparse
import json
import sys

import ab_common as ab

MODES = [("async", 0), ("async reroot=2", 2)]
SHORT = 9
TRACED = {10: "off", 11: "first factor"}


def line_setting(args, line):
    """(name, reroot, lead_stop) of a timed line: four lines per mode - off and the three factors - and the short-interval line."""
    factors = [float(x) for x in args.factors.split(",")]
    if line == SHORT:
        return f"async I={args.short_interval} f={factors[0]:g}", 0, (args.short_interval, factors[0], args.min_sims)
    mode, k = divmod(line - 1, 4)
    name, reroot = MODES[mode]
    if k == 0:
        return name + " off", reroot, None
    return f"{name} I={args.interval} f={factors[k - 1]:g}", reroot, (args.interval, factors[k - 1], args.min_sims)


def runner_for(args, kt, replay, reroot, lead):
    opts = dict(lead_stop=lead)
    if reroot:
        opts.update(reroot=reroot, arena_nodes=args.arena_nodes)
    return ab.async_runner(args, kt, replay, **opts)


def worker(args):
    from selfplay import KernelTimer
    name, reroot, lead = line_setting(args, args.line)
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    runner = runner_for(args, kt, replay, reroot, lead)
    ab.preroll(runner, args, cheap=False)
    before = runner.lead_stats() if lead else None
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    extra = dict(share_ended_early=None, share_forced=None, sims_unrun_per_search=None)
    if lead:
        after = runner.lead_stats()
        diff = {k: after[k] - before[k] for k in after}
        over = max(1, diff["ended_early"] + diff["forced"] + diff["ran_allowance"])
        extra = dict(share_ended_early=diff["ended_early"] / over, share_forced=diff["forced"] / over, sims_unrun_per_search=diff["sims_unrun"] / over)
    print(json.dumps(dict(fields, line=args.line, name=name, reroot=reroot, lead_stop=lead, **extra, **ab.leaf_fields(c, max(1, d["moves"])))))


def traced(args):
    """A short run for the profiler."""
    from selfplay import KernelTimer
    factors = [float(x) for x in args.factors.split(",")]
    lead = None if TRACED[args.line] == "off" else (args.interval, factors[0], args.min_sims)
    runner = runner_for(args, KernelTimer(stride=args.timer_stride), ab.device_replay(args), 0, lead)
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
    ap.add_argument("--short-interval", type=int, default=25)
    ap.add_argument("--min-sims", type=int, default=0)
    ap.add_argument("--factors", default="1,1.33,2", help="three factors, comma separated")
    ap.add_argument("--arena-nodes", type=int, default=0, help="reroot lines: nodes per game (0: the engine's default)")
    ap.add_argument("--no-trace", action="store_true", help="leave the two profiler runs out")
    ab.add_common_args(ap, "games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
                       "steps_per_graph", "timer_stride", "timeout")
    ap.add_argument("--out", default=ab.out_path("lead_stop_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return traced(args) if args.line in TRACED else worker(args)
    forwarded = ["games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
                 "steps_per_graph", "timer_stride", "interval", "short_interval", "min_sims", "arena_nodes", "factors"]
    lines = list(range(1, 4 * len(MODES) + 1))
    status, rows = ab.collect_lines(__file__, args, lines, forwarded, rounds=args.rounds)
    if status != 0:
        return status
    status, short = ab.collect_lines(__file__, args, [SHORT], forwarded)
    if status != 0:
        return status
    kernels = {}
    for line in ([] if args.no_trace else sorted(TRACED)):
        status, kernels[f"async {TRACED[line]}"] = ab.traced_kernels(ab.child_cmd(__file__, args, "--line", line, forwarded), 2 * args.timeout,
                                                                     f"kernel trace {line}", ("k_move_async", "k_tree", "k_kld_arm"))
        if status != 0:
            return status
    keys = ("ms_per_G_moves", "sims_per_move", "share_ended_early", "share_forced", "leaves_evaluated_per_move", "cache_hit_share",
            "mean_plies_of_finished_games", "k_tree_us_per_launch")
    summary = {line_setting(args, i)[0]: {k: ab.mean_of(rows, i, k) for k in keys} for i in lines}
    ab.write_doc(args.out, what="adaptive search budgets' lead rule inside the asynchronous movers at the headline workload, plain and with top-up "
                 "re-rooting, one box, one process after the other, the lines alternated (tools/lead_stop_ab.py); the lines are different searches "
                 "except where moves are greedy, and are described, not priced against each other; every pre-roll runs at the line's own budget; "
                 "the kernel times come from rocprofv3 --kernel-trace --stats runs of their own; the strength of a network trained under the rule "
                 "is not measured", factors=args.factors, lines=rows, short_interval_line=short, means=summary, kernels_us_per_launch=kernels)
    print(json.dumps(dict(means=summary, short=short, kernels=kernels)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
