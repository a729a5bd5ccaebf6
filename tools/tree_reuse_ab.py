#!/usr/bin/env python3
"""Same-box A/B of tree reuse across moves (azk_config.tree_reuse) at the headline workload: SelfPlayRunner, Gomoku 15x15, 2 048 games,
800 simulations, bf16 evaluator, captured-graph runner, shared eval cache - with tree_reuse 0 (off), 1 (carry) and 2 (top-up).

    python3 tools/tree_reuse_ab.py [--out profiles/tree_reuse_ab.json]

One child process per mode, one after the other on the same GPU, each under its own time limit; the first one that fails ends the
run (nothing more is started on the GPU).  Per mode: ms per move, simulations and tree launches per move, games/s, the time of the
search-begin kernel (k_begin_search, or k_reroot on a reuse engine) per call from HIP events around its launch, k_tree's mean time per
launch (HIP events around sampled eager launches, as bench.py's kernel timer), the share of roots reused, the mean nodes carried per
re-root and the mean root visits a search starts with.  bench.py and its headline stay the reuse-off configuration.
"""
import argparse
import json
import sys
import time

import ab_common as ab


def worker(args):
    import torch
    from selfplay import KernelTimer, SelfPlayRunner
    net = ab.headline_net(args)
    kt = KernelTimer(stride=args.timer_stride)
    runner = SelfPlayRunner("gomoku", net, args.games, args.sims, use_graph=True, n_split=1, tree_reuse=args.mode,
                            **ab.headline_options(args, kt, steps_per_graph=32))
    eng = runner.eng
    begin_events = []
    for method in ("begin_search", "begin_search_budget"):
        ab.bracket_calls(eng, method, begin_events, lambda *a, **k: kt.enabled)
    ab.preroll(runner, args)
    runner.reset_counters()
    fin0, finp0, launches0 = runner.games_finished, runner.finished_plies, runner.launches
    start_visits = []
    kt.enabled = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        runner.play_move()
        start_visits.append(eng.root_visit.clone())           # root visits at the END of the move's search (azk_root_stats)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kt.enabled = False
    runner.check_error()
    c = runner.counters()
    moves = c["moves_played"]
    fin, finp = runner.games_finished - fin0, runner.finished_plies - finp0
    tree = kt.robust_mean_ms()
    sims_per_move = c["sims"] / max(1, moves)
    end_visit = float(torch.stack(start_visits).double().mean().item())
    out = dict(tree_reuse=args.mode, games=args.games, sims=args.sims, size=args.size, steps=args.steps,
               ms_per_move=1e3 * dt / args.steps, moves_per_s=moves / dt, games_per_s=fin / dt,
               mean_plies_of_finished_games=finp / max(1, fin),
               sims_per_move=sims_per_move, tree_launches_per_move=(runner.launches - launches0) / args.steps,
               begin_kernel_us_per_call=1e3 * ab.events_ms(begin_events) / max(1, len(begin_events)),
               begin_kernel_calls=len(begin_events),
               k_tree_us_per_launch=None if tree[0] is None else 1e3 * tree[0], k_tree_samples=tree[2],
               roots_reused_share=c["roots_reused"] / max(1, moves), nodes_carried_per_reroot=c["nodes_carried"] / max(1, c["roots_reused"]),
               root_visits_at_end_of_search=end_visit, root_visits_carried_per_move=end_visit - sims_per_move, **ab.leaf_fields(c, moves))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=int, default=None, help="internal: run one mode in this process and print its JSON line")
    ap.add_argument("--modes", default="0,1,2")
    ab.add_common_args(ap, "games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "timer_stride", "timeout",
                       help=dict(timeout="seconds per mode"))
    ap.add_argument("--out", default=ab.out_path("tree_reuse_ab.json"))
    args = ap.parse_args()
    if args.mode is not None:
        return worker(args)
    status, rows = ab.collect_lines(__file__, args, [int(x) for x in args.modes.split(",")],
                                    ("games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "timer_stride"),
                                    flag="--mode")
    if status == 0:
        ab.write_doc(args.out, what="SelfPlayRunner at the headline workload with tree_reuse 0 / 1 / 2, one box, one process after the other "
                                    "(tools/tree_reuse_ab.py)", modes=rows)
    return status


if __name__ == "__main__":
    sys.exit(main())
