#!/usr/bin/env python3
"""Same-box A/B of policy surprise weighting (azk_set_surprise_weighting) inside the asynchronous movers at the headline
workload with a replay ring attached: Gomoku 15x15, 2 048 games, 800 simulations, bf16 clsfold evaluator, captured graphs, shared eval
cache of 32 768 entries, and the pre-roll of tools/tree_reuse_ab.py.

    python3 tools/surprise_weighting_ab.py [--out profiles/surprise_weighting_ab.json] [--lam 0.5] [--rounds 2]

Lines: 1 asynchronous off, 2 asynchronous with surprise weighting (lambda), alternated `rounds` times.  One child process per line, one after
the other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per
line: ms per G moves (G = 2 048: ms per 2 048 moves), tuples emitted per finished ply (ring cursor over the plies of the games that
finished), the drain's time per call.  Line 2 then keeps playing, untimed, with the move records switched on, and reports from the kl and
coin of every game it saw from its first ply to its last: the share of plies with no copy and with two or more, the mean and the largest
weight w, and the copies per ply (selfplay.surprise_copies: the emission rule on the host).  The option changes neither searches nor games, so
the two lines are one workload and ms per G moves compares directly.  Then each line runs once more, short, under
`rocprofv3 --kernel-trace --stats` (a run of its own each): the per-launch time of k_move_async and k_emit_*.
"""
import argparse
import json
import sys

import ab_common as ab

# (name, surprise weighting on)
LINES = [("async off", False), ("async surprise weighting", True)]
FORWARDED = ("games", "sims", "size", "lam", "steps", "warmup", "preroll_cheap", "preroll_full", "stat_moves", "cache_entries", "replay_capacity",
             "per_launch", "steps_per_graph", "timer_stride")


def game_statistics(games, lam):
    """games: [(kl array, coin array)] of whole games -> shares, weights and copies over their plies (every ply is a recorded one: no cap)."""
    import numpy as np
    from selfplay import surprise_copies
    ws, cs = [], []
    for kl, coin in games:
        kl, coin = np.asarray(kl, np.float64), np.asarray(coin, np.float64)
        s = 0.0
        for x in kl:
            s += float(x)
        ws.append((1.0 - lam) + ((lam * len(kl)) * kl) / s if s > 0.0 else np.ones(len(kl)))
        cs.append(surprise_copies(kl, coin, lam))
    if not games:
        return dict(games_seen_whole=0)
    w, c = np.concatenate(ws), np.concatenate(cs)
    return dict(games_seen_whole=len(games), plies_seen=int(len(w)), share_plies_no_copy=float((c == 0).mean()), share_plies_two_or_more=float((c >= 2).mean()),
                mean_w=float(w.mean()), max_w=float(w.max()), mean_copies_per_ply=float(c.mean()), max_copies=int(c.max()),
                mean_kl=float(np.concatenate([np.asarray(k) for k, _ in games]).mean()))


def worker(args):
    from selfplay import KernelTimer
    name, on = LINES[args.line - 1]
    kt, replay = KernelTimer(stride=args.timer_stride), ab.device_replay(args)
    # the record ring exists in both lines (the movers write a record per move either way); nobody reads it inside the timed window
    runner = ab.async_runner(args, kt, replay, record_capacity=8 * args.games, surprise_weight=args.lam if on else None)
    drain_events = []
    ab.bracket_calls(runner.eng, "async_drain", drain_events, lambda *a, **k: kt.enabled)
    ab.preroll(runner, args)
    dt, d, c, fields = ab.timed_window(runner, replay, args, args.steps)
    out = dict(fields, line=args.line, name=name, surprise_weight=args.lam if on else None,
               tuples_per_finished_ply=d["tuples"] / max(1, d["plies"]), finished_plies=d["plies"], tuples=d["tuples"], drains=d["drains"],
               **ab.drain_fields(drain_events, dt))
    if on and args.stat_moves > 0:
        # untimed: the records of the next moves, by slot; a game counts once it was seen from the record after a game's end to its own end
        open_games, whole = {}, []

        def on_records(meta, q, pi):
            kl, coin = runner.record_surprise
            for i in range(len(meta)):
                g, ended = int(meta[i, 0]), int(meta[i, 3]) != -2
                if g in open_games:
                    open_games[g][0].append(float(kl[i]))
                    open_games[g][1].append(float(coin[i]))
                    if ended:
                        whole.append(open_games.pop(g))
                if ended:
                    open_games[g] = ([], [])
        runner.finish()
        runner.rec_read = int(runner._seen[6])                # the records of the timed window are not read
        runner.on_records = on_records
        for _ in range(args.stat_moves):
            runner.play_move()
        runner.finish()
        runner.check_error()
        out.update(game_statistics(whole, args.lam))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ab.add_common_args(ap, "line")
    ap.add_argument("--rounds", type=int, default=2, help="off / on pairs, alternated")
    ab.add_common_args(ap, "games", "sims", "size")
    ap.add_argument("--lam", type=float, default=0.5, help="lambda of line 2")
    ab.add_common_args(ap, "steps", "warmup", "preroll_cheap", "preroll_full")
    ap.add_argument("--stat-moves", type=int, default=60, help="line 2: untimed moves per slot whose records give the copy statistics")
    ab.add_common_args(ap, "cache_entries", "replay_capacity", "per_launch", "steps_per_graph", "timer_stride", "timeout")
    ap.add_argument("--trace-steps", type=int, default=4, help="steps of the two traced runs (0: no traced run)")
    ap.add_argument("--trace-timeout", type=int, default=240)
    ap.add_argument("--out", default=ab.out_path("surprise_weighting_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    status, rows = ab.collect_lines(__file__, args, (1, 2), FORWARDED, rounds=args.rounds)
    if status != 0:
        return status
    traced = None
    if args.trace_steps > 0:
        traced = {}
        for line in (1, 2):
            child = ab.child_cmd(__file__, args, "--line", line, FORWARDED, steps=args.trace_steps, warmup=1, preroll_cheap=32, preroll_full=2, stat_moves=0)
            status, kernels = ab.traced_kernels(child, args.trace_timeout, f"traced run of line {line}", ("k_move_async", "k_emit_alloc", "k_emit_tuples", "k_tree"))
            if status != 0:
                return status
            traced[LINES[line - 1][0]] = kernels
            print(json.dumps({LINES[line - 1][0]: kernels}), flush=True)
    summary = {k: dict(off=ab.mean_of(rows, 1, k), on=ab.mean_of(rows, 2, k))
               for k in ("ms_per_G_moves", "tuples_per_finished_ply", "mean_plies_of_finished_games", "k_tree_us_per_launch", "drain_us_per_call",
                         "tree_launches_per_G_moves")}
    for k in ("share_plies_no_copy", "share_plies_two_or_more", "mean_w", "max_w", "mean_copies_per_ply"):
        summary[k] = dict(on=ab.mean_of(rows, 2, k))
    ab.write_doc(args.out, what="policy surprise weighting inside the asynchronous movers at the headline workload with a replay ring attached, one box, one "
                                "process after the other, off and on alternated (tools/surprise_weighting_ab.py); every figure is measured; kernels_traced "
                                "comes from a separate short run of each line under rocprofv3 --kernel-trace --stats; what the option does to the strength "
                                "of a trained network is not measured",
                 lines=rows, mean_of_rounds=summary, kernels_traced=traced)
    return 0


if __name__ == "__main__":
    sys.exit(main())
