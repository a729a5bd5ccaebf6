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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "alpha-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (name, surprise weighting on)
LINES = [("async off", False), ("async surprise weighting", True)]


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
    import torch
    import azk
    from pvnet import NetConfig, PolicyValueNet
    from selfplay import AsyncSelfPlayRunner, KernelTimer
    name, on = LINES[args.line - 1]
    torch.cuda.set_device(0)
    A = args.size * args.size
    net = PolicyValueNet(NetConfig(args.size, args.size, 2, A, 5, 512, 8, 1), seed=0, device="cuda:0", dtype=torch.bfloat16, path="clsfold")
    kt = KernelTimer(stride=args.timer_stride)
    replay = azk.DeviceReplay(args.replay_capacity, 2, args.size, args.size, A)
    # the record ring exists in both lines (the movers write a record per move either way); nobody reads it inside the timed window
    runner = AsyncSelfPlayRunner("gomoku", net, args.games, args.sims, per_launch=args.per_launch, size=args.size, seed=0, device=0,
                                 leaf_dtype="bfloat16", recycle=True, kernel_timer=kt, cache_entries=args.cache_entries, cache_shared=True,
                                 steps_per_graph=args.steps_per_graph, replay=replay, record_capacity=8 * args.games,
                                 surprise_weight=args.lam if on else None)
    drain_events = []
    eng, plain_drain = runner.eng, runner.eng.async_drain

    def timed_drain(*a, **k):
        if not kt.enabled:
            return plain_drain(*a, **k)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = plain_drain(*a, **k)
        e.record()
        drain_events.append((s, e))
        return r
    eng.async_drain = timed_drain

    def totals():
        st = runner.finish()
        return dict(moves=int(st[5]), games=int(st[0]), plies=int(st[1]), searches=int(st[7]), tuples=int(replay.cursor.item()))

    full = runner.n_sims
    runner.n_sims = 16
    for _ in range(args.preroll_cheap):
        runner.play_move()
    runner.n_sims = full
    for _ in range(args.preroll_full + args.warmup):
        runner.play_move()
    t_a = totals()
    runner.reset_counters()
    launches0, chunks0 = runner.launches, runner.chunks
    kt.enabled = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        runner.play_move()
    t_b = totals()                                            # (waits for everything enqueued)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kt.enabled = False
    runner.check_error()
    c = runner.counters()
    d = {k: t_b[k] - t_a[k] for k in t_a}
    moves = max(1, d["moves"])
    tree = kt.robust_mean_ms()
    out = dict(line=args.line, name=name, surprise_weight=args.lam if on else None, steps_per_graph=args.steps_per_graph,
               per_launch=args.per_launch, games=args.games, sims=args.sims, size=args.size, steps=args.steps,
               ms_per_G_moves=1e3 * dt * args.games / moves, moves_per_s=d["moves"] / dt,
               games_per_s=d["games"] / dt, mean_plies_of_finished_games=d["plies"] / max(1, d["games"]),
               tuples_per_finished_ply=d["tuples"] / max(1, d["plies"]), finished_plies=d["plies"], tuples=d["tuples"],
               sims_per_move=c["sims"] / moves, tree_launches_per_G_moves=(runner.launches - launches0) * args.games / moves,
               k_tree_us_per_launch=None if tree[0] is None else 1e3 * tree[0], k_tree_samples=tree[2],
               drains=runner.chunks - chunks0,
               drain_us_per_call=1e3 * sum(a.elapsed_time(b) for a, b in drain_events) / max(1, len(drain_events)),
               drain_share_of_time=1e-3 * sum(a.elapsed_time(b) for a, b in drain_events) / dt)
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
    ap.add_argument("--line", type=int, default=None, help="internal: run one line in this process and print its JSON line")
    ap.add_argument("--rounds", type=int, default=2, help="off / on pairs, alternated")
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--lam", type=float, default=0.5, help="lambda of line 2")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll-cheap", type=int, default=128)
    ap.add_argument("--preroll-full", type=int, default=26)
    ap.add_argument("--stat-moves", type=int, default=60, help="line 2: untimed moves per slot whose records give the copy statistics")
    ap.add_argument("--cache-entries", type=int, default=32768)
    ap.add_argument("--replay-capacity", type=int, default=200000)
    ap.add_argument("--per-launch", type=int, default=1, help="most simulations a game runs inside one tree launch")
    ap.add_argument("--steps-per-graph", type=int, default=32, help="steps between two drains")
    ap.add_argument("--timer-stride", type=int, default=176)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per line")
    ap.add_argument("--trace-steps", type=int, default=4, help="steps of the two traced runs (0: no traced run)")
    ap.add_argument("--trace-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surprise_weighting_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    keys = ("games", "sims", "size", "lam", "steps", "warmup", "preroll_cheap", "preroll_full", "stat_moves", "cache_entries", "replay_capacity",
            "per_launch", "steps_per_graph", "timer_stride")

    def child(line, **over):
        return [sys.executable, os.path.abspath(__file__), "--line", str(line)] + [f"--{k.replace('_', '-')}={over.get(k, getattr(args, k))}" for k in keys]
    rows = []
    for rnd in range(args.rounds):
        for line in (1, 2):
            try:
                r = subprocess.run(child(line), capture_output=True, text=True, timeout=args.timeout)
            except subprocess.TimeoutExpired:
                print(f"round {rnd} line {line}: no result after {args.timeout} s - stopping here", file=sys.stderr)
                return 124
            if r.returncode != 0:
                print(f"round {rnd} line {line}: exit status {r.returncode} - stopping here\n{r.stderr[-4000:]}", file=sys.stderr)
                return r.returncode
            rows.append(dict(json.loads(r.stdout.strip().splitlines()[-1]), round=rnd))
            print(json.dumps(rows[-1]), flush=True)
    traced = None
    if args.trace_steps > 0:
        import csv
        import glob
        import tempfile
        traced = {}
        for line in (1, 2):
            with tempfile.TemporaryDirectory() as d:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + child(
                    line, steps=args.trace_steps, warmup=1, preroll_cheap=32, preroll_full=2, stat_moves=0)
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.trace_timeout)
                except subprocess.TimeoutExpired:
                    print(f"traced run of line {line}: no result after {args.trace_timeout} s - stopping here", file=sys.stderr)
                    return 124
                if r.returncode != 0:
                    print(f"traced run of line {line}: exit status {r.returncode}\n{r.stderr[-4000:]}", file=sys.stderr)
                    return r.returncode
                files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
                kernels = {}
                for row in (csv.DictReader(open(files[0])) if files else []):
                    for want in ("k_move_async", "k_emit_alloc", "k_emit_tuples", "k_tree"):
                        if want in row["Name"]:
                            k = kernels.setdefault(want, dict(calls=0, total_ns=0.0))
                            k["calls"] += int(row["Calls"])
                            k["total_ns"] += float(row["TotalDurationNs"])
                for k in kernels.values():
                    k["us_per_launch"] = 1e-3 * k.pop("total_ns") / max(1, k["calls"])
                traced[LINES[line - 1][0]] = kernels
                print(json.dumps({LINES[line - 1][0]: kernels}), flush=True)

    def mean(line, key):
        v = [r[key] for r in rows if r["line"] == line and r.get(key) is not None]
        return sum(v) / len(v) if v else None
    summary = {k: dict(off=mean(1, k), on=mean(2, k)) for k in ("ms_per_G_moves", "tuples_per_finished_ply", "mean_plies_of_finished_games", "k_tree_us_per_launch",
                                                               "drain_us_per_call", "tree_launches_per_G_moves")}
    for k in ("share_plies_no_copy", "share_plies_two_or_more", "mean_w", "max_w", "mean_copies_per_ply"):
        summary[k] = dict(on=mean(2, k))
    doc = dict(what="policy surprise weighting inside the asynchronous movers at the headline workload with a replay ring attached, one box, one process after "
                    "the other, off and on alternated (tools/surprise_weighting_ab.py); every figure is measured; kernels_traced comes from a separate short "
                    "run of each line under rocprofv3 --kernel-trace --stats; what the option does to the strength of a trained network is not measured",
               lines=rows, mean_of_rounds=summary, kernels_traced=traced)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
