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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "alpha-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (name, forced playouts on)
LINES = [("async off", False), ("async forced playouts", True)]


def worker(args):
    import torch
    import azk
    from pvnet import NetConfig, PolicyValueNet
    from selfplay import AsyncSelfPlayRunner, KernelTimer
    name, forced = LINES[args.line - 1]
    torch.cuda.set_device(0)
    A = args.size * args.size
    net = PolicyValueNet(NetConfig(args.size, args.size, 2, A, 5, 512, 8, 1), seed=0, device="cuda:0", dtype=torch.bfloat16, path="clsfold")
    kt = KernelTimer(stride=args.timer_stride)
    replay = azk.DeviceReplay(args.replay_capacity, 2, args.size, args.size, A)
    runner = AsyncSelfPlayRunner("gomoku", net, args.games, args.sims, per_launch=args.per_launch, size=args.size, seed=0, device=0,
                                 leaf_dtype="bfloat16", recycle=True, kernel_timer=kt, cache_entries=args.cache_entries, cache_shared=True,
                                 steps_per_graph=args.steps_per_graph, replay=replay, forced_playouts=args.k if forced else None)
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

    # untimed pre-roll as bench.py's: de-phase the slots with cheap searches, then one game length under the real search
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
    out = dict(line=args.line, name=name, forced_playouts=args.k if forced else 0.0, steps_per_graph=args.steps_per_graph,
               per_launch=args.per_launch, games=args.games, sims=args.sims, size=args.size, steps=args.steps,
               ms_per_G_moves=1e3 * dt * args.games / moves, moves_per_s=d["moves"] / dt,
               games_per_s=d["games"] / dt, mean_plies_of_finished_games=d["plies"] / max(1, d["games"]),
               sims_per_move=c["sims"] / moves,
               tree_launches_per_G_moves=(runner.launches - launches0) * args.games / moves,
               forced_share_of_root_selections=c["forced_selections"] / max(1, c["sims"]),
               pruned_share_of_recorded_visits=c["visits_pruned"] / max(1, c["visits_before_pruning"]),
               recorded_tuples_per_s=d["tuples"] / dt, leaves_evaluated_per_move=c["leaves_evaluated"] / moves,
               cache_hit_share=c["cache_hits"] / max(1, c["sims"]),
               k_tree_us_per_launch=None if tree[0] is None else 1e3 * tree[0], k_tree_samples=tree[2],
               drains=runner.chunks - chunks0,
               drain_us_per_call=1e3 * sum(a.elapsed_time(b) for a, b in drain_events) / max(1, len(drain_events)),
               drain_share_of_time=1e-3 * sum(a.elapsed_time(b) for a, b in drain_events) / dt)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--line", type=int, default=None, help="internal: run one line in this process and print its JSON line")
    ap.add_argument("--lines", default="1,2")
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--k", type=float, default=2.0, help="forced playouts' k of line 2 (KataGo: 2)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll-cheap", type=int, default=128)
    ap.add_argument("--preroll-full", type=int, default=26)
    ap.add_argument("--cache-entries", type=int, default=32768)
    ap.add_argument("--replay-capacity", type=int, default=200000)
    ap.add_argument("--per-launch", type=int, default=1, help="most simulations a game runs inside one tree launch")
    ap.add_argument("--steps-per-graph", type=int, default=32, help="steps between two drains")
    ap.add_argument("--timer-stride", type=int, default=176)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forced_playouts_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    rows = []
    for line in [int(x) for x in args.lines.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--line", str(line)] + [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in
               ("games", "sims", "size", "k", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity",
                "per_launch", "steps_per_graph", "timer_stride")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"line {line}: no result after {args.timeout} s - stopping here", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f"line {line}: exit status {r.returncode} - stopping here\n{r.stderr[-4000:]}", file=sys.stderr)
            return r.returncode
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    doc = dict(what="forced playouts and policy target pruning inside the asynchronous movers at the headline workload, one box, one process after "
                    "the other (tools/forced_playouts_ab.py); every figure is measured, the two shares come from the device counters",
               lines=rows)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
