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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "alpha-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (name, asynchronous, tree reuse mode, steps per graph)
LINES = [("lock-step off", False, 0, 32), ("lock-step top-up", False, 2, 32), ("async off", True, 0, 32),
         ("async top-up spg 8", True, 2, 8), ("async top-up spg 16", True, 2, 16), ("async top-up spg 32", True, 2, 32),
         ("async carry spg 32", True, 1, 32)]


def worker(args):
    import torch
    from pvnet import NetConfig, PolicyValueNet
    from selfplay import AsyncSelfPlayRunner, KernelTimer, SelfPlayRunner
    name, is_async, mode, spg = LINES[args.line - 1]
    torch.cuda.set_device(0)
    A = args.size * args.size
    net = PolicyValueNet(NetConfig(args.size, args.size, 2, A, 5, 512, 8, 1), seed=0, device="cuda:0", dtype=torch.bfloat16, path="clsfold")
    kt = KernelTimer(stride=args.timer_stride)
    common = dict(size=args.size, seed=0, device=0, leaf_dtype="bfloat16", recycle=True, kernel_timer=kt, cache_entries=args.cache_entries,
                  cache_shared=True, steps_per_graph=spg)
    drain_events = []
    if is_async:
        runner = AsyncSelfPlayRunner("gomoku", net, args.games, args.sims, per_launch=args.per_launch, reroot=mode, **common)
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
    else:
        runner = SelfPlayRunner("gomoku", net, args.games, args.sims, use_graph=True, n_split=1, tree_reuse=mode, **common)

    def totals():
        if is_async:
            st = runner.finish()
            return dict(moves=int(st[5]), games=int(st[0]), plies=int(st[1]), searches=int(st[7]))
        return dict(moves=runner.plies_played, games=runner.games_finished, plies=runner.finished_plies, searches=0)

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
    launches0, chunks0 = runner.launches, getattr(runner, "chunks", 0)
    kt.enabled = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        runner.play_move()
    t_b = totals()                                            # (asynchronous: waits for everything enqueued)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kt.enabled = False
    runner.check_error()
    c = runner.counters()
    moves, fin, finp = t_b["moves"] - t_a["moves"], t_b["games"] - t_a["games"], t_b["plies"] - t_a["plies"]
    tree = kt.robust_mean_ms()
    out = dict(line=args.line, name=name, asynchronous=is_async, tree_reuse=mode, steps_per_graph=spg, per_launch=args.per_launch if is_async else None,
               games=args.games, sims=args.sims, size=args.size, steps=args.steps,
               ms_per_G_moves=1e3 * dt * args.games / max(1, moves), moves_per_s=moves / dt,
               sims_per_move=c["sims"] / max(1, moves), tree_launches_per_G_moves=(runner.launches - launches0) * args.games / max(1, moves),
               leaves_evaluated_per_move=c["leaves_evaluated"] / max(1, moves), cache_hit_share=c["cache_hits"] / max(1, c["sims"]),
               roots_reused_share=c["roots_reused"] / max(1, moves), nodes_carried_per_reroot=c["nodes_carried"] / max(1, c["roots_reused"]),
               games_per_s=fin / dt, mean_plies_of_finished_games=finp / max(1, fin),
               k_tree_us_per_launch=None if tree[0] is None else 1e3 * tree[0], k_tree_samples=tree[2])
    if is_async:
        drains = runner.chunks - chunks0
        out.update(drains=drains, drain_us_per_call=1e3 * sum(a.elapsed_time(b) for a, b in drain_events) / max(1, len(drain_events)),
                   drain_share_of_time=1e-3 * sum(a.elapsed_time(b) for a, b in drain_events) / dt,
                   # searches begun = re-roots (carried or fallback) + restarts of finished games; engines without reuse begin them in the move kernel
                   games_rerooted_per_drain=(t_b["searches"] - t_a["searches"] - fin) / max(1, drains) if mode else 0.0)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--line", type=int, default=None, help="internal: run one line in this process and print its JSON line")
    ap.add_argument("--lines", default="1,2,3,4,5,6,7")
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll-cheap", type=int, default=128)
    ap.add_argument("--preroll-full", type=int, default=26)
    ap.add_argument("--cache-entries", type=int, default=32768)
    ap.add_argument("--per-launch", type=int, default=1, help="asynchronous lines: most simulations a game runs inside one tree launch")
    ap.add_argument("--timer-stride", type=int, default=176)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_reuse_async_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    rows = []
    for line in [int(x) for x in args.lines.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--line", str(line)] + [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in
               ("games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "per_launch", "timer_stride")]
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
    base = {r["line"]: r["moves_per_s"] for r in rows}
    best = max((r for r in rows if r["asynchronous"] and r["tree_reuse"] == 2), key=lambda r: r["moves_per_s"], default=None)
    doc = dict(what="tree reuse inside the asynchronous movers against the lock-step runners at the headline workload, one box, one process after the "
                    "other (tools/tree_reuse_async_ab.py); games/s are not comparable across modes",
               best_async_top_up=None if best is None else best["name"],
               async_top_up_beats_lockstep_off=None if best is None or 1 not in base else best["moves_per_s"] > base[1],
               async_top_up_beats_lockstep_top_up=None if best is None or 2 not in base else best["moves_per_s"] > base[2],
               lines=rows)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
