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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "alpha-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (name, eval symmetry on)
LINES = [("async off", False), ("async eval symmetry", True)]


def worker(args):
    import torch
    import azk
    from pvnet import NetConfig, PolicyValueNet
    from selfplay import AsyncSelfPlayRunner, KernelTimer
    name, sym = LINES[args.line - 1]
    torch.cuda.set_device(0)
    A = args.size * args.size
    net = PolicyValueNet(NetConfig(args.size, args.size, 2, A, 5, 512, 8, 1), seed=0, device="cuda:0", dtype=torch.bfloat16, path="clsfold")
    kt = KernelTimer(stride=args.timer_stride)
    replay = azk.DeviceReplay(args.replay_capacity, 2, args.size, args.size, A)
    runner = AsyncSelfPlayRunner("gomoku", net, args.games, args.sims, per_launch=args.per_launch, size=args.size, seed=0, device=0,
                                 leaf_dtype="bfloat16", recycle=True, kernel_timer=kt, cache_entries=args.cache_entries, cache_shared=True,
                                 steps_per_graph=args.steps_per_graph, replay=replay, eval_symmetry=True if sym else None)
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
    out = dict(line=args.line, name=name, eval_symmetry=bool(sym), steps_per_graph=args.steps_per_graph,
               per_launch=args.per_launch, games=args.games, sims=args.sims, size=args.size, steps=args.steps,
               ms_per_G_moves=1e3 * dt * args.games / moves, moves_per_s=d["moves"] / dt,
               games_per_s=d["games"] / dt, mean_plies_of_finished_games=d["plies"] / max(1, d["games"]),
               sims_per_move=c["sims"] / moves,
               tree_launches_per_G_moves=(runner.launches - launches0) * args.games / moves,
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
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2, help="how often the pair of lines is run, alternated")
    ap.add_argument("--trace-steps", type=int, default=3, help="timed steps of the traced run (0: no traced run)")
    ap.add_argument("--trace-timeout", type=int, default=300, help="seconds for the traced run")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_symmetry_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    keys = ("games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "replay_capacity", "per_launch",
            "steps_per_graph", "timer_stride")

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
    kernels = None
    if args.trace_steps > 0:
        import csv
        import glob
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + child(2, steps=args.trace_steps, warmup=1, preroll_cheap=32, preroll_full=2)
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.trace_timeout)
            except subprocess.TimeoutExpired:
                print(f"traced run: no result after {args.trace_timeout} s - stopping here", file=sys.stderr)
                return 124
            if r.returncode != 0:
                print(f"traced run: exit status {r.returncode}\n{r.stderr[-4000:]}", file=sys.stderr)
                return r.returncode
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            kernels = {}
            for row in (csv.DictReader(open(files[0])) if files else []):
                for want in ("k_sym_leaves", "k_sym_logits", "k_tree", "k_move_async"):
                    if want in row["Name"]:
                        k = kernels.setdefault(want, dict(calls=0, total_ns=0.0))
                        k["calls"] += int(row["Calls"])
                        k["total_ns"] += float(row["TotalDurationNs"])
            for k in kernels.values():
                k["us_per_launch"] = 1e-3 * k.pop("total_ns") / max(1, k["calls"])
            print(json.dumps(kernels), flush=True)

    def mean(line, key):
        v = [r[key] for r in rows if r["line"] == line]
        return sum(v) / len(v)
    summary = {k: dict(off=mean(1, k), on=mean(2, k)) for k in ("ms_per_G_moves", "leaves_evaluated_per_move", "cache_hit_share", "k_tree_us_per_launch",
                                                               "tree_launches_per_G_moves", "mean_plies_of_finished_games")}
    doc = dict(what="evaluation under a position-keyed board symmetry inside the asynchronous movers at the headline workload, one box, one process after the "
                    "other, off and on alternated (tools/eval_symmetry_ab.py); every figure is measured; kernels_traced comes from a separate short run of the "
                    "'on' line under rocprofv3 --kernel-trace --stats",
               lines=rows, mean_of_rounds=summary, kernels_traced=kernels)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
