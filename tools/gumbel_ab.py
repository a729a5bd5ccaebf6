#!/usr/bin/env python3
"""Same-box report of the Gumbel root search (azk_set_gumbel_root) inside the asynchronous movers at the headline workload:
Gomoku 15x15, 2 048 games, bf16 clsfold evaluator, captured graphs, shared eval cache of 32 768 entries.

    python3 tools/gumbel_ab.py [--out profiles/gumbel_root_ab.json] [--m 16 --c-visit 50 --c-scale 1]

Lines: 1 option off at 800 simulations, 2 option off at 64, 3 Gumbel root (m, c_visit, c_scale) at 64.  One child process per line, one after
the other on the same GPU, each under its own time limit; the first one that fails ends the run (nothing more is started on the GPU).  Per
line: ms per G moves, k_tree's and k_move_async's mean time per launch (HIP events around sampled eager launches), the drain's time per call,
the movers' share of the wall time (k_move_async in every step + the drains), and leaves evaluated per move from the device counters.  A
Gumbel search's budget is fixed (its halving table is built for it), so the 64-simulation lines run their pre-roll at 64 simulations; line 1
has the cheap pre-roll of the other tools.  Nothing here has a bar: the option changes the search, so the lines are not one workload.
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

# (name, simulations: "long" | "short", Gumbel root on)
LINES = [("off, long search", "long", False), ("off, short search", "short", False), ("gumbel root, short search", "short", True)]


def worker(args):
    import torch
    import azk
    from pvnet import NetConfig, PolicyValueNet
    from selfplay import AsyncSelfPlayRunner, KernelTimer
    name, kind, gumbel = LINES[args.line - 1]
    sims = args.sims if kind == "long" else args.sims_short
    steps = args.steps if kind == "long" else args.steps_short
    torch.cuda.set_device(0)
    A = args.size * args.size
    net = PolicyValueNet(NetConfig(args.size, args.size, 2, A, 5, 512, 8, 1), seed=0, device="cuda:0", dtype=torch.bfloat16, path="clsfold")
    kt = KernelTimer(stride=args.timer_stride)
    replay = azk.DeviceReplay(args.replay_capacity, 2, args.size, args.size, A)
    runner = AsyncSelfPlayRunner("gomoku", net, args.games, sims, per_launch=args.per_launch, size=args.size, seed=0, device=0,
                                 leaf_dtype="bfloat16", recycle=True, kernel_timer=kt, cache_entries=args.cache_entries, cache_shared=True,
                                 steps_per_graph=args.steps_per_graph, replay=replay,
                                 gumbel_root=(args.m, args.c_visit, args.c_scale) if gumbel else None)
    drain_events, mover_events = [], []
    eng, plain_drain, plain_step = runner.eng, runner.eng.async_drain, runner.eng.async_step

    def bracket(store, fn, *a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = fn(*a, **k)
        e.record()
        store.append((s, e))
        return r

    def timed_drain(*a, **k):
        return bracket(drain_events, plain_drain, *a, **k) if kt.enabled else plain_drain(*a, **k)

    def timed_step(logits, values, phases=3):                   # phases == 2 alone: the movers of a sampled eager step
        return bracket(mover_events, plain_step, logits, values, phases) if kt.enabled and phases == 2 else plain_step(logits, values, phases)
    eng.async_drain, eng.async_step = timed_drain, timed_step

    def totals():
        st = runner.finish()
        return dict(moves=int(st[5]), games=int(st[0]), plies=int(st[1]), searches=int(st[7]), tuples=int(replay.cursor.item()))

    if kind == "long":                                          # untimed pre-roll as bench.py's: cheap searches de-phase the slots
        runner.n_sims = 16
        for _ in range(args.preroll_cheap):
            runner.play_move()
        runner.n_sims = sims
        for _ in range(args.preroll_full + args.warmup):
            runner.play_move()
    else:                                                       # a short search is cheap: the whole pre-roll at its own budget
        for _ in range(args.preroll_cheap + args.preroll_full + args.warmup):
            runner.play_move()
    t_a = totals()
    runner.reset_counters()
    launches0, chunks0 = runner.launches, runner.chunks
    kt.enabled = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
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
    launches = runner.launches - launches0

    def robust_us(pairs):
        t = sorted(a.elapsed_time(b) for a, b in pairs)
        kept = [x for x in t if x <= 3.0 * t[len(t) // 2]] if t else []
        return 1e3 * sum(kept) / len(kept) if kept else None
    mover_us = robust_us(mover_events)
    drain_s = 1e-3 * sum(a.elapsed_time(b) for a, b in drain_events)
    out = dict(line=args.line, name=name, gumbel_root=[args.m, args.c_visit, args.c_scale] if gumbel else None, steps_per_graph=args.steps_per_graph,
               per_launch=args.per_launch, games=args.games, sims=sims, size=args.size, steps=steps,
               ms_per_G_moves=1e3 * dt * args.games / moves, moves_per_s=d["moves"] / dt,
               games_per_s=d["games"] / dt, mean_plies_of_finished_games=d["plies"] / max(1, d["games"]),
               sims_per_move=c["sims"] / moves, tree_launches_per_G_moves=launches * args.games / moves,
               leaves_evaluated_per_move=c["leaves_evaluated"] / moves, cache_hit_share=c["cache_hits"] / max(1, c["sims"]),
               recorded_tuples_per_s=d["tuples"] / dt,
               k_tree_us_per_launch=None if tree[0] is None else 1e3 * tree[0], k_tree_samples=tree[2],
               k_move_async_us_per_launch=mover_us, k_move_async_samples=len(mover_events),
               drains=runner.chunks - chunks0, drain_us_per_call=1e6 * drain_s / max(1, len(drain_events)),
               movers_share_of_time=None if mover_us is None else (1e-6 * mover_us * launches + drain_s) / dt)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--line", type=int, default=None, help="internal: run one line in this process and print its JSON line")
    ap.add_argument("--lines", default="1,2,3")
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=800, help="simulations of line 1")
    ap.add_argument("--sims-short", type=int, default=64, help="simulations of lines 2 and 3")
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--c-visit", type=float, default=50.0)
    ap.add_argument("--c-scale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20, help="timed moves per slot of line 1")
    ap.add_argument("--steps-short", type=int, default=200, help="timed moves per slot of lines 2 and 3")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll-cheap", type=int, default=128)
    ap.add_argument("--preroll-full", type=int, default=26)
    ap.add_argument("--cache-entries", type=int, default=32768)
    ap.add_argument("--replay-capacity", type=int, default=200000)
    ap.add_argument("--per-launch", type=int, default=1, help="most simulations a game runs inside one tree launch")
    ap.add_argument("--steps-per-graph", type=int, default=32, help="steps between two drains")
    ap.add_argument("--timer-stride", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gumbel_root_ab.json"))
    args = ap.parse_args()
    if args.line is not None:
        return worker(args)
    rows = []
    for line in [int(x) for x in args.lines.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--line", str(line)] + [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in
               ("games", "sims", "sims_short", "size", "m", "c_visit", "c_scale", "steps", "steps_short", "warmup", "preroll_cheap", "preroll_full",
                "cache_entries", "replay_capacity", "per_launch", "steps_per_graph", "timer_stride")]
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
    doc = dict(what="Gumbel root search inside the asynchronous movers at the headline workload, one box, one process after the other "
                    "(tools/gumbel_ab.py); every figure is measured; the strength of a network trained on these targets is not",
               lines=rows)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
