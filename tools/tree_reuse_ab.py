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
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "alpha-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def worker(args):
    import torch
    from pvnet import NetConfig, PolicyValueNet
    from selfplay import KernelTimer, SelfPlayRunner
    torch.cuda.set_device(0)
    A = args.size * args.size
    net = PolicyValueNet(NetConfig(args.size, args.size, 2, A, 5, 512, 8, 1), seed=0, device="cuda:0", dtype=torch.bfloat16, path="clsfold")
    kt = KernelTimer(stride=args.timer_stride)
    runner = SelfPlayRunner("gomoku", net, args.games, args.sims, size=args.size, seed=0, device=0, leaf_dtype="bfloat16", recycle=True,
                            kernel_timer=kt, use_graph=True, n_split=1, cache_entries=args.cache_entries, cache_shared=True,
                            steps_per_graph=32, tree_reuse=args.mode)
    eng = runner.eng
    begin_events = []

    def timed(fn):
        def call(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **k)
            e.record()
            if kt.enabled:
                begin_events.append((s, e))
            return r
        return call
    eng.begin_search = timed(eng.begin_search)
    eng.begin_search_budget = timed(eng.begin_search_budget)

    # untimed pre-roll as bench.py's: de-phase the slots with cheap searches, then one game length under the real search
    full = runner.n_sims
    runner.n_sims = 16
    for _ in range(args.preroll_cheap):
        runner.play_move()
    runner.n_sims = full
    for _ in range(args.preroll_full + args.warmup):
        runner.play_move()
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
               begin_kernel_us_per_call=1e3 * sum(a.elapsed_time(b) for a, b in begin_events) / max(1, len(begin_events)),
               begin_kernel_calls=len(begin_events),
               k_tree_us_per_launch=None if tree is None else 1e3 * tree[0], k_tree_samples=None if tree is None else tree[2],
               roots_reused_share=c["roots_reused"] / max(1, moves), nodes_carried_per_reroot=c["nodes_carried"] / max(1, c["roots_reused"]),
               root_visits_at_end_of_search=end_visit, root_visits_carried_per_move=end_visit - sims_per_move,
               cache_hit_share=c["cache_hits"] / max(1, c["sims"]), leaves_evaluated_per_move=c["leaves_evaluated"] / max(1, moves))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=int, default=None, help="internal: run one mode in this process and print its JSON line")
    ap.add_argument("--modes", default="0,1,2")
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--preroll-cheap", type=int, default=128)
    ap.add_argument("--preroll-full", type=int, default=26)
    ap.add_argument("--cache-entries", type=int, default=32768)
    ap.add_argument("--timer-stride", type=int, default=176)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per mode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_reuse_ab.json"))
    args = ap.parse_args()
    if args.mode is not None:
        return worker(args)
    rows = []
    for mode in [int(x) for x in args.modes.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", str(mode)] + [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in
               ("games", "sims", "size", "steps", "warmup", "preroll_cheap", "preroll_full", "cache_entries", "timer_stride")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"mode {mode}: no result after {args.timeout} s - stopping here", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f"mode {mode}: exit status {r.returncode} - stopping here\n{r.stderr[-4000:]}", file=sys.stderr)
            return r.returncode
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    doc = dict(what="SelfPlayRunner at the headline workload with tree_reuse 0 / 1 / 2, one box, one process after the other (tools/tree_reuse_ab.py)",
               modes=rows)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
