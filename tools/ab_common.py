"""What the tools/*_ab.py programs share: the import path, the arguments, the headline network and asynchronous runner, HIP-event brackets
around an engine call, bench.py's pre-roll, the timed window with its common output fields, and the parent side - one child process per
line, one after the other on the same GPU, each under its own time limit, nothing more started after the first that fails.  Helpers, not
a framework: a tool keeps its docstring, its LINES, its own arguments and output fields, and calls what fits it."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "alpha-zero_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# dest: (type, default, help) - a tool names the ones it takes, in the order its --help lists them, and overrides defaults and help texts
COMMON_ARGS = dict(
    line=(int, None, "internal: run one line in this process and print its JSON line"),
    games=(int, 2048, None), sims=(int, 800, None), size=(int, 15, None), steps=(int, 20, None), warmup=(int, 5, None),
    preroll_cheap=(int, 128, None), preroll_full=(int, 26, None), cache_entries=(int, 32768, None), replay_capacity=(int, 200000, None),
    per_launch=(int, 1, "most simulations a game runs inside one tree launch"), steps_per_graph=(int, 32, "steps between two drains"),
    timer_stride=(int, 176, None), timeout=(int, 240, "seconds per line"))


def add_common_args(ap, *names, help={}, **defaults):
    for n in names or COMMON_ARGS:
        kind, default, text = COMMON_ARGS[n]
        ap.add_argument("--" + n.replace("_", "-"), type=kind, default=defaults.get(n, default), help=help.get(n, text))


def out_path(name):
    return os.path.join(ROOT, "profiles", name)


# ---- the child: one line in one process ---------------------------------------------------------------------------------------------
def headline_net(args):
    """The headline evaluator: 5 blocks, width 512, 8 heads, bf16, the clsfold path, on a size x size Gomoku board."""
    import torch
    from pvnet import NetConfig, PolicyValueNet
    torch.cuda.set_device(0)
    A = args.size * args.size
    return PolicyValueNet(NetConfig(args.size, args.size, 2, A, 5, 512, 8, 1), seed=0, device="cuda:0", dtype=torch.bfloat16, path="clsfold")


def headline_options(args, kt, **options):
    """The runner keywords of the headline workload; `options` override and add."""
    return dict(dict(size=args.size, seed=0, device=0, leaf_dtype="bfloat16", recycle=True, kernel_timer=kt, cache_entries=args.cache_entries,
                     cache_shared=True), **options)


def device_replay(args):
    import azk
    return azk.DeviceReplay(args.replay_capacity, 2, args.size, args.size, args.size * args.size)


def async_runner(args, kt, replay, sims=None, **options):
    from selfplay import AsyncSelfPlayRunner
    if "steps_per_graph" not in options:
        options["steps_per_graph"] = args.steps_per_graph
    return AsyncSelfPlayRunner("gomoku", headline_net(args), args.games, args.sims if sims is None else sims,
                               **headline_options(args, kt, per_launch=args.per_launch, replay=replay, **options))


def bracket_calls(obj, method, store, when):
    """Put HIP events around the calls of obj.method for which when(*args) holds; the (start, end) pairs go to `store`."""
    import torch
    plain = getattr(obj, method)

    def call(*a, **k):
        if not when(*a, **k):
            return plain(*a, **k)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        r = plain(*a, **k)
        e.record()
        store.append((s, e))
        return r
    setattr(obj, method, call)


def events_ms(store):
    return sum(a.elapsed_time(b) for a, b in store)


def drain_fields(drain_events, dt):
    return dict(drain_us_per_call=1e3 * events_ms(drain_events) / max(1, len(drain_events)), drain_share_of_time=1e-3 * events_ms(drain_events) / dt)


def leaf_fields(c, moves):
    return dict(leaves_evaluated_per_move=c["leaves_evaluated"] / max(1, moves), cache_hit_share=c["cache_hits"] / max(1, c["sims"]))


def preroll(runner, args, cheap=True):
    """The untimed pre-roll as bench.py's: de-phase the slots with cheap searches, then one game length under the real search.  cheap=False:
    the whole pre-roll at the runner's own budget (a search whose budget is fixed, or is cheap anyway)."""
    moves = args.preroll_full + args.warmup
    if cheap:
        full = runner.n_sims
        runner.n_sims = 16
        for _ in range(args.preroll_cheap):
            runner.play_move()
        runner.n_sims = full
    else:
        moves += args.preroll_cheap
    for _ in range(moves):
        runner.play_move()


def totals(runner, replay):
    if hasattr(runner, "finish"):                                 # asynchronous: waits for everything enqueued
        st = runner.finish()
        t = dict(moves=int(st[5]), games=int(st[0]), plies=int(st[1]), searches=int(st[7]), full=int(st[8]), fast=int(st[9]))
    else:
        t = dict(moves=runner.plies_played, games=runner.games_finished, plies=runner.finished_plies, searches=0)
    if replay is not None:
        t["tuples"] = int(replay.cursor.item())
    return dict(t, launches=runner.launches, drains=getattr(runner, "chunks", 0))


def timed_window(runner, replay, args, steps):
    """`steps` timed moves per slot with the kernel timer on -> (seconds, the deltas of totals() over the window, the device counters of the
    window, the output fields every tool reports)."""
    import torch
    kt = runner.kernel_timer
    t_a = totals(runner, replay)
    runner.reset_counters()
    kt.enabled = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        runner.play_move()
    t_b = totals(runner, replay)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kt.enabled = False
    runner.check_error()
    c = runner.counters()
    d = {k: t_b[k] - t_a[k] for k in t_a}
    moves = max(1, d["moves"])
    tree = kt.robust_mean_ms()
    fields = dict(steps_per_graph=runner.steps_per_graph, per_launch=runner.per_launch, games=args.games, sims=runner.n_sims, size=args.size, steps=steps,
                  ms_per_G_moves=1e3 * dt * args.games / moves, moves_per_s=d["moves"] / dt,
                  games_per_s=d["games"] / dt, mean_plies_of_finished_games=d["plies"] / max(1, d["games"]),
                  sims_per_move=c["sims"] / moves, tree_launches_per_G_moves=d["launches"] * args.games / moves,
                  k_tree_us_per_launch=None if tree[0] is None else 1e3 * tree[0], k_tree_samples=tree[2])
    return dt, d, c, fields


# ---- the parent: one child process per line -----------------------------------------------------------------------------------------
def child_cmd(script, args, flag, value, forwarded, **over):
    return [sys.executable, os.path.abspath(script), flag, str(value)] + [f"--{k.replace('_', '-')}={over.get(k, getattr(args, k))}" for k in forwarded]


def run_child(cmd, timeout, label):
    """One child under its own time limit -> (0, its standard output), or (the status that ends the run, None): 124 after the time limit,
    else the child's own.  The caller starts nothing more after a status that is not 0."""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        print(f"{label}: no result after {timeout} s - stopping here", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(f"{label}: exit status {r.returncode} - stopping here\n{r.stderr[-4000:]}", file=sys.stderr)
        return r.returncode, None
    return 0, r.stdout


def collect_lines(script, args, lines, forwarded, rounds=None, flag="--line"):
    """The lines, one child each, one after the other (rounds: the whole list that many times, each row marked with its round) ->
    (0, their JSON rows), or (the status of the first child that failed, the rows so far) with nothing started after it."""
    rows = []
    for rnd in range(rounds or 1):
        for line in lines:
            label = f"{flag[2:]} {line}" if rounds is None else f"round {rnd} {flag[2:]} {line}"
            status, text = run_child(child_cmd(script, args, flag, line, forwarded), args.timeout, label)
            if status != 0:
                return status, rows
            row = json.loads(text.strip().splitlines()[-1])
            rows.append(row if rounds is None else dict(row, round=rnd))
            print(json.dumps(rows[-1]), flush=True)
    return 0, rows


def write_doc(out, **doc):
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def run_lines(script, args, lines, forwarded, what, out):
    status, rows = collect_lines(script, args, lines, forwarded)
    if status == 0:
        write_doc(out, what=what, lines=rows)
    return status


def traced_kernels(child, timeout, label, wanted):
    """One more child, under `rocprofv3 --kernel-trace --stats` and a time limit of its own -> (0, {kernel: calls, us_per_launch} for the
    wanted name fragments, from the profiler's per-kernel statistics), or (status, None) as run_child."""
    import csv
    import glob
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        status, _ = run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + child, timeout, label)
        if status != 0:
            return status, None
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        kernels = {}
        for row in (csv.DictReader(open(files[0])) if files else []):
            for want in wanted:
                if want in row["Name"]:
                    k = kernels.setdefault(want, dict(calls=0, total_ns=0.0))
                    k["calls"] += int(row["Calls"])
                    k["total_ns"] += float(row["TotalDurationNs"])
    for k in kernels.values():
        k["us_per_launch"] = 1e-3 * k.pop("total_ns") / max(1, k["calls"])
    return 0, kernels


def mean_of(rows, line, key):
    v = [r[key] for r in rows if r["line"] == line and r.get(key) is not None]
    return sum(v) / len(v) if v else None
