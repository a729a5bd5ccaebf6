#!/usr/bin/env python3
"""DeviceReplay.sample(512) against sample(512, augment="board") on a filled 15x15 ring (azk_replay_gather), on the GPU:

    python3 tools/replay_gather_bench.py [--out profiles/replay_gather_sample.json] [--capacity 400000] [--batch 512] [--rounds 5]

Each round times both forms back to back - 20 warm-up calls, then HIP events around 200 calls - so that whatever else the machine is doing
hits both alike; the figures are the per-call medians over the rounds, with the rounds' extremes.  sample() draws its indices with
torch.randperm over the whole ring in both forms, so the same pair is also timed with the indices fixed: the three torch gathers plus the
dtype conversion against the one azk_replay_gather launch.  There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alpha-zero_amd"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--capacity", type=int, default=400000, help="ring tuples (bench.py's DeviceReplay holds 400000)")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    import azk
    rows = cols = 15
    rp = azk.DeviceReplay(a.capacity, 2, rows, cols, rows * cols)
    gen = torch.Generator(device=rp.states.device).manual_seed(1)
    rp.states.copy_((torch.rand(rp.states.shape, generator=gen, device=rp.states.device) < 0.3).to(torch.float32))
    rp.pis.copy_(torch.rand(rp.pis.shape, generator=gen, device=rp.pis.device, dtype=torch.float64))
    rp.zs.copy_(torch.randint(-1, 2, rp.zs.shape, generator=gen, device=rp.zs.device).to(torch.float32))
    rp.cursor.fill_(a.capacity)
    idx = torch.randperm(a.capacity, device=rp.states.device)[:a.batch]
    draws = torch.randint(-(1 << 31), 1 << 31, (a.batch,), dtype=torch.int32, device=rp.states.device)
    forms = {
        "sample": lambda: rp.sample(a.batch),
        "sample_augment_board": lambda: rp.sample(a.batch, augment="board"),
        "fixed_idx_torch_gathers": lambda: (rp.states[idx], rp.pis[idx].float(), rp.zs[idx][:, None]),
        "fixed_idx_replay_gather": lambda: rp.gather(idx, draws, 0xFF),
    }
    # the two forms of each pair compute the same thing where they can be compared: no draws = torch's gathers, exactly
    s, p, z = rp.gather(idx, None, 0xFF)
    assert torch.equal(s, rp.states[idx]) and torch.equal(p, rp.pis[idx].float()) and torch.equal(z, rp.zs[idx])
    us = {k: [] for k in forms}
    for _ in range(a.rounds):
        for name, f in forms.items():
            for _ in range(a.warmup):
                f()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                f()
            t1.record()
            t1.synchronize()
            us[name].append(t0.elapsed_time(t1) * 1e3 / a.calls)
    out = {"what": "per-call time in microseconds: HIP events around `calls` calls after `warmup` warm-up calls, per round; median over the rounds",
           "device": torch.cuda.get_device_name(0), "gcn_arch": torch.cuda.get_device_properties(0).gcnArchName, "board": [rows, cols], "ring_tuples": a.capacity, "batch": a.batch, "calls": a.calls,
           "warmup": a.warmup, "rounds": a.rounds,
           "us_per_call": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in us.items()}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
