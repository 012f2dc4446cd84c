"""Time st_afterstates (with and without boards) and st_placement_actions
against st_policy_greedy, which evaluates the same placements one env per lane
and keeps one action byte.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30).  Each
workload is timed with device events over enough launches to fill about a
quarter of a second, four rounds alternating the workloads in one process,
after a warm-up.  Reported per workload: the rounds' us per call and their
median; the ratio to st_policy_greedy; and the share of the write floor --
the output bytes, computed from the shapes, over the best store rate
tools/write_bw (built from tools/write_bw.hip, run here as a child process)
measures on the same box in the same call.

usage: python tools/afterstates_bench.py [--envs N] [--age STEPS] [--seconds S] [--no-write-bw]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
from gym_simpletetris_amd import TetrisBatch, _lib as C  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def write_rate():
    """Best TB/s of tools/write_bw's runs, or None if it is not built."""
    exe = os.path.join(ROOT, "tools", "write_bw")
    if not os.path.exists(exe):
        return None, "tools/write_bw not built (hipcc --offload-arch=gfx950 -O3 tools/write_bw.hip -o tools/write_bw)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True)
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    best = max(rows, key=lambda d: d["TBps"])
    return best["TBps"], best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--no-write-bw", action="store_true")
    args = ap.parse_args()
    n, W, H = args.envs, 10, 20
    b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    S, NF = b.n_slots, C.AFTER_NFEAT
    feat = torch.empty((n, NF, S), dtype=torch.int32, device=b.device)
    brd = torch.empty((n, W, S), dtype=torch.int32, device=b.device)
    slots = torch.randint(-1, S, (n,), dtype=torch.int32, device=b.device)
    act = torch.empty(n, dtype=torch.uint8, device=b.device)
    work = {
        "afterstates_boards": lambda: b.afterstates(out=(feat, brd)),
        "afterstates_features": lambda: b.afterstates(boards=False, out=(feat, None)),
        "placement_actions": lambda: b.placement_actions(slots, out=act),
        "policy_greedy": lambda: b.policy_greedy(0, seed=3, explore=0, out=act),
    }
    bytes_out = {"afterstates_boards": n * (NF + W) * S * 4, "afterstates_features": n * NF * S * 4,
                 "placement_actions": n, "policy_greedy": n}
    reps = {}
    for k, fn in work.items():  # warm-up, and launches per quarter second
        timed(fn, 5)
        us = timed(fn, 20)
        reps[k] = max(20, int(args.seconds / args.rounds * 1e6 / us))
    runs = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, fn in work.items():
            runs[k].append(timed(fn, reps[k]))
    valid = float(feat[:, C.AFTER["valid"]].sum()) / (n * S)
    b.close()
    torch.cuda.synchronize()
    rate, rate_src = (None, "skipped") if args.no_write_bw else write_rate()
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {"envs": n, "board": [W, H], "slots": S, "aged_steps": args.age, "valid_share": round(valid, 4),
           "device": torch.cuda.get_device_name(b.device), "launches_per_round": reps,
           "write_bw_TBps": rate, "write_bw_run": rate_src, "workloads": {}}
    for k in work:
        w = {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2),
             "ratio_to_policy_greedy": round(med[k] / med["policy_greedy"], 3),
             "output_bytes": bytes_out[k], "output_bytes_per_env": bytes_out[k] / n}
        if rate and k.startswith("afterstates"):
            floor = bytes_out[k] / (rate * 1e6)  # us
            w["write_floor_us"] = round(floor, 2)
            w["share_of_write_floor"] = round(floor / med[k], 3)
        out["workloads"][k] = w
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
