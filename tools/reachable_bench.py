"""Time st_reachable (with and without `first`) and st_route_actions beside
st_afterstates (features only) and st_policy_greedy, the parent's calls that
look at the same placements, as the scale to read them on.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30).  Each
workload is timed with device events over enough launches to fill about a
quarter of a second, four rounds alternating the workloads in one process,
after a warm-up.  Reported per workload: the rounds' us per call and their
median; the ratio to st_policy_greedy; and, for the two st_reachable calls, the
share of the write floor -- the output bytes over the best store rate
tools/write_bw (built from tools/write_bw.hip, run here as a child process)
measures on the same box in the same call.  Also reported: the share of valid
slots that is reachable, and the longest shortest route (the search runs that
many layers and then until no set grows).

usage: python tools/reachable_bench.py [--envs N] [--age STEPS] [--seconds S] [--lock-delay L] [--no-write-bw]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from afterstates_bench import timed, write_rate  # noqa: E402
from gym_simpletetris_amd import TetrisBatch, _lib as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--lock-delay", type=int, default=0)
    ap.add_argument("--no-write-bw", action="store_true")
    args = ap.parse_args()
    n, W, H = args.envs, 10, 20
    b = TetrisBatch(n, width=W, height=H, lock_delay=args.lock_delay, step_reset=args.lock_delay > 0,
                    autoreset="same_step", seeds=[1000 + e for e in range(n)], validate_actions=False)
    b.reset()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    S, NF = b.n_slots, C.AFTER_NFEAT
    feat = torch.empty((n, NF, S), dtype=torch.int32, device=b.device)
    steps = torch.empty((n, S), dtype=torch.int32, device=b.device)
    first = torch.empty((n, S), dtype=torch.uint8, device=b.device)
    act = torch.empty(n, dtype=torch.uint8, device=b.device)
    rsteps = torch.empty(n, dtype=torch.int32, device=b.device)
    b.reachable(out=(steps, first))
    b.afterstates(boards=False, out=(feat, None))
    reach = steps > 0
    valid = feat[:, C.AFTER["valid"]] != 0
    # a reachable target per env (its farthest), and a random slot per env: valid or not, reachable or not
    far = steps.argmax(dim=1).to(torch.int32)
    rnd = torch.randint(-1, S, (n,), dtype=torch.int32, device=b.device)
    work = {
        "reachable_first": lambda: b.reachable(out=(steps, first)),
        "reachable_steps": lambda: b.reachable(first=False, out=(steps, None)),
        "route_actions_farthest": lambda: b.route_actions(far, out=act, steps=rsteps),
        "route_actions_random": lambda: b.route_actions(rnd, out=act, steps=rsteps),
        "afterstates_features": lambda: b.afterstates(boards=False, out=(feat, None)),
        "policy_greedy": lambda: b.policy_greedy(0, seed=3, explore=0, out=act),
    }
    bytes_out = {"reachable_first": n * S * 5, "reachable_steps": n * S * 4, "route_actions_farthest": n * 5,
                 "route_actions_random": n * 5, "afterstates_features": n * NF * S * 4, "policy_greedy": n}
    stats = {"valid_share": round(float(valid.sum()) / (n * S), 4),
             "reachable_share_of_valid": round(float(reach.sum()) / float(valid.sum()), 4),
             "longest_route_steps": int(steps.max()),
             "mean_steps_of_reachable": round(float(steps[reach].float().mean()), 3),
             "mean_longest_route_per_env": round(float(steps.max(dim=1).values.float().mean()), 3)}
    reps = {}
    for k, fn in work.items():  # warm-up, and launches per quarter second
        timed(fn, 5)
        us = timed(fn, 20)
        reps[k] = max(20, int(args.seconds / args.rounds * 1e6 / us))
    runs = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, fn in work.items():
            runs[k].append(timed(fn, reps[k]))
    b.close()
    torch.cuda.synchronize()
    rate, rate_src = (None, "skipped") if args.no_write_bw else write_rate()
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {"envs": n, "board": [W, H], "slots": S, "aged_steps": args.age, "lock_delay": args.lock_delay,
           "step_reset": args.lock_delay > 0, **stats, "device": torch.cuda.get_device_name(b.device),
           "launches_per_round": reps, "write_bw_TBps": rate, "write_bw_run": rate_src, "workloads": {}}
    for k in work:
        w = {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2),
             "ratio_to_policy_greedy": round(med[k] / med["policy_greedy"], 3),
             "ns_per_env": round(med[k] * 1e3 / n, 3),
             "output_bytes": bytes_out[k], "output_bytes_per_env": bytes_out[k] / n}
        if rate and k.startswith("reachable"):
            floor = bytes_out[k] / (rate * 1e6)  # us
            w["write_floor_us"] = round(floor, 2)
            w["share_of_write_floor"] = round(floor / med[k], 3)
        out["workloads"][k] = w
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
