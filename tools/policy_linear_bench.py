"""Time st_policy_linear and st_play_linear against what a linear feature
player had before them.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30).  Each
workload is timed with device events over enough calls to fill about a
quarter of a second, four rounds alternating the workloads in one process,
after a warm-up; reported are the rounds' us and their median.

  policy_linear_nw1 / _nw1024   all four outputs, GREEDY_WEIGHTS as one row /
                                as 1,024 rows (env e reads row e % 1024)
  policy_linear_actions         n_w = 1, the action byte alone
  policy_greedy                 the compiled-in weights, one env per lane
  afterstates_features          afterstates(boards=False) alone
  parent_pipeline               afterstates(boards=False) -> torch score and
                                argmax -> placement_actions
  step                          st_step alone (obs 'none'), for scale
  play_linear_k100              us per STEP of play_linear(k=100)
  python_loop                   us per STEP of policy_linear -> step in Python
  python_loop_sums              the same loop keeping play_linear's two sums
                                (two torch adds per step)

The last two advance the envs, so the rounds see states of growing age; the
greedy player with autoreset keeps them mid-game.  The comparisons the numbers
are held against are printed as `held_against` (true: reached).

usage: python tools/policy_linear_bench.py [--envs N] [--age STEPS] [--seconds S] [--only NAME ...]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
from gym_simpletetris_amd import GREEDY_WEIGHTS, TetrisBatch, _lib as C  # noqa: E402
from gym_simpletetris_amd.engine import weight_rows  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only", nargs="*", default=None, help="workload names (default: all)")
    args = ap.parse_args()
    n, W, H, K = args.envs, 10, 20, 100
    b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    S, NF, dev = b.n_slots, C.AFTER_NFEAT, b.device
    feat = torch.empty((n, NF, S), dtype=torch.int32, device=dev)
    act = torch.empty(n, dtype=torch.uint8, device=dev)
    out = (torch.empty(n, dtype=torch.int32, device=dev), act, torch.empty(n, dtype=torch.float32, device=dev),
           torch.empty((NF, n), dtype=torch.int32, device=dev))
    w1 = torch.as_tensor(weight_rows(GREEDY_WEIGHTS), device=dev)
    w1024 = w1.repeat(1024, 1).contiguous()
    ret = torch.zeros(n, dtype=torch.int64, device=dev)
    eps = torch.zeros(n, dtype=torch.int32, device=dev)
    slot_no = torch.arange(S, device=dev)

    def pipeline():
        a = b.afterstates(boards=False, out=(feat, None))
        sc = 80 * a.lines - 12 * a.holes - 3 * a.height - 2000 * a.above
        key = torch.where(a.valid != 0, sc.to(torch.int64) * 256 + (255 - slot_no), -(1 << 40))
        slots = torch.where((a.valid != 0).any(dim=1), key.argmax(dim=1), -1)
        b.placement_actions(slots, out=act)

    def loop_step():
        b.step(b.policy_linear(w1, out=(None, act, None, None)).actions, obs="none")

    ret2, eps2 = torch.zeros_like(ret), torch.zeros_like(eps)

    def loop_step_sums():
        _, r, d = b.step(b.policy_linear(w1, out=(None, act, None, None)).actions, obs="none")
        ret2.add_(r)
        eps2.add_(d)

    work = {
        "policy_linear_nw1": (lambda: b.policy_linear(w1, out=out), 1),
        "policy_linear_nw1024": (lambda: b.policy_linear(w1024, out=out), 1),
        "policy_linear_actions": (lambda: b.policy_linear(w1, out=(None, act, None, None)), 1),
        "policy_greedy": (lambda: b.policy_greedy(0, seed=3, explore=0, out=act), 1),
        "afterstates_features": (lambda: b.afterstates(boards=False, out=(feat, None)), 1),
        "parent_pipeline": (pipeline, 1),
        "step": (lambda: b.step(act, obs="none"), 1),
        "play_linear_k100": (lambda: b.play_linear(w1, K, returns=ret, episodes=eps), K),
        "python_loop": (loop_step, 1),
        "python_loop_sums": (loop_step_sums, 1),
    }
    if args.only:
        work = {k: work[k] for k in args.only}
    reps = {}
    for k, (fn, per) in work.items():  # warm-up, and calls per quarter second
        timed(fn, 3)
        us = timed(fn, 5 if per > 1 else 20)
        reps[k] = max(3 if per > 1 else 20, int(args.seconds / args.rounds * 1e6 / us))
    runs = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, (fn, per) in work.items():
            runs[k].append(timed(fn, reps[k]) / per)
    b.close()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in runs.items()}
    res = {"envs": n, "board": [W, H], "slots": S, "aged_steps": args.age, "lib": C.LIB_PATH,
           "device": torch.cuda.get_device_name(dev), "calls_per_round": reps,
           "workloads": {k: {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2)} for k in work}}
    held = {}
    for a, bb in (("policy_linear_nw1", "afterstates_features"), ("policy_linear_nw1", "policy_greedy"),
                  ("policy_linear_nw1024", "afterstates_features"), ("policy_linear_nw1024", "policy_greedy")):
        if a in med and bb in med:
            held[f"{a} < {bb}"] = bool(med[a] < med[bb])
    for loop in ("python_loop", "python_loop_sums"):
        if "play_linear_k100" in med and loop in med:
            held[f"play_linear_k100 <= {loop} (per step)"] = bool(med["play_linear_k100"] <= med[loop])
    res["held_against"] = held
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
