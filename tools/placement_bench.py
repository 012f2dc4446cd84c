"""Time the placement step against the primitive-action player it replaces.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30).  Each
workload is timed with device events over enough calls to fill its share of
--seconds, four rounds alternating the workloads in one process, after a
warm-up; reported are the rounds' figures and their median.

  play_placements_k100   us per ITERATION (one piece) of
                         play_linear(k=100, placements=True)
  play_linear_k100       us per primitive STEP of play_linear(k=100), the
                         parent's player, in the same process
  loop_policy_hard_drop  us per step of a Python loop policy_linear (action
                         byte alone, not used) -> step on hard drops: the
                         placement iteration's two launches without the
                         commit -- every env locks in every step, as in a
                         placement iteration -- on the parent's kernels
  step_placements        place + step (two launches) on one slot tensor, the
                         greedy choice for the states at the round's start,
                         reused by every call: after the first call the slots
                         belong to earlier pieces, an arbitrary mix of valid
                         and invalid, so the commit is not taken in every
                         call; every env still locks (lock_delay is 0)
  place                  the commit alone, on the same reused slots
  step                   st_step alone on hard drops (obs 'none'), for scale

For the two players also the pieces locked per second and the primitive steps
(iterations) per locked piece: locks are counted from the sum of the seven
shape-count rows before and after each timed run (every lock spawns a piece,
in the step or in the same-step reset behind a death).

The two players advance the envs, so the rounds see states of growing age;
the greedy weights with autoreset keep them mid-game.  The comparisons the
numbers are held against are printed as `held_against` (true: reached):
  (a) a placement iteration costs no more than the parent's play_linear step,
      within the spread (max - min) of the parent's own four rounds;
  (b) pieces per second are above the parent's.

usage: python tools/placement_bench.py [--envs N] [--age STEPS] [--seconds S] [--out PATH]
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
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "placements.txt"))
    args = ap.parse_args()
    n, W, H, K = args.envs, 10, 20, 100
    b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    dev = b.device
    w1 = torch.as_tensor(weight_rows(GREEDY_WEIGHTS), device=dev)
    ret = torch.zeros(n, dtype=torch.int64, device=dev)
    eps = torch.zeros(n, dtype=torch.int32, device=dev)
    drops = torch.full((n,), 2, dtype=torch.uint8, device=dev)
    slots = torch.empty(n, dtype=torch.int32, device=dev)
    placed = torch.empty(n, dtype=torch.uint8, device=dev)

    def spawned():
        st = b.state_tensors(("stats",), sync=False)["stats"]
        return int(st[C.STAT["count0"]: C.STAT["count0"] + 7, :n].sum(dtype=torch.int64))

    act = torch.empty(n, dtype=torch.uint8, device=dev)

    def loop_policy_hard_drop():
        b.policy_linear(w1, out=(None, act, None, None))
        b.step(drops, obs="none")

    def fresh_slots():  # the greedy choice of the present states (valid for the first call that uses them)
        b.policy_linear(w1, out=(slots, None, None, None))

    work = {
        "play_placements_k100": (lambda: b.play_linear(w1, K, returns=ret, episodes=eps, placements=True), K),
        "play_linear_k100": (lambda: b.play_linear(w1, K, returns=ret, episodes=eps), K),
        "loop_policy_hard_drop": (loop_policy_hard_drop, 1),
        "step_placements": (lambda: b.step_placements(slots, obs="none"), 1),
        "place": (lambda: b.place(slots, out=placed), 1),
        "step": (lambda: b.step(drops, obs="none"), 1),
    }
    players = ("play_placements_k100", "play_linear_k100")
    reps = {}
    for k, (fn, per) in work.items():  # warm-up, and calls per round
        fresh_slots()
        timed(fn, 3)
        us = timed(fn, 5 if per > 1 else 20)
        reps[k] = max(3 if per > 1 else 20, int(args.seconds / args.rounds / len(work) * 1e6 / us))
    runs = {k: [] for k in work}
    locks = {k: [] for k in players}
    for _ in range(args.rounds):
        for k, (fn, per) in work.items():
            fresh_slots()
            c0 = spawned() if k in players else 0
            us = timed(fn, reps[k])
            runs[k].append(us / per)
            if k in players:
                locks[k].append((spawned() - c0, us * reps[k]))  # pieces, us
    b.close()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in runs.items()}
    res = {"envs": n, "board": [W, H], "aged_steps": args.age, "k": K, "lib": os.path.relpath(C.LIB_PATH, ROOT),
           "device": torch.cuda.get_device_name(dev), "calls_per_round": reps,
           "workloads": {k: {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2)} for k in work}}
    for k in players:
        pps = [p / (us * 1e-6) for p, us in locks[k]]
        spp = [reps[k] * K * n / p for p, _ in locks[k]]
        res["workloads"][k].update(
            pieces_per_s=[round(x) for x in pps], median_pieces_per_s=round(statistics.median(pps)),
            steps_per_piece=[round(x, 3) for x in spp], median_steps_per_piece=round(statistics.median(spp), 3))
    parent = runs["play_linear_k100"]
    spread = max(parent) - min(parent)
    pl, pa = res["workloads"]["play_placements_k100"], res["workloads"]["play_linear_k100"]
    res["parent_spread_us"] = round(spread, 2)
    res["pieces_per_s_ratio"] = round(pl["median_pieces_per_s"] / pa["median_pieces_per_s"], 3)
    res["held_against"] = {
        "(a) play_placements_k100 <= play_linear_k100 + parent spread (us per iteration / step)":
            bool(med["play_placements_k100"] <= med["play_linear_k100"] + spread),
        "(b) pieces per second above the parent's": bool(pl["median_pieces_per_s"] > pa["median_pieces_per_s"]),
    }
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("tools/placement_bench.py --seconds %g: %d 10x20 envs aged %d greedy steps, device events, %d rounds\n"
                    "alternating the workloads in one process; us per call (per ITERATION = piece for\n"
                    "play_placements_k100, per primitive STEP for play_linear_k100).\n\n"
                    % (args.seconds, n, args.age, args.rounds))
            f.write(text + "\n")


if __name__ == "__main__":
    main()
