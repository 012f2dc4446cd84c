"""Time st_routes, st_policy_routed and st_play_routed beside the calls they
replace and the players of the parent, and play the three BCTS players out.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30), for the
feature sets 'base' (GREEDY_WEIGHTS) and 'bcts' (BCTS_WEIGHTS).  Each workload
is timed with device events over enough launches to fill its share of
--seconds, four rounds alternating the workloads in one process, after a
warm-up; every round of a playing workload starts from the aged snapshot.
Reported per workload: the rounds' us per call (per step for the players, per
piece for the placement player) and their median.  Then:
  honest_vs_by_hand   play_routed per step against the fastest round of the
                      loop by hand (reachable(first=False) + policy_linear(
                      allowed=) + route_actions + step, all envs every step),
                      and whether the gap exceeds the rounds' spread;
  planner_vs_parts    policy_routed over (reachable_steps + policy_linear_allowed
                      + routes_chosen), the three calls it fuses, all envs;
  need_quarter        policy_routed with one env in four needed (a random
                      quarter), over a quarter of the all-env time;
                      policy_routed_need_every_4th is the same load on a
                      strided mask, which two of the eight XCDs serve alone.
`players` (bcts only): from a reset, K primitive steps of play_routed and of
play_linear, and as many placement steps as play_routed locked pieces per env;
pieces = spawns (the shape counters), deaths = episodes, lines = (return + 100 *
deaths) / 100 under the default reward (a lock that dies pays -100 whatever it
cleared); and, in a loop by hand of the teleporting player, the share of its
placements whose slot reachable() does not hold.

usage: python tools/routed_bench.py [--envs N] [--age STEPS] [--seconds S] [--k K] [--play-steps K]
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
from afterstates_bench import timed  # noqa: E402
from gym_simpletetris_amd import BCTS_WEIGHTS, GREEDY_WEIGHTS, TetrisBatch, _lib as C  # noqa: E402


def spawns(b):
    st = b.state_tensors(("stats",))["stats"]
    return st[C.STAT["count0"]:C.STAT["count0"] + 7, :b.n].sum(dim=0).to(torch.int64)


def players(n, k_steps):
    """Lines per piece and deaths of the three BCTS players from a reset."""
    out = {}
    def mk():
        return TetrisBatch(n, width=10, height=20, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                           validate_actions=False)

    def row(b, s0, ret, eps):
        pieces, deaths = int((spawns(b) - s0).sum()), int(eps.sum())
        lines = (int(ret.sum()) + 100 * deaths) / 100
        return {"pieces": pieces, "lines": lines, "lines_per_piece": round(lines / max(pieces, 1), 4), "deaths": deaths}

    b = mk()
    b.reset()
    w = b._weights(BCTS_WEIGHTS, "bcts")
    s0 = spawns(b)
    ret, eps, pcs = b.play_routed(w, k_steps, features="bcts", obs="none")
    out["play_routed"] = dict(row(b, s0, ret, eps), steps=k_steps, routes_finished=int(pcs.sum()))
    per_env = max(1, round(out["play_routed"]["pieces"] / n))
    b.close()
    b = mk()
    b.reset()
    s0 = spawns(b)
    ret, eps = b.play_linear(w, k_steps, features="bcts")
    out["play_linear"] = dict(row(b, s0, ret, eps), steps=k_steps)
    b.close()
    b = mk()
    b.reset()
    s0 = spawns(b)
    ret, eps = b.play_linear(w, per_env, placements=True, features="bcts")
    out["play_linear_placements"] = dict(row(b, s0, ret, eps), placement_steps=per_env)
    b.close()
    b = mk()  # the teleporting player by hand: how many of its placements the piece could not have reached
    b.reset()
    placed = torch.zeros((), dtype=torch.int64, device=b.device)
    unreach = torch.zeros((), dtype=torch.int64, device=b.device)
    for _ in range(per_env):
        steps = b.reachable(first=False).steps
        sl = b.policy_linear(w, features="bcts").slots
        ok = sl >= 0
        placed += ok.sum()
        unreach += (ok & (steps.gather(1, sl.clamp(min=0).long()[:, None])[:, 0] == 0)).sum()
        b.step_placements(sl, obs="none")
    out["teleported_unreachable_share"] = round(int(unreach) / max(int(placed), 1), 4)
    out["teleported_placements"] = int(placed)
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--play-steps", type=int, default=400)
    ap.add_argument("--no-players", action="store_true")
    args = ap.parse_args()
    n, K = args.envs, args.k
    b = TetrisBatch(n, width=10, height=20, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    aged = b.save()
    S = b.n_slots
    steps = torch.empty((n, S), dtype=torch.int32, device=b.device)
    b.reachable(first=False, out=(steps, None))
    far = steps.argmax(dim=1).to(torch.int32)
    # a random reachable slot per env (the farthest where an env has none)
    pick = (torch.rand((n, S), device=b.device) * (steps > 0)).argmax(dim=1).to(torch.int32)
    rnd = torch.where((steps > 0).any(dim=1), pick, far)
    # one env in four: at random, as a player's plans run out -- and every fourth env, which the
    # round-robin of workgroups over the eight XCDs sends to two of them
    need4 = (torch.rand(n, device=b.device) < 0.25).to(torch.uint8)
    need4s = (torch.arange(n, device=b.device) % 4 == 0).to(torch.uint8)
    act = torch.empty(n, dtype=torch.uint8, device=b.device)
    rsteps = torch.empty(n, dtype=torch.int32, device=b.device)
    lin_out = (torch.empty(n, dtype=torch.int32, device=b.device), None, None, None)
    r_out = (torch.empty((C.ROUTE_WORDS, n), dtype=torch.int64, device=b.device),
             torch.empty(n, dtype=torch.int32, device=b.device))
    p_out = (torch.empty(n, dtype=torch.int32, device=b.device), r_out[0], r_out[1],
             torch.empty(n, dtype=torch.float32, device=b.device))
    out = {"envs": n, "board": [10, 20], "slots": S, "aged_steps": args.age, "k": K,
           "device": torch.cuda.get_device_name(b.device),
           "reachable_share_of_envs": round(float((steps > 0).any(dim=1).float().mean()), 4),
           "mean_route_steps_random": round(float(steps.gather(1, rnd.long()[:, None]).float().mean()), 3),
           "mean_route_steps_farthest": round(float(steps.max(dim=1).values.float().mean()), 3), "sets": {}}

    for feats, weights in (("base", GREEDY_WEIGHTS), ("bcts", BCTS_WEIGHTS)):
        w = b._weights(weights, feats)

        def by_hand_step():
            b.reachable(first=False, out=(steps, None))
            b.policy_linear(w, out=lin_out, features=feats, allowed=steps)
            b.route_actions(lin_out[0], out=act, steps=rsteps)
            b.step(act, obs="none")

        def by_hand():
            for _ in range(K):
                by_hand_step()

        b.load(aged)
        b.reachable(first=False, out=(steps, None))
        chosen = b.policy_linear(w, features=feats, allowed=steps).slots.clone()
        # name -> (callable, divisor of the call's time, restore the aged state first)
        work = {
            "routes_random": (lambda: b.routes(rnd, out=r_out), 1, False),
            "routes_farthest": (lambda: b.routes(far, out=r_out), 1, False),
            "routes_chosen": (lambda: b.routes(chosen, out=r_out), 1, False),
            "reachable_steps": (lambda: b.reachable(first=False, out=(steps, None)), 1, False),
            "policy_linear_allowed": (lambda: b.policy_linear(w, out=lin_out, features=feats, allowed=steps), 1, False),
            "route_actions_chosen": (lambda: b.route_actions(chosen, out=act, steps=rsteps), 1, False),
            "policy_routed_all": (lambda: b.policy_routed(w, features=feats, out=p_out), 1, False),
            "policy_routed_need_quarter": (lambda: b.policy_routed(w, features=feats, need=need4, out=p_out), 1, False),
            "policy_routed_need_every_4th": (lambda: b.policy_routed(w, features=feats, need=need4s, out=p_out), 1,
                                             False),
            "play_routed_per_step": (lambda: b.play_routed(w, K, features=feats, obs="none"), K, True),
            "by_hand_per_step": (by_hand, K, True),
            "play_linear_per_step": (lambda: b.play_linear(w, K, features=feats), K, True),
            "play_linear_placements_per_piece": (lambda: b.play_linear(w, K, placements=True, features=feats), K, True),
        }
        reps = {}
        for k, (fn, div, restore) in work.items():  # warm-up, and calls per round
            if restore:
                b.load(aged)
            timed(fn, 1)
            us = timed(fn, 2)
            reps[k] = max(2, int(args.seconds / args.rounds * 1e6 / us))
        runs = {k: [] for k in work}
        for _ in range(args.rounds):
            for k, (fn, div, restore) in work.items():
                if restore:
                    b.load(aged)
                    torch.cuda.synchronize()
                runs[k].append(timed(fn, reps[k]) / div)
        b.load(aged)
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = {k: max(v) - min(v) for k, v in runs.items()}
        res = {"calls_per_round": reps,
               "workloads": {k: {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2),
                                 "spread_us": round(spread[k], 2)} for k in work}}
        gap = min(runs["by_hand_per_step"]) - med["play_routed_per_step"]
        res["honest_vs_by_hand"] = {
            "play_routed_median_us": round(med["play_routed_per_step"], 2),
            "by_hand_fastest_us": round(min(runs["by_hand_per_step"]), 2), "gap_us": round(gap, 2),
            "rounds_spread_us": round(max(spread["by_hand_per_step"], spread["play_routed_per_step"]), 2),
            "reached": bool(gap > max(spread["by_hand_per_step"], spread["play_routed_per_step"]))}
        parts = med["reachable_steps"] + med["policy_linear_allowed"] + med["routes_chosen"]
        res["planner_vs_parts"] = {"policy_routed_all_us": round(med["policy_routed_all"], 2),
                                   "three_calls_us": round(parts, 2),
                                   "ratio": round(med["policy_routed_all"] / parts, 3)}
        res["need_quarter"] = {"us": round(med["policy_routed_need_quarter"], 2),
                               "needed_envs": int(need4.sum()),
                               "quarter_of_all_us": round(med["policy_routed_all"] / 4, 2),
                               "ratio_to_needed_envs_times_three_calls":
                                   round(med["policy_routed_need_quarter"] / (parts * int(need4.sum()) / n), 3)}
        out["sets"][feats] = res
    b.close()
    torch.cuda.synchronize()
    if not args.no_players:
        out["players"] = players(n, args.play_steps)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
