"""Time st_lock_set, st_afterstates_at, st_routes_at, st_policy_locks and
st_play_locks beside the slot-landing calls of the parent, and play the
lock-position player out beside the routed player.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30), for the
feature sets 'base' (GREEDY_WEIGHTS) and 'bcts' (BCTS_WEIGHTS).  Each workload
is timed with device events over enough launches to fill its share of
--seconds, four rounds alternating the workloads in one process, after a
warm-up; every round of every workload starts from the aged snapshot.
Reported per workload: the rounds' us per call (per step for the players) and
their median.  Then:
  fused_vs_by_hand    play_locks per step against the fastest round of the only
                      other way to play over lock positions (lock_set(cap=64) +
                      afterstates_at + a torch score / argmax + routes_at + step,
                      all envs every step), and whether the gap exceeds the
                      rounds' spread -- both sides are new code: a consistency
                      figure, no speed-up over the parent;
  planner_vs_routed   policy_locks over policy_routed (all envs), beside the
                      lock positions evaluated over the reachable slots;
  need_quarter        policy_locks with a random quarter of the envs needed.
`players` (bcts only): from a reset, K primitive steps of play_locks and of
play_routed; pieces = spawns, deaths = episodes, lines = (return + 100 * deaths)
/ 100 under the default reward; and, in a loop by hand of play_locks, the share
of chosen positions that are no slot's landing.

usage: python tools/locks_bench.py [--envs N] [--age STEPS] [--seconds S] [--k K] [--play-steps K]
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
from routed_bench import spawns  # noqa: E402

CAP = 64


def players(n, k_steps):
    """Lines per piece and deaths of the two honest BCTS players from a reset,
    and how often the lock-position player tucks."""
    out = {}

    def mk():
        return TetrisBatch(n, width=10, height=20, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                           validate_actions=False)

    def row(b, s0, ret, eps):
        pieces, deaths = int((spawns(b) - s0).sum()), int(eps.sum())
        lines = (int(ret.sum()) + 100 * deaths) / 100
        return {"pieces": pieces, "lines": lines, "lines_per_piece": round(lines / max(pieces, 1), 4), "deaths": deaths}

    for name in ("play_locks", "play_routed"):
        b = mk()
        b.reset()
        w = b._weights(BCTS_WEIGHTS, "bcts")
        s0 = spawns(b)
        ret, eps, pcs = getattr(b, name)(w, k_steps, features="bcts", obs="none")
        out[name] = dict(row(b, s0, ret, eps), steps=k_steps, routes_finished=int(pcs.sum()))
        b.close()
    # play_locks by hand: which of the chosen positions are no slot's landing
    b = mk()
    b.reset()
    w = b._weights(BCTS_WEIGHTS, "bcts")
    dev = b.device
    rem = torch.zeros(n, dtype=torch.int32, device=dev)
    outs = (torch.full((n,), -1, dtype=torch.int32, device=dev),
            torch.full((C.ROUTE_WORDS, n), (1 << 63) - 1, dtype=torch.int64, device=dev),
            torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
            torch.zeros((18, n), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    pos, route, steps = outs[0], outs[1], outs[2]
    chosen = torch.zeros((), dtype=torch.int64, device=dev)
    tucks = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(k_steps):
        need = rem == 0
        b.policy_locks(w, features="bcts", need=need, out=outs)
        af = b.afterstates(boards=False)
        slot = (pos >> 5).clamp(min=0).long()[:, None]
        landing = (af.valid.gather(1, slot)[:, 0] != 0) & (af.y.gather(1, slot)[:, 0] == (pos & 31))
        picked = need & (pos >= 0)
        chosen += picked.sum()
        tucks += (picked & ~landing).sum()
        length = steps.clamp(max=C.ROUTE_MAX)
        rem = torch.where(need, length, rem)
        i = (length - rem).clamp(min=0).long()
        word = torch.where(i >= 21, route[1], route[0])
        a = torch.where(rem > 0, (word >> (3 * (i % 21))) & 7, torch.full_like(word, 2)).to(torch.uint8)
        rem = (rem - 1).clamp(min=0)
        b.step(a, obs="none")
    out["chosen_positions"] = int(chosen)
    out["chosen_no_landing_share"] = round(int(tucks) / max(int(chosen), 1), 4)
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
    S, dev = b.n_slots, b.device
    steps = torch.empty((n, S), dtype=torch.int32, device=dev)
    b.reachable(first=False, out=(steps, None))
    ls_out = (torch.empty((n, S), dtype=torch.int32, device=dev), torch.empty((n, CAP), dtype=torch.int32, device=dev),
              torch.empty(n, dtype=torch.int32, device=dev))
    ls = b.lock_set(cap=CAP, out=ls_out)
    lst, cnt = ls.pos.clone(), ls.count.clone()
    # a random lock position per env (-1 where an env has none), and the landing of its farthest slot
    pick = (torch.rand(n, device=dev) * cnt.clamp(max=CAP)).long().clamp(max=CAP - 1)
    rnd_pos = lst.gather(1, pick[:, None])[:, 0].contiguous()
    far = steps.argmax(dim=1)
    far_pos = torch.where(steps.max(dim=1).values > 0,
                          far * 32 + b.afterstates(boards=False).y.gather(1, far[:, None])[:, 0].long(),
                          torch.full_like(far, -1)).to(torch.int32)
    rnd_slot = (torch.rand((n, S), device=dev) * (steps > 0)).argmax(dim=1).to(torch.int32)
    need4 = (torch.rand(n, device=dev) < 0.25).to(torch.uint8)
    r_out = (torch.empty((C.ROUTE_WORDS, n), dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
    p_out = (torch.empty(n, dtype=torch.int32, device=dev), r_out[0], r_out[1],
             torch.empty(n, dtype=torch.float32, device=dev))
    out = {"envs": n, "board": [10, 20], "slots": S, "aged_steps": args.age, "k": K, "cap": CAP,
           "device": torch.cuda.get_device_name(dev),
           "mean_lock_positions": round(float(cnt.float().mean()), 3),
           "mean_reachable_slots": round(float((steps > 0).sum(dim=1).float().mean()), 3),
           "no_landing_share_of_lock_positions":
               round(1.0 - float((steps > 0).sum()) / max(float(cnt.sum()), 1.0), 4),
           "max_lock_positions": int(cnt.max()), "sets": {}}

    for feats, weights in (("base", GREEDY_WEIGHTS), ("bcts", BCTS_WEIGHTS)):
        w = b._weights(weights, feats)
        rows = w.shape[1]
        l_out = (torch.empty(n, dtype=torch.int32, device=dev), r_out[0], r_out[1],
                 torch.empty(n, dtype=torch.float32, device=dev), torch.empty((rows, n), dtype=torch.int32, device=dev),
                 torch.empty(n, dtype=torch.int32, device=dev))
        wcol = w[0][None, :, None]

        def by_hand_step():
            q = b.lock_set(cap=CAP, out=ls_out).pos
            feat = b.afterstates_at(q, boards=False, features=feats).feat
            score = (feat.float() * wcol).sum(dim=1)
            score = torch.where(feat[:, 0] != 0, score, torch.full_like(score, float("-inf")))
            best = q.gather(1, score.argmax(dim=1, keepdim=True))[:, 0].contiguous()
            rt = b.routes_at(best, out=r_out)
            b.step(torch.where(rt.steps > 0, rt.action(0), torch.full_like(rt.action(0), 2)), obs="none")

        def by_hand():
            for _ in range(K):
                by_hand_step()

        b.load(aged)
        work = {
            "lock_set_rows": (lambda: b.lock_set(out=(ls_out[0], None, ls_out[2])), 1, False),
            "lock_set_rows_and_list": (lambda: b.lock_set(cap=CAP, out=ls_out), 1, False),
            "afterstates_at_cap64": (lambda: b.afterstates_at(lst, features=feats), 1, False),
            "routes_at_random": (lambda: b.routes_at(rnd_pos, out=r_out), 1, False),
            "routes_at_farthest": (lambda: b.routes_at(far_pos, out=r_out), 1, False),
            "policy_locks_all": (lambda: b.policy_locks(w, features=feats, out=l_out), 1, False),
            "policy_locks_need_quarter": (lambda: b.policy_locks(w, features=feats, need=need4, out=l_out), 1, False),
            "play_locks_per_step": (lambda: b.play_locks(w, K, features=feats, obs="none"), K, True),
            "by_hand_per_step": (by_hand, K, True),
            "reachable_steps": (lambda: b.reachable(first=False, out=(steps, None)), 1, False),
            "afterstates": (lambda: b.afterstates(features=feats), 1, False),
            "routes_random": (lambda: b.routes(rnd_slot, out=r_out), 1, False),
            "policy_routed_all": (lambda: b.policy_routed(w, features=feats, out=p_out), 1, False),
            "play_routed_per_step": (lambda: b.play_routed(w, K, features=feats, obs="none"), K, True),
        }
        reps = {}
        for k, (fn, div, restore) in work.items():  # warm-up, and calls per round
            b.load(aged)  # (every workload from the aged snapshot: the stateless calls' inputs were taken on it)
            timed(fn, 1)
            us = timed(fn, 2)
            reps[k] = max(2, int(args.seconds / args.rounds * 1e6 / us))
        runs = {k: [] for k in work}
        for _ in range(args.rounds):
            for k, (fn, div, restore) in work.items():
                b.load(aged)
                torch.cuda.synchronize()
                runs[k].append(timed(fn, reps[k]) / div)
        b.load(aged)
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = {k: max(v) - min(v) for k, v in runs.items()}
        res = {"calls_per_round": reps,
               "workloads": {k: {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2),
                                 "spread_us": round(spread[k], 2)} for k in work}}
        gap = min(runs["by_hand_per_step"]) - med["play_locks_per_step"]
        res["fused_vs_by_hand"] = {
            "play_locks_median_us": round(med["play_locks_per_step"], 2),
            "by_hand_fastest_us": round(min(runs["by_hand_per_step"]), 2), "gap_us": round(gap, 2),
            "rounds_spread_us": round(max(spread["by_hand_per_step"], spread["play_locks_per_step"]), 2),
            "reached": bool(gap > max(spread["by_hand_per_step"], spread["play_locks_per_step"]))}
        res["planner_vs_routed"] = {
            "policy_locks_all_us": round(med["policy_locks_all"], 2),
            "policy_routed_all_us": round(med["policy_routed_all"], 2),
            "ratio": round(med["policy_locks_all"] / med["policy_routed_all"], 3),
            "positions_over_slots": round(out["mean_lock_positions"] / max(out["mean_reachable_slots"], 1e-9), 3)}
        res["need_quarter"] = {"us": round(med["policy_locks_need_quarter"], 2), "needed_envs": int(need4.sum()),
                               "quarter_of_all_us": round(med["policy_locks_all"] / 4, 2)}
        res["play_locks_over_play_routed"] = round(med["play_locks_per_step"] / med["play_routed_per_step"], 3)
        out["sets"][feats] = res
    b.close()
    torch.cuda.synchronize()
    if not args.no_players:
        out["players"] = players(n, args.play_steps)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
