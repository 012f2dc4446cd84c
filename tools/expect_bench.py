"""Time st_next_weights / st_policy_expect / st_play_expect against
st_policy_lookahead and the one-ply entry points.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30).  Each
workload is timed with device events over enough calls to fill about a quarter
of a second, four rounds alternating the workloads in one process, after a
warm-up; reported are the rounds' us and their median.

  next_weights                    st_next_weights
  expect_base / _bcts             policy_expect, the three per-env outputs, one weight row, first_weights too
  expect_base_table / _bcts_table with scores_all, tails and slots2_all
  lookahead_base / _bcts          policy_lookahead of the same set (four per-env outputs): the parent's call
  policy_linear_base / _bcts      policy_linear of the same set (all four outputs)
  play_expect_base / _bcts        us per PIECE of play_expect(k=100)
  play_lookahead_base / _bcts     us per PIECE of play_lookahead(k=100)
  play_linear_base / _bcts        us per PIECE of play_linear(k=100, placements=True)

`held_against`, as reached or not reached:
  (a) expect_<set> <= 7 x lookahead_<set> (medians), by more than the rounds'
      spread: the slowest round of expect is below 7 x the fastest round of
      lookahead.  The expectimax without the fused call is seven known-piece
      calls' worth of second plies; the kernel shares the staging and the first
      ply across the seven pieces.
  (b) is decided across processes: `--ab LABEL` prints one line of timings of
      the entry points the new translation unit must leave as they were
      (policy_linear, policy_lookahead, play_linear) through the library ST_LIB
      names (ST_AB_OLD_ABI=1 for a build that predates the new calls); run it
      in alternated processes, one library each, and compare the lines.
`players`: lines per piece and deaths over 100 pieces from a reset with
BCTS_WEIGHTS -- one ply, the next piece known, expectimax (information).

usage: python tools/expect_bench.py [--envs N] [--age STEPS] [--seconds S] [--only NAME ...] [--ab LABEL]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
from gym_simpletetris_amd import BCTS_WEIGHTS, GREEDY_WEIGHTS, TetrisBatch, _lib as C  # noqa: E402
from gym_simpletetris_amd.engine import weight_rows  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def players(n, W, H, k):
    """Lines per piece and deaths with BCTS_WEIGHTS: one ply, the next piece
    known, and the expectimax."""
    out = {}
    for name in ("one_ply", "known_next_piece", "expectimax"):
        b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                        validate_actions=False)
        b.reset()
        wt = torch.as_tensor(weight_rows(BCTS_WEIGHTS, "bcts"), device=b.device)
        lines = torch.zeros((), dtype=torch.int64, device=b.device)
        deaths = torch.zeros((), dtype=torch.int64, device=b.device)
        for _ in range(k):
            if name == "one_ply":
                c = b.policy_linear(wt, features="bcts")
            elif name == "known_next_piece":
                c = b.policy_lookahead(wt, first_weights=wt, features="bcts")
            else:
                c = b.policy_expect(wt, first_weights=wt, features="bcts")
            feat = b.afterstates(boards=False, features="bcts").feat
            lines += feat[:, C.AFTER["lines"]].gather(1, c.slots.clamp(min=0).long()[:, None]).sum()
            _, _, d = b.step_placements(c.slots, obs="none")
            deaths += d.sum()
        out[name] = {"lines_per_piece": round(int(lines) / (n * k), 4), "deaths": int(deaths), "pieces": n * k}
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only", nargs="*", default=None, help="workload names (default: all)")
    ap.add_argument("--no-players", action="store_true")
    ap.add_argument("--ab", default=None, metavar="LABEL", help="one line of the unchanged entry points' timings")
    args = ap.parse_args()
    n, W, H, K = args.envs, 10, 20, 100
    new = hasattr(C.load(), "st_policy_expect")  # (a library from before the calls: the older workloads only)

    b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    aged = b.save()
    S, dev = b.n_slots, b.device

    def outs(rows):
        return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                torch.empty(n, dtype=torch.float32, device=dev), torch.empty((rows, n), dtype=torch.int32, device=dev))
    o11, o18 = outs(11), outs(18)
    w11 = torch.as_tensor(weight_rows(GREEDY_WEIGHTS), device=dev)
    w18 = torch.as_tensor(weight_rows(BCTS_WEIGHTS, "bcts"), device=dev)
    ret = torch.zeros(n, dtype=torch.int64, device=dev)
    eps = torch.zeros(n, dtype=torch.int32, device=dev)
    la4 = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    work = {
        "policy_linear_base": (lambda: b.policy_linear(w11, out=o11), 1),
        "policy_linear_bcts": (lambda: b.policy_linear(w18, out=o18, features="bcts"), 1),
        "lookahead_base": (lambda: b.policy_lookahead(w11, first_weights=w11, out=la4), 1),
        "lookahead_bcts": (lambda: b.policy_lookahead(w18, first_weights=w18, features="bcts", out=la4), 1),
        "play_linear_base": (lambda: b.play_linear(w11, K, returns=ret, episodes=eps, placements=True), K),
        "play_linear_bcts": (lambda: b.play_linear(w18, K, returns=ret, episodes=eps, placements=True,
                                                   features="bcts"), K),
    }
    if args.ab is not None:  # criterion (b): one process, one library, one line
        work["play_linear_steps_base"] = (lambda: b.play_linear(w11, K), K)
        out = {"label": args.ab}
        for k, (fn, per) in work.items():
            b.load(aged)
            timed(fn, 1)
            us = timed(fn, 2)
            b.load(aged)
            b.next_piece()  # (every env holds its preview: policy_lookahead's steady state)
            torch.cuda.synchronize()
            out[k] = round(timed(fn, max(2, int(0.25e6 / us))) / per, 2)
        b.close()
        print(json.dumps(out))
        return
    res = {"envs": n, "board": [W, H], "slots": S, "aged_steps": args.age, "lib": C.LIB_PATH,
           "device": torch.cuda.get_device_name(dev)}
    if new:
        ex3 = (la4[0], la4[2], la4[3])
        ex6 = ex3 + (torch.empty((n, S), dtype=torch.float32, device=dev),
                     torch.empty((n, 7, S), dtype=torch.float32, device=dev),
                     torch.empty((n, 7, S), dtype=torch.int32, device=dev))
        mo = torch.empty((7, n), dtype=torch.int32, device=dev)
        work.update({
            "next_weights": (lambda: b.next_weights(out=mo), 1),
            "expect_base": (lambda: b.policy_expect(w11, first_weights=w11, out=ex3), 1),
            "expect_base_table": (lambda: b.policy_expect(w11, first_weights=w11, table=True, out=ex6), 1),
            "expect_bcts": (lambda: b.policy_expect(w18, first_weights=w18, features="bcts", out=ex3), 1),
            "expect_bcts_table": (lambda: b.policy_expect(w18, first_weights=w18, features="bcts", table=True,
                                                          out=ex6), 1),
            "play_lookahead_base": (lambda: b.play_lookahead(w11, K, first_weights=w11, returns=ret, episodes=eps,
                                                             obs="none"), K),
            "play_lookahead_bcts": (lambda: b.play_lookahead(w18, K, first_weights=w18, features="bcts", returns=ret,
                                                             episodes=eps, obs="none"), K),
            "play_expect_base": (lambda: b.play_expect(w11, K, first_weights=w11, returns=ret, episodes=eps,
                                                       obs="none"), K),
            "play_expect_bcts": (lambda: b.play_expect(w18, K, first_weights=w18, features="bcts", returns=ret,
                                                       episodes=eps, obs="none"), K),
        })
        feat = b.afterstates(boards=False).feat
        live = ((feat[:, C.AFTER["valid"]] != 0) & (feat[:, C.AFTER["dead"]] == 0)).sum(1).to(torch.float64).mean()
        res["mean_live_first_ply_slots"] = round(float(live), 3)
    if args.only:
        work = {k: work[k] for k in args.only}
    reps = {}
    for k, (fn, per) in work.items():  # warm-up, and calls per quarter second
        slow = per > 1
        if not slow:
            b.load(aged)  # (the play workloads move the states on; the single calls see the aged ones)
        timed(fn, 1 if slow else 3)
        us = timed(fn, 1 if slow else 5)
        reps[k] = max(1 if slow else 5, int(args.seconds / args.rounds * 1e6 / us))
    runs = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, (fn, per) in work.items():
            if per == 1:
                b.load(aged)
                b.next_piece()  # (every env holds its preview: policy_lookahead's steady state)
                torch.cuda.synchronize()
            runs[k].append(timed(fn, reps[k]) / per)
    b.close()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in runs.items()}
    res["calls_per_round"] = reps
    res["workloads"] = {k: {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2)} for k in work}
    held, ratio, cost = {}, {}, {}
    for fs in ("base", "bcts"):
        ex, la, pl = "expect_" + fs, "lookahead_" + fs, "policy_linear_" + fs
        if ex in med and la in med:
            ok = med[ex] <= 7 * med[la] and max(runs[ex]) < 7 * min(runs[la])
            held[f"(a) {ex} {round(med[ex], 1)} <= 7 x {la} {round(med[la], 1)} = {round(7 * med[la], 1)}, "
                 f"slowest round {round(max(runs[ex]), 1)} < 7 x fastest round {round(7 * min(runs[la]), 1)}"] = \
                "reached" if ok else "not reached"
            ratio[f"{ex} / {la}"] = round(med[ex] / med[la], 2)
        if ex in med and pl in med and "mean_live_first_ply_slots" in res:
            ratio[f"work ratio {ex} / ({pl} x 7 x live)"] = \
                round(med[ex] / (med[pl] * 7 * res["mean_live_first_ply_slots"]), 3)
        for x, y in (("play_expect_" + fs, "play_lookahead_" + fs), ("play_expect_" + fs, "play_linear_" + fs),
                     (ex + "_table", ex)):
            if x in med and y in med:
                cost[f"{x} - {y}"] = round(med[x] - med[y], 2)
    res["held_against"], res["ratios"], res["cost_us"] = held, ratio, cost
    if new and not args.no_players:
        res["players"] = players(n, W, H, K)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
