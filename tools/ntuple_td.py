"""A short TD(0) demo on the n-tuple player: afterstate learning from a zero
table, everything on the device.

One iteration is one piece in every env:
  c  = policy_ntuple(table, weights = REWARD row 1, index=True)   argmax r + V(s'), its value and table entries
  the previous piece's afterstate s'_prev is updated towards r + V(s'): delta = r + V(s') - V(s'_prev), where
     r is the reward of the placement chosen now (its REWARD row), 0 and V = dead_value where it ends the game
  step_placements(c.slots)
with td_update(table, index_prev, delta, alpha / (T n)): index_add_ sums the envs' steps into the entries they
share, so the step is the batch's mean (the sum over 4,096 envs diverges).  Lines per piece are measured over
`--eval` pieces from a reset, before and after `--pieces` iterations.  Information only: nothing is asserted, and whether it learns in the pieces given is
reported as it comes out.

usage: python tools/ntuple_td.py [--envs N] [--pieces K] [--alpha A] [--eval K]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
from gym_simpletetris_amd import NTupleNet, TetrisBatch, _lib as C, td_update  # noqa: E402


def lines_per_piece(b, table, w, k):
    """Mean lines per piece and episode ends over k pieces from a reset: the
    rounds of play_ntuple by hand, so that the chosen slot's LINES row can be
    summed on the way."""
    b.reset()
    lines = torch.zeros((), dtype=torch.int64, device=b.device)
    ends = torch.zeros((), dtype=torch.int64, device=b.device)
    for _ in range(k):
        c = b.policy_ntuple(table, weights=w, dead_value=-100.0)
        lines += c.lines.sum()
        ends += b.step_placements(c.slots, obs="none")[2].sum()
    return {"lines_per_piece": round(int(lines) / (b.n * k), 4), "episode_ends": int(ends), "pieces": b.n * k}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--pieces", type=int, default=2000)
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--eval", type=int, default=200)
    args = ap.parse_args()
    n, W, H = args.envs, 10, 20
    b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    net = NTupleNet.systematic(W, H, 3, 3)
    b.set_ntuple(net)
    table = net.new_table(b.device)
    w = torch.zeros((1, C.AFTER_NFEAT), dtype=torch.float32, device=b.device)
    w[0, C.AFTER["reward"]] = 1.0  # score = r + V(s')
    res = {"envs": n, "network": {"tuples": len(net), "table_len": net.table_len}, "alpha": args.alpha,
           "before": lines_per_piece(b, table, w, args.eval)}
    b.reset()
    prev_index, prev_value = None, None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.pieces):
        c = b.policy_ntuple(table, weights=w, dead_value=-100.0, index=True)
        if prev_index is not None:
            # the target of the afterstate before: this placement's reward and value (no slot: nothing to learn from)
            target = torch.where(c.slots >= 0, c.reward.to(torch.float32) + c.values, prev_value)
            td_update(table, prev_index, target - prev_value, args.alpha / (len(net) * n))
        # an afterstate that ends the game has -1 rows: nothing is updated for it, and the next episode starts afresh
        prev_index, prev_value = c.index.clone(), c.values.clone()
        b.step_placements(c.slots, obs="none")
    torch.cuda.synchronize()
    res["train"] = {"pieces": n * args.pieces, "seconds": round(time.perf_counter() - t0, 2),
                    "table_abs_mean": round(float(table.abs().mean()), 5)}
    res["after"] = lines_per_piece(b, table, w, args.eval)
    b.close()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
