"""One timing of the entry points that st_routes's translation unit must leave
as they were -- reachable(first=False), reachable(), policy_linear (both
feature sets, with a mask) and play_linear(k=100) -- through the library ST_LIB
names (ST_AB_OLD_ABI=1 for a build that predates st_routes).  Run it in
alternated processes, one library each, and compare the lines.

65,536 envs, 10x20, aged 300 greedy steps; device events over a quarter of a
second a workload, after a warm-up.

usage: ST_LIB=lib.so python tools/routed_ab.py [label]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from afterstates_bench import timed  # noqa: E402
from gym_simpletetris_amd import BCTS_WEIGHTS, GREEDY_WEIGHTS, TetrisBatch  # noqa: E402


def main():
    n, K = 65536, 100
    b = TetrisBatch(n, width=10, height=20, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(300):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    aged = b.save()
    S = b.n_slots
    steps = torch.empty((n, S), dtype=torch.int32, device=b.device)
    first = torch.empty((n, S), dtype=torch.uint8, device=b.device)
    lin_out = (torch.empty(n, dtype=torch.int32, device=b.device), None, None, None)
    wb, wx = b._weights(GREEDY_WEIGHTS, "base"), b._weights(BCTS_WEIGHTS, "bcts")
    b.reachable(first=False, out=(steps, None))
    work = {
        "reachable_steps": (lambda: b.reachable(first=False, out=(steps, None)), 1),
        "reachable_first": (lambda: b.reachable(out=(steps, first)), 1),
        "policy_linear_base": (lambda: b.policy_linear(wb, out=lin_out), 1),
        "policy_linear_bcts_allowed": (lambda: b.policy_linear(wx, out=lin_out, features="bcts", allowed=steps), 1),
        "play_linear_base_per_step": (lambda: b.play_linear(wb, K), K),
        "play_linear_bcts_per_step": (lambda: b.play_linear(wx, K, features="bcts"), K),
    }
    out = {"label": sys.argv[1] if len(sys.argv) > 1 else os.environ.get("ST_LIB", "in-tree")}
    for k, (fn, div) in work.items():
        b.load(aged)
        timed(fn, 1)
        us = timed(fn, 2)
        b.load(aged)
        torch.cuda.synchronize()
        out[k] = round(timed(fn, max(2, int(0.25e6 / us))) / div, 2)
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
