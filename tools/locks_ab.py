"""One timing of the entry points that st_locks's translation unit must leave
as they were -- reachable(first=False), policy_linear, policy_routed (all envs)
and play_routed(k=100), both feature sets -- through the library ST_LIB names
(ST_AB_OLD_ABI=1 for a build that predates st_lock_set).  Run it in alternated
processes, one library each, and compare the lines.

65,536 envs, 10x20, aged 300 greedy steps; device events over a quarter of a
second a workload, after a warm-up.

usage: ST_LIB=lib.so python tools/locks_ab.py [label]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from afterstates_bench import timed  # noqa: E402
from gym_simpletetris_amd import BCTS_WEIGHTS, GREEDY_WEIGHTS, TetrisBatch, _lib as C  # noqa: E402


def main():
    n, K = 65536, 100
    b = TetrisBatch(n, width=10, height=20, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(300):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    aged = b.save()
    S, dev = b.n_slots, b.device
    steps = torch.empty((n, S), dtype=torch.int32, device=dev)
    lin_out = (torch.empty(n, dtype=torch.int32, device=dev), None, None, None)
    p_out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty((C.ROUTE_WORDS, n), dtype=torch.int64, device=dev),
             torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    wb, wx = b._weights(GREEDY_WEIGHTS, "base"), b._weights(BCTS_WEIGHTS, "bcts")
    work = {
        "reachable_steps": (lambda: b.reachable(first=False, out=(steps, None)), 1),
        "policy_linear_base": (lambda: b.policy_linear(wb, out=lin_out), 1),
        "policy_linear_bcts": (lambda: b.policy_linear(wx, out=lin_out, features="bcts"), 1),
        "policy_routed_base": (lambda: b.policy_routed(wb, out=p_out), 1),
        "policy_routed_bcts": (lambda: b.policy_routed(wx, features="bcts", out=p_out), 1),
        "play_routed_base_per_step": (lambda: b.play_routed(wb, K, obs="none"), K),
        "play_routed_bcts_per_step": (lambda: b.play_routed(wx, K, features="bcts", obs="none"), K),
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
