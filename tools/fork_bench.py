"""Time st_fork beside the routes of the parent commit, and play the rollout
player out.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30), copied
into a second batch of the same size.  Workloads, each timed with device events
over enough calls to fill its share of --seconds, four rounds alternating the
workloads in one process, after a warm-up:
  fork_identity / fork_random / fork_groups64   the deep copy: into the second
      batch with the NULL index, with a random index, and fork_groups(64) in
      place; each once per grid of the deep copy (ST_FORK_WAVES = 1, the
      library's choice, and 4 waves per 64 envs), and each with keep_rng=True;
  st_copy_route   the parent's whole-batch device copy: three st_copy calls
      over the board, stats and mt views;
  host_route      the parent's only per-env route, get_state -> set_state
      (host clock around a call that ends in a synchronise).
Beside them the byte floor: the bytes a fork reads and writes over the rate
tools/write_bw reaches in this call.  Reported: the rounds, their median and
spread; (a) whether the deep fork's median lies below the fastest round of the
host route by more than the rounds' spread; the ratio to the st_copy route and
the share of the byte floor (no threshold).
`players`: --roots envs played for --pieces pieces each by policy_rollout
(BCTS_WEIGHTS, --horizon, --samples) and by play_linear(placements=True) from
the same seeds: lines per piece, deaths, time per decision.  lines = (return +
100 * deaths) / 100 under the default reward.

usage: python tools/fork_bench.py [--envs N] [--age STEPS] [--seconds S] [--roots R] [--pieces P]
                                  [--horizon H] [--samples M]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from afterstates_bench import timed, write_rate  # noqa: E402
from gym_simpletetris_amd import BCTS_WEIGHTS, TetrisBatch, _lib as C, search  # noqa: E402
from routed_bench import spawns  # noqa: E402


def mk(n, seed0=1000):
    b = TetrisBatch(n, width=10, height=20, autoreset="same_step", seeds=[seed0 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    return b


def host_timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def players(roots, pieces, horizon, samples):
    out = {"roots": roots, "pieces_per_root": pieces, "horizon": horizon, "samples": samples}

    def row(b, s0, ret, eps):
        n_pieces, deaths = int((spawns(b) - s0).sum()), int(eps.sum())
        lines = (int(ret.sum()) + 100 * deaths) / 100
        return {"pieces": n_pieces, "lines": lines, "lines_per_piece": round(lines / max(n_pieces, 1), 4),
                "deaths": deaths}

    root = mk(roots)
    branch = mk(roots * root.n_slots * samples, seed0=500000)
    w = root._weights(BCTS_WEIGHTS, "bcts")
    ret = torch.zeros(roots, dtype=torch.int64, device=root.device)
    eps = torch.zeros(roots, dtype=torch.int64, device=root.device)
    s0 = spawns(root)

    def decide():
        slots = search.policy_rollout(root, branch, w, horizon, samples, "bcts")
        _, r, d = root.step_placements(slots, obs="none")
        ret.add_(r)
        eps.add_(d)

    timed(decide, 2)  # warm-up (two pieces that count)
    us = timed(decide, pieces - 2)
    out["policy_rollout"] = dict(row(root, s0, ret, eps), us_per_decision=round(us, 1),
                                 branch_envs=branch.n)
    root.close()
    branch.close()
    root = mk(roots)
    s0 = spawns(root)
    timed(lambda: root.play_linear(w, 2, placements=True, features="bcts"), 1)
    root.close()
    root = mk(roots)
    s0 = spawns(root)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ret, eps = root.play_linear(w, pieces, placements=True, features="bcts")
    b.record()
    b.synchronize()
    out["play_linear_placements"] = dict(row(root, s0, ret, eps),
                                         us_per_decision=round(a.elapsed_time(b) * 1e3 / pieces, 1))
    root.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--roots", type=int, default=1024)
    ap.add_argument("--pieces", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--no-players", action="store_true")
    ap.add_argument("--no-write-bw", action="store_true")
    args = ap.parse_args()
    n = args.envs
    src = mk(n)
    for t in range(args.age):
        src.step(src.policy_greedy(t, seed=3, explore=30), obs="none")
    dst = mk(n, seed0=200000)
    # a copy of the aged batch that is never read back: its envs keep their previews and generation buffers
    # as play leaves them, which is what keep_rng has to put into CPython's form
    live = mk(n, seed0=300000)
    live.fork(src)
    rnd = torch.randint(0, n, (n,), device=src.device, dtype=torch.int32)
    L, s = src._L, src._stream()
    views = [(f, int(torch.tensor(src._sizes()[f]).prod()) * 4) for f in ("board", "stats", "mt")]

    def st_copy_route():
        for f, nbytes in views:
            C.check(L.st_copy(ctypes.c_void_p(dst._view_ptr(f)), ctypes.c_void_p(src._view_ptr(f)), nbytes, s))

    def host_route():
        dst.set_state(**src.get_state())

    def waves(k, fn):
        def run():
            os.environ["ST_FORK_WAVES"] = k
            fn()
        return run

    work = {}  # name -> (callable, timer)
    for k in ("1", "4"):
        work[f"fork_identity_deep_w{k}"] = (waves(k, lambda: dst.fork(src)), timed)
        work[f"fork_random_deep_w{k}"] = (waves(k, lambda: dst.fork(src, index=rnd)), timed)
        work[f"fork_groups64_deep_w{k}"] = (waves(k, lambda: dst.fork_groups(64)), timed)
    work["fork_identity_keep_rng"] = (lambda: dst.fork(src, keep_rng=True), timed)
    work["fork_random_keep_rng"] = (lambda: dst.fork(src, index=rnd, keep_rng=True), timed)
    work["fork_groups64_keep_rng"] = (lambda: dst.fork_groups(64, keep_rng=True), timed)

    def restore_then_keep():
        os.environ["ST_FORK_WAVES"] = "1"
        dst.fork(live)
        dst.fork(src, keep_rng=True)

    work["restore_live_then_keep_rng"] = (restore_then_keep, timed)
    work["st_copy_route"] = (st_copy_route, timed)
    work["host_route"] = (host_route, host_timed)

    reps = {}
    for k, (fn, tm) in work.items():  # warm-up, and calls per round
        tm(fn, 1)
        us = tm(fn, 1 if k == "host_route" else 2)
        reps[k] = 1 if k == "host_route" else max(2, int(args.seconds / args.rounds * 1e6 / us))
    runs = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, (fn, tm) in work.items():
            runs[k].append(tm(fn, reps[k]))
    os.environ.pop("ST_FORK_WAVES", None)
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    W, pitch = src.width, int(src._views.mt_pitch)
    env_bytes = (W + C.NSTAT + pitch) * 4
    deep_bytes = {"fork_identity": 2 * n * env_bytes, "fork_random": 2 * n * env_bytes + 4 * n,
                  "fork_groups64": 2 * (n - n // 64) * env_bytes + 5 * n}
    keep_bytes = 2 * (W + C.NSTAT - 1) * 4
    out = {"envs": n, "board": [10, 20], "aged_steps": args.age, "device": torch.cuda.get_device_name(src.device),
           "state_bytes_per_env": env_bytes, "calls_per_round": reps,
           "workloads": {k: {"us": [round(x, 1) for x in runs[k]], "median_us": round(med[k], 1),
                             "spread_us": round(spread[k], 1)} for k in work}}
    out["deep_copy_grid"] = {name: {"w1_us": round(med[f"{name}_deep_w1"], 1), "w4_us": round(med[f"{name}_deep_w4"], 1)}
                             for name in deep_bytes}
    # keep_rng where every written env still holds play's engine-private form (the identity fork above finds
    # them in CPython's form from the second call on): the pair less the deep copy that restores them
    out["keep_rng_on_live_envs_us"] = round(med["restore_live_then_keep_rng"] - med["fork_identity_deep_w1"], 1)
    # the library's grid is one wave per 64 envs: (a) and the ratios are stated for it
    host_fast = min(runs["host_route"])
    out["a_fork_vs_host_route"] = {}
    for name in deep_bytes:
        k = f"{name}_deep_w1"
        gap, sp = host_fast - med[k], max(spread[k], spread["host_route"])
        out["a_fork_vs_host_route"][name] = {"fork_median_us": round(med[k], 1), "host_route_fastest_us": round(host_fast, 1),
                                             "gap_us": round(gap, 1), "rounds_spread_us": round(sp, 1),
                                             "reached": bool(gap > sp), "speedup": round(host_fast / med[k], 1)}
    out["vs_st_copy_route"] = {name: round(med[f"{name}_deep_w1"] / med["st_copy_route"], 3) for name in deep_bytes}
    if not args.no_write_bw:
        tbps, detail = write_rate()
        out["write_bw"] = detail
        if tbps:
            floor = {}
            for name, nbytes in deep_bytes.items():
                f_us = nbytes / (tbps * 1e12) * 1e6
                floor[name + "_deep"] = {"bytes": nbytes, "floor_us": round(f_us, 1),
                                         "share_of_floor": round(f_us / med[f"{name}_deep_w1"], 3)}
            for name in ("fork_identity", "fork_random"):
                f_us = n * keep_bytes / (tbps * 1e12) * 1e6
                floor[name + "_keep_rng"] = {"bytes": n * keep_bytes, "floor_us": round(f_us, 2),
                                             "share_of_floor": round(f_us / med[name + "_keep_rng"], 3)}
            out["byte_floor"] = floor
    for b in (src, dst, live):
        b.close()
    torch.cuda.synchronize()
    if not args.no_players:
        out["players"] = players(args.roots, args.pieces, args.horizon, args.samples)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
