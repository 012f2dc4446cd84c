"""Time st_policy_ntuple / st_play_ntuple / st_ntuple_eval against the linear
player and against the only route to an n-tuple player there was before them.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30).  Each
workload is timed with device events over enough calls to fill about a quarter
of a second, four rounds alternating the workloads in one process, after a
warm-up; reported are the rounds' us and their median.  Networks: the
systematic 3x3 with a table per position (144 tuples, 295 KB) and the
systematic 2x4 with one shared table and mirror images (306 tuples, 1 KB).

  policy_ntuple_<net>_<set>   policy_ntuple, slots / actions / scores / feat / values, one weight row
  policy_ntuple_<net>_index   the same (base rows) with the index rows [T, n] too
  play_ntuple_<net>_<set>     us per PIECE of play_ntuple(k=100)
  ntuple_eval_<net>           ntuple_eval of the envs' own boards
  policy_linear_<set>         policy_linear of the same set (all four outputs)
  afterstates_<set>           afterstates(boards=False)
  policy_lookahead_base, play_linear_base   the older players (for the A/B across libraries)
  route_<net>_<set>           the route without the kernel: afterstates(boards=True), then per tuple the
                              index from the board words, the gather and the add in torch over [n, S],
                              the chain of the rows, S1 + V, the first maximum over the valid slots, and
                              placement_actions.

`route_choices_equal`: the route's slots equal the kernel's.  `held_against`:
  (a) policy_ntuple_<net>_<set> is below the fastest round of route_<net>_<set> by more than the rounds' spread
      (the largest max - min of the two workloads' rounds);
  (b) is decided across processes (policy_linear_base, policy_lookahead_base and play_linear_base through the
      library before and after: --only ... with ST_LIB and ST_AB_OLD_ABI=1), not here.
`per_tuple`: policy_ntuple / policy_linear, and (policy_ntuple - policy_linear) / T in us.

usage: python tools/ntuple_bench.py [--envs N] [--age STEPS] [--seconds S] [--only NAME ...]
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

DEAD = -1.0e6


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def chain(w, feat):
    """The float32 chain over feat int32 [n, R, S] with one weight row w [R]."""
    acc = torch.zeros(feat.shape[0], feat.shape[2], dtype=torch.float32, device=feat.device)
    for r in range(feat.shape[1]):
        acc = acc + w[r] * feat[:, r].to(torch.float32)
    return acc


class Route:
    """The n-tuple choice from afterstates(boards=True) and torch ops."""

    def __init__(self, b, net, table, fs, w):
        self.b, self.tuples, self.table, self.fs, self.w = b, net.tuples.tolist(), table, fs, w
        n, W, S, dev = b.n, b.width, b.n_slots, b.device
        self.feat = torch.empty((n, w.shape[1], S), dtype=torch.int32, device=dev)
        self.brd = torch.empty((n, W, S), dtype=torch.int32, device=dev)
        self.idx = torch.arange(S, device=dev)[None].expand(n, S)
        self.slots = None

    def __call__(self):
        b = self.b
        n, S = b.n, b.n_slots
        a = b.afterstates(boards=True, out=(self.feat, self.brd), features=self.fs)
        acc = torch.zeros((n, S), dtype=torch.float32, device=b.device)
        for x, y, w, h, flip, base in self.tuples:
            at = None
            for i in range(w):
                part = ((a.boards[:, x + (w - 1 - i if flip else i)] >> y) & ((1 << h) - 1)) << (i * h)
                at = part if at is None else at | part
            acc = acc + self.table[(at + base).long()]
        valid, dead = a.feat[:, C.AFTER["valid"]] != 0, a.feat[:, C.AFTER["dead"]] != 0
        tot = chain(self.w[0], a.feat) + torch.where(dead, torch.full_like(acc, DEAD), acc)
        masked = torch.where(valid, tot, torch.full_like(tot, -float("inf")))
        top = masked.max(dim=1, keepdim=True).values
        self.slots = torch.where(valid & (masked == top), self.idx, torch.full_like(self.idx, S)).min(dim=1).values
        self.slots = torch.where(self.slots == S, torch.full_like(self.slots, -1), self.slots).to(torch.int32)
        b.placement_actions(self.slots)
        return self.slots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--age", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--only", nargs="*", default=None, help="workload names (default: all)")
    args = ap.parse_args()
    n, W, H, K = args.envs, 10, 20, 100
    new = hasattr(C.load(), "st_policy_ntuple")  # (a library from before the calls: the older workloads only)

    b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    S, dev = b.n_slots, b.device

    def outs(rows):
        return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                torch.empty(n, dtype=torch.float32, device=dev), torch.empty((rows, n), dtype=torch.int32, device=dev))
    o = {"base": outs(11), "bcts": outs(18)}
    wts = {"base": torch.as_tensor(weight_rows(GREEDY_WEIGHTS), device=dev),
           "bcts": torch.as_tensor(weight_rows(BCTS_WEIGHTS, "bcts"), device=dev)}
    ret = torch.zeros(n, dtype=torch.int64, device=dev)
    eps = torch.zeros(n, dtype=torch.int32, device=dev)
    la4 = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
    af = {fs: torch.empty((n, rows, S), dtype=torch.int32, device=dev) for fs, rows in (("base", 11), ("bcts", 18))}
    work = {}
    for fs in ("base", "bcts"):
        work["policy_linear_" + fs] = (lambda fs=fs: b.policy_linear(wts[fs], out=o[fs], features=fs), 1)
        work["afterstates_" + fs] = (lambda fs=fs: b.afterstates(boards=False, out=(af[fs], None), features=fs), 1)
    work["policy_lookahead_base"] = (lambda: b.policy_lookahead(wts["base"], first_weights=wts["base"], out=la4), 1)
    work["play_linear_base"] = (lambda: b.play_linear(wts["base"], K, returns=ret, episodes=eps), K)
    res = {"envs": n, "board": [W, H], "slots": S, "aged_steps": args.age, "lib": C.LIB_PATH,
           "device": torch.cuda.get_device_name(dev)}
    nets, tables, routes = {}, {}, {}
    if new:
        from gym_simpletetris_amd import NTupleNet
        nets = {"3x3": NTupleNet.systematic(W, H, 3, 3), "2x4sm": NTupleNet.systematic(W, H, 2, 4, share=True, mirror=True)}
        gen = torch.Generator(device="cpu").manual_seed(11)
        val = torch.empty(n, dtype=torch.float32, device=dev)
        res["networks"] = {k: {"tuples": len(v), "table_bytes": 4 * v.table_len} for k, v in nets.items()}
        equal = {}
        for name, net in nets.items():
            tables[name] = ((torch.rand(net.table_len, generator=gen) * 2 - 1) *
                            10.0 ** torch.randint(-2, 3, (net.table_len,), generator=gen)).to(dev)
            index = torch.empty((len(net), n), dtype=torch.int32, device=dev)

            def use(name=name, net=net):  # the context holds one network: the workload sets its own when it differs
                if b._ntuple is not net:
                    b.set_ntuple(net)
                return tables[name]
            for fs in ("base", "bcts"):
                work[f"policy_ntuple_{name}_{fs}"] = (lambda fs=fs, use=use: b.policy_ntuple(
                    use(), weights=wts[fs], dead_value=DEAD, features=fs, out=o[fs] + (val,)), 1)
                work[f"play_ntuple_{name}_{fs}"] = (lambda fs=fs, use=use: b.play_ntuple(
                    use(), K, weights=wts[fs], dead_value=DEAD, features=fs, returns=ret, episodes=eps, obs="none"), K)
                routes[(name, fs)] = Route(b, net, tables[name], fs, wts[fs])
                work[f"route_{name}_{fs}"] = (routes[(name, fs)], 1)
                c = b.policy_ntuple(use(), weights=wts[fs], dead_value=DEAD, features=fs)
                equal[f"{name}_{fs}"] = bool(torch.equal(routes[(name, fs)](), c.slots))
            work[f"policy_ntuple_{name}_index"] = (lambda use=use, index=index: b.policy_ntuple(
                use(), weights=wts["base"], dead_value=DEAD, index=True, out=o["base"] + (val, index)), 1)
            work[f"ntuple_eval_{name}"] = (lambda use=use: b.ntuple_eval(use(), out=(val, None)), 1)
        res["route_choices_equal"] = equal
    if args.only:
        work = {k: work[k] for k in args.only}
    reps = {}
    for k, (fn, per) in work.items():  # warm-up, and calls per quarter second
        slow = per > 1 or k.startswith("route")
        timed(fn, 1 if slow else 3)
        us = timed(fn, 2 if slow else 20)
        reps[k] = max(2 if slow else 20, int(args.seconds / args.rounds * 1e6 / us))
    runs = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, (fn, per) in work.items():
            runs[k].append(timed(fn, reps[k]) / per)
    b.close()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in runs.items()}
    res["calls_per_round"] = reps
    res["workloads"] = {k: {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2)} for k in work}
    held, per_tuple = {}, {}
    for name, net in nets.items():
        for fs in ("base", "bcts"):
            nt, rt, pl = f"policy_ntuple_{name}_{fs}", f"route_{name}_{fs}", "policy_linear_" + fs
            if nt in med and rt in med:
                spread = max(max(runs[nt]) - min(runs[nt]), max(runs[rt]) - min(runs[rt]))
                held[f"(a) {nt} {round(med[nt], 1)} < fastest round of {rt} {round(min(runs[rt]), 1)} - spread "
                     f"{round(spread, 1)}"] = "reached" if med[nt] < min(runs[rt]) - spread else "not reached"
            if nt in med and pl in med:
                per_tuple[f"{nt} / {pl}"] = round(med[nt] / med[pl], 2)
                per_tuple[f"({nt} - {pl}) / {len(net)} tuples, us"] = round((med[nt] - med[pl]) / len(net), 3)
    res["held_against"], res["per_tuple"] = held, per_tuple
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
