"""Time st_next_piece / st_policy_lookahead / st_play_lookahead against the
one-ply entry points and against the only two-ply route there was before them.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30).  Each
workload is timed with device events over enough calls to fill about a quarter
of a second, four rounds alternating the workloads in one process, after a
warm-up; reported are the rounds' us and their median.

  next_piece                      every env holds its preview (the steady state behind a lookahead call)
  next_piece_draw                 st_mt_sync + next_piece: every env draws (minus mt_sync alone: see cost_us)
  mt_sync                         st_mt_sync alone
  lookahead_base / _bcts          policy_lookahead, the four per-env outputs, one weight row, first_weights too
  lookahead_base_table / _bcts_table   with scores_all and slots2_all
  policy_linear_base / _bcts      policy_linear of the same set (all four outputs)
  play_lookahead_base / _bcts     us per PIECE of play_lookahead(k=100)
  play_linear_base / _bcts        us per PIECE of play_linear(k=100, placements=True)
  route_base / route_bcts         the route without the fused call: afterstates(boards=True), then for each
                                  of the S first-ply slots a scratch batch's state written on the device
                                  (st_state views + st_copy: board, piece id, holes counter) and its
                                  policy_linear, then the combine in torch.  The next piece is taken from
                                  next_piece() outside the timed region (the route has no way to it), so
                                  the route is timed in its favour.

`route_choices_equal`: the route's slots equal the kernel's.  `held_against`,
as reached or not reached:
  (a) lookahead_<set> is faster than the fastest round of route_<set>;
  (b) is decided across processes (the one-ply workloads through the library
      before and after: --only policy_linear_base ... with ST_LIB), not here.
`work_ratio`: lookahead time / (policy_linear time x mean live first-ply slots).
`players`: lines per piece and deaths over 100 pieces from a reset with
BCTS_WEIGHTS, one ply and two plies (information).

usage: python tools/lookahead_bench.py [--envs N] [--age STEPS] [--seconds S] [--only NAME ...]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
from gym_simpletetris_amd import BCTS_WEIGHTS, GREEDY_WEIGHTS, TetrisBatch, _lib as C  # noqa: E402
from gym_simpletetris_amd.engine import _ptr, weight_rows  # noqa: E402

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
    """The float32 chain over feat int32 [n, R, S] with one weight row w [R]:
    every product and every sum a torch op of its own."""
    acc = torch.zeros(feat.shape[0], feat.shape[2], dtype=torch.float32, device=feat.device)
    for r in range(feat.shape[1]):
        acc = acc + w[r] * feat[:, r].to(torch.float32)
    return acc


class Route:
    """The two-ply choice from the one-ply calls and a scratch batch."""

    def __init__(self, b, scratch, fs, w, nxt):
        self.b, self.sc, self.fs, self.w, self.nxt = b, scratch, fs, w, nxt
        n, W, S, dev = b.n, b.width, b.n_slots, b.device
        assert b.stride == n and scratch.stride == n, "the route writes whole state rows: n must be a multiple of 64"
        rows = w.shape[1]
        self.feat = torch.empty((n, rows, S), dtype=torch.int32, device=dev)
        self.brd = torch.empty((n, W, S), dtype=torch.int32, device=dev)
        self.out = (torch.empty(n, dtype=torch.int32, device=dev), None,
                    torch.empty(n, dtype=torch.float32, device=dev), None)
        self.piece = (nxt.to(torch.int32) | ((W // 2) << 5)).contiguous()
        self.slots = None

    def __call__(self):
        b, sc, L = self.b, self.sc, self.b._L
        n, W, S = b.n, b.width, b.n_slots
        a = b.afterstates(boards=True, out=(self.feat, self.brd), features=self.fs)
        s1 = chain(self.w[0], a.feat)
        valid, dead = a.feat[:, C.AFTER["valid"]] != 0, a.feat[:, C.AFTER["dead"]] != 0
        tot = torch.zeros((n, S), dtype=torch.float32, device=b.device)
        stream = b._stream()
        C.check(L.st_copy(sc._stat_ptr(C.STAT["piece"]), _ptr(self.piece), 4 * n, stream))
        for s in range(S):
            board = a.boards[:, :, s].T.contiguous()
            holes = a.feat[:, C.AFTER["holes"], s].contiguous()
            C.check(L.st_copy(ctypes.c_void_p(sc._view_ptr("board")), _ptr(board), 4 * n * W, stream))
            C.check(L.st_copy(sc._stat_ptr(C.STAT["holes"]), _ptr(holes), 4 * n, stream))
            c = sc.policy_linear(self.w, out=self.out, features=self.fs)
            tail = torch.where(dead[:, s] | (c.slots < 0), torch.full_like(c.scores, DEAD), c.scores)
            tot[:, s] = s1[:, s] + tail
        masked = torch.where(valid, tot, torch.full_like(tot, -float("inf")))
        top = masked.max(dim=1, keepdim=True).values
        idx = torch.arange(S, device=b.device)[None].expand(n, S)
        self.slots = torch.where(valid & (masked == top), idx, torch.full_like(idx, S)).min(dim=1).values
        return self.slots


def players(n, W, H, k):
    """Lines per piece and deaths with BCTS_WEIGHTS, one ply and two plies."""
    out = {}
    for name in ("one_ply", "two_ply"):
        b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                        validate_actions=False)
        b.reset()
        wt = torch.as_tensor(weight_rows(BCTS_WEIGHTS, "bcts"), device=b.device)
        lines = torch.zeros((), dtype=torch.int64, device=b.device)
        deaths = torch.zeros((), dtype=torch.int64, device=b.device)
        for _ in range(k):
            c = b.policy_linear(wt, features="bcts") if name == "one_ply" else \
                b.policy_lookahead(wt, first_weights=wt, features="bcts")
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
    args = ap.parse_args()
    n, W, H, K = args.envs, 10, 20, 100
    new = hasattr(C.load(), "st_policy_lookahead")  # (a library from before the calls: the one-ply workloads only)

    def batch():
        x = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                        validate_actions=False)
        x.reset()
        return x
    b = batch()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    S, dev = b.n_slots, b.device

    def outs(rows):
        return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                torch.empty(n, dtype=torch.float32, device=dev), torch.empty((rows, n), dtype=torch.int32, device=dev))
    o11, o18 = outs(11), outs(18)
    w11 = torch.as_tensor(weight_rows(GREEDY_WEIGHTS), device=dev)
    w18 = torch.as_tensor(weight_rows(BCTS_WEIGHTS, "bcts"), device=dev)
    ret = torch.zeros(n, dtype=torch.int64, device=dev)
    eps = torch.zeros(n, dtype=torch.int32, device=dev)
    work = {
        "policy_linear_base": (lambda: b.policy_linear(w11, out=o11), 1),
        "policy_linear_bcts": (lambda: b.policy_linear(w18, out=o18, features="bcts"), 1),
    }
    res = {"envs": n, "board": [W, H], "slots": S, "aged_steps": args.age, "lib": C.LIB_PATH,
           "device": torch.cuda.get_device_name(dev)}
    routes = {}
    if new:
        nxt = b.next_piece().clone()
        la4 = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.float32, device=dev))
        la6 = la4 + (torch.empty((n, S), dtype=torch.float32, device=dev),
                     torch.empty((n, S), dtype=torch.int32, device=dev))
        npo = torch.empty(n, dtype=torch.uint8, device=dev)
        scratch = batch()
        for fs, w in (("base", w11), ("bcts", w18)):
            routes[fs] = Route(b, scratch, fs, w, nxt)

        def draw():
            b.sync_mt()
            b.next_piece(out=npo)
        work.update({
            "next_piece": (lambda: b.next_piece(out=npo), 1),
            "mt_sync": (b.sync_mt, 1),
            "next_piece_draw": (draw, 1),
            "lookahead_base": (lambda: b.policy_lookahead(w11, first_weights=w11, out=la4), 1),
            "lookahead_base_table": (lambda: b.policy_lookahead(w11, first_weights=w11, table=True, out=la6), 1),
            "lookahead_bcts": (lambda: b.policy_lookahead(w18, first_weights=w18, features="bcts", out=la4), 1),
            "lookahead_bcts_table": (lambda: b.policy_lookahead(w18, first_weights=w18, features="bcts", table=True,
                                                                out=la6), 1),
            "route_base": (routes["base"], 1),
            "route_bcts": (routes["bcts"], 1),
        })
        # the route's choices against the kernel's, and the live first-ply slots, on the aged states
        equal = {}
        for fs, w in (("base", w11), ("bcts", w18)):
            c = b.policy_lookahead(w, first_weights=w, features=fs)
            equal[fs] = bool(torch.equal(routes[fs]().to(torch.int32), c.slots))
        feat = b.afterstates(boards=False).feat
        live = ((feat[:, C.AFTER["valid"]] != 0) & (feat[:, C.AFTER["dead"]] == 0)).sum(1).to(torch.float64).mean()
        res["route_choices_equal"] = equal
        res["mean_live_first_ply_slots"] = round(float(live), 3)
    work.update({
        "play_linear_base": (lambda: b.play_linear(w11, K, returns=ret, episodes=eps, placements=True), K),
        "play_linear_bcts": (lambda: b.play_linear(w18, K, returns=ret, episodes=eps, placements=True,
                                                   features="bcts"), K),
    })
    if new:
        work.update({
            "play_lookahead_base": (lambda: b.play_lookahead(w11, K, first_weights=w11, returns=ret, episodes=eps,
                                                             obs="none"), K),
            "play_lookahead_bcts": (lambda: b.play_lookahead(w18, K, first_weights=w18, features="bcts", returns=ret,
                                                             episodes=eps, obs="none"), K),
        })
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
    held, ratio, cost = {}, {}, {}
    for fs in ("base", "bcts"):
        la, rt, pl = "lookahead_" + fs, "route_" + fs, "policy_linear_" + fs
        if la in med and rt in med:
            fastest = min(runs[rt])
            held[f"(a) {la} {round(med[la], 1)} < fastest round of {rt} {round(fastest, 1)}"] = \
                "reached" if med[la] < fastest else "not reached"
            ratio[f"{rt} / {la}"] = round(fastest / med[la], 2)
        if la in med and pl in med and "mean_live_first_ply_slots" in res:
            ratio[f"work ratio {la} / ({pl} x live)"] = round(med[la] / (med[pl] * res["mean_live_first_ply_slots"]), 3)
        for x, y in (("play_lookahead_" + fs, "play_linear_" + fs), (la + "_table", la)):
            if x in med and y in med:
                cost[f"{x} - {y}"] = round(med[x] - med[y], 2)
    if "next_piece_draw" in med and "mt_sync" in med:
        cost["next_piece_draw - mt_sync"] = round(med["next_piece_draw"] - med["mt_sync"], 2)
    res["held_against"], res["ratios"], res["cost_us"] = held, ratio, cost
    if new and not args.no_players:
        res["players"] = players(n, W, H, K)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
