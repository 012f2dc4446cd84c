"""Time the ST_FEATS_BCTS feature set (afterstates / policy_linear /
play_linear with features='bcts', policy_linear's `allowed` mask) against the
base set and against what a Dellacherie / BCTS player had before it.

65,536 envs, 10x20, states aged 300 steps by policy_greedy(explore=30).  Each
workload is timed with device events over enough calls to fill about a
quarter of a second, four rounds alternating the workloads in one process,
after a warm-up; reported are the rounds' us and their median.

  afterstates_base / _bcts        afterstates(boards=False), 11 / 18 rows
  afterstates_base_set            the base set through st_afterstates_set
  policy_linear_base / _bcts      all four outputs, one weight row
  policy_linear_base_set          the base set through st_policy_linear_set (no mask)
  policy_linear_bcts_allowed      features='bcts', allowed = reachable().steps
  policy_linear_base_allowed      the base set with the same mask (the new kernel's base instantiation)
  play_base / play_bcts           us per PIECE of play_linear(k=100, placements=True)
  play_base_set                   the base set through st_play_linear_set
  parent_boards_torch             afterstates(boards=True) -> the seven rows by torch ops over the board
                                  words: the only route to these rows before this feature set

The torch rows are compared with the kernel's (`torch_rows_equal`).  The play
workloads advance the envs; the players with autoreset keep them mid-game.
`held_against` states, as reached or not reached:
  (a) the base set through the _set entry points is no slower than the old
      entry points, within the spread (max - min) of the old ones' four rounds;
  (b) afterstates(features='bcts', boards=False) is faster than
      parent_boards_torch by more than that spread.
`players`: lines cleared per piece and deaths over play at placement level,
100 pieces from a reset, for GREEDY / DELLACHERIE / BCTS weights (information).

usage: python tools/features_bench.py [--envs N] [--age STEPS] [--seconds S] [--only NAME ...]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gym-simpletetris_amd"))
from gym_simpletetris_amd import BCTS_WEIGHTS, DELLACHERIE_WEIGHTS, GREEDY_WEIGHTS, TetrisBatch, _lib as C  # noqa: E402
from gym_simpletetris_amd.engine import _ptr, weight_rows  # noqa: E402

# the piece table (T J L Z S I O) and its rotation rule, as in csrc/st_kernels.hip's core (kShapes)
SHAPES = (((0, 0), (-1, 0), (1, 0), (0, -1)), ((0, 0), (-1, 0), (0, -1), (0, -2)),
          ((0, 0), (1, 0), (0, -1), (0, -2)), ((0, 0), (-1, 0), (0, -1), (1, -1)),
          ((0, 0), (-1, -1), (0, -1), (1, 0)), ((0, 0), (0, -1), (0, -2), (0, -3)),
          ((0, 0), (0, -1), (-1, 0), (-1, -1)))


def cell_table(dev):
    """int64 [7, 4 rotations, 4 cells, 2]: (dx, dy) of every cell."""
    t = []
    for cells in SHAPES:
        rots = []
        for _ in range(4):
            rots.append(cells)
            cells = tuple((j, -i) for i, j in cells)
        t.append(rots)
    return torch.tensor(t, dtype=torch.int64, device=dev)


def popc(x):
    """Set bits of every int32 word (non-negative, below 2^29)."""
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) >> 24) & 0xFF


def torch_rows(boards, feat, board, ids, W, H, cells):
    """The seven extension rows int32 [n, 7, S] from afterstates(boards=True):
    boards int32 [n, W, S], its feat [n, 11, S], the envs' board words [W, n]
    and piece ids [n]."""
    n, _, S = boards.shape
    dev = boards.device
    hm = (1 << H) - 1
    valid = feat[:, C.AFTER["valid"]]
    wall = torch.full((n, 1, S), hm, dtype=torch.int32, device=dev)
    left, right = torch.cat((wall, boards[:, :-1]), 1), torch.cat((boards[:, 1:], wall), 1)
    row_trans = popc(left ^ boards).sum(1) + popc(boards[:, -1] ^ hm)
    wf = boards | (1 << H)
    col_trans = popc((wf ^ (wf >> 1)) & hm).sum(1)
    m = ~boards & left & right & hm
    wells = torch.zeros((n, S), dtype=torch.int32, device=dev)
    for _ in range(H):
        wells += popc(m).sum(1)
        m = m & (m << 1)
    top = boards & -boards
    hole = ~boards & hm & ~(top | (top - 1))
    hole_or = torch.zeros((n, S), dtype=torch.int32, device=dev)
    for c in range(W):
        hole_or |= hole[:, c]
    depth = torch.zeros((n, S), dtype=torch.int32, device=dev)
    for y in range(1, H):
        depth += (((hole >> y) & 1) * popc(boards & ((1 << y) - 1))).sum(1)
    # the piece: its cells per slot, the rows they span, and the cells in rows the placement filled
    per = W + 6
    s = torch.arange(S, device=dev)
    rot, x = s // per, s % per - 3
    cl = cells[ids.long()][:, rot]                        # [n, S, 4, 2]
    y = feat[:, C.AFTER["y"]].long()
    col, row = x[None, :, None] + cl[..., 0], y[:, :, None] + cl[..., 1]
    inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    bits = (board.T.long()[:, :, None] >> torch.arange(H, device=dev)) & 1   # [n, W, H]
    fill = bits.sum(1)                                                       # cells per row before the piece
    rowc = row.clamp(0, H - 1)
    same = (rowc[..., :, None] == rowc[..., None, :]) & inside[..., None, :]
    after = torch.gather(fill[:, None, :].expand(n, S, H), 2, rowc) + same.sum(-1)
    gone = (inside & (after == W)).sum(-1)
    landing2 = 2 * H - 1 - (row.min(-1).values + row.max(-1).values)
    eroded = feat[:, C.AFTER["lines"]] * gone
    rows = torch.stack((landing2, eroded, row_trans, col_trans, wells, depth, popc(hole_or)), 1)
    return (rows * valid[:, None]).to(torch.int32)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # us per call


def players(n, W, H, k):
    """Lines per piece and deaths of the three published weight sets."""
    out = {}
    for name, w, fs in (("GREEDY_WEIGHTS", GREEDY_WEIGHTS, "base"), ("DELLACHERIE_WEIGHTS", DELLACHERIE_WEIGHTS, "bcts"),
                        ("BCTS_WEIGHTS", BCTS_WEIGHTS, "bcts")):
        b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                        validate_actions=False)
        b.reset()
        wt = torch.as_tensor(weight_rows(w, fs), device=b.device)
        lines = torch.zeros((), dtype=torch.int64, device=b.device)
        deaths = torch.zeros((), dtype=torch.int64, device=b.device)
        for _ in range(k):
            c = b.policy_linear(wt, features=fs)
            _, _, d = b.step_placements(c.slots, obs="none")
            lines += c.lines.sum()
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
    b = TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[1000 + e for e in range(n)],
                    validate_actions=False)
    b.reset()
    for t in range(args.age):
        b.step(b.policy_greedy(t, seed=3, explore=30), obs="none")
    S, dev = b.n_slots, b.device
    L, ctx, stream = b._L, b._ctx, b._stream
    f11 = torch.empty((n, 11, S), dtype=torch.int32, device=dev)
    f18 = torch.empty((n, 18, S), dtype=torch.int32, device=dev)
    brd = torch.empty((n, W, S), dtype=torch.int32, device=dev)

    def outs(rows):
        return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                torch.empty(n, dtype=torch.float32, device=dev), torch.empty((rows, n), dtype=torch.int32, device=dev))
    o11, o18 = outs(11), outs(18)
    w11 = torch.as_tensor(weight_rows(GREEDY_WEIGHTS), device=dev)
    w18 = torch.as_tensor(weight_rows(BCTS_WEIGHTS, "bcts"), device=dev)
    ret = torch.zeros(n, dtype=torch.int64, device=dev)
    eps = torch.zeros(n, dtype=torch.int32, device=dev)
    steps = b.reachable(first=False).steps
    cells = cell_table(dev)
    st = b.state_tensors(("board", "piece"))
    board, ids = st["board"][:, :n].clone(), (st["piece"][:n] & 7).clone()

    def parent():
        a = b.afterstates(boards=True, out=(f11, brd))
        return torch_rows(a.boards, a.feat, board, ids, W, H, cells)

    equal = bool(torch.equal(parent(), b.afterstates(boards=False, features="bcts").feat[:, 11:]))

    def base_set_policy():
        C.check(L.st_policy_linear_set(ctx, 0, _ptr(w11), 1, None, *(_ptr(t) for t in o11), stream()))

    def base_set_play():
        C.check(L.st_play_linear_set(ctx, 0, _ptr(w11), 1, K, 1, _ptr(ret), _ptr(eps), None, _ptr(b.reward),
                                     _ptr(b.done), stream()))

    work = {
        "afterstates_base": (lambda: b.afterstates(boards=False, out=(f11, None)), 1),
        "afterstates_base_set": (lambda: C.check(L.st_afterstates_set(ctx, 0, _ptr(f11), None, stream())), 1),
        "afterstates_bcts": (lambda: b.afterstates(boards=False, out=(f18, None), features="bcts"), 1),
        "policy_linear_base": (lambda: b.policy_linear(w11, out=o11), 1),
        "policy_linear_base_set": (base_set_policy, 1),
        "policy_linear_bcts": (lambda: b.policy_linear(w18, out=o18, features="bcts"), 1),
        "policy_linear_bcts_allowed": (lambda: b.policy_linear(w18, out=o18, features="bcts", allowed=steps), 1),
        "policy_linear_base_allowed": (lambda: b.policy_linear(w11, out=o11, allowed=steps), 1),
        "parent_boards_torch": (parent, 1),
        "play_base": (lambda: b.play_linear(w11, K, returns=ret, episodes=eps, placements=True), K),
        "play_base_set": (base_set_play, K),
        "play_bcts": (lambda: b.play_linear(w18, K, returns=ret, episodes=eps, placements=True, features="bcts"), K),
    }
    if args.only:
        work = {k: work[k] for k in args.only}
    reps = {}
    for k, (fn, per) in work.items():  # warm-up, and calls per quarter second
        timed(fn, 3)
        us = timed(fn, 5 if per > 1 else 20)
        reps[k] = max(3 if per > 1 else 20, int(args.seconds / args.rounds * 1e6 / us))
    runs = {k: [] for k in work}
    for _ in range(args.rounds):
        for k, (fn, per) in work.items():
            runs[k].append(timed(fn, reps[k]) / per)
    b.close()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: max(v) - min(v) for k, v in runs.items()}
    res = {"envs": n, "board": [W, H], "slots": S, "aged_steps": args.age, "lib": C.LIB_PATH,
           "device": torch.cuda.get_device_name(dev), "calls_per_round": reps, "torch_rows_equal": equal,
           "workloads": {k: {"us": [round(x, 2) for x in runs[k]], "median_us": round(med[k], 2)} for k in work}}
    held = {}
    for old, new in (("afterstates_base", "afterstates_base_set"), ("policy_linear_base", "policy_linear_base_set"),
                     ("play_base", "play_base_set")):
        if old in med and new in med:
            held[f"(a) {new} <= {old} + spread {round(spread[old], 2)}"] = \
                "reached" if med[new] <= med[old] + spread[old] else "not reached"
    if "afterstates_bcts" in med and "parent_boards_torch" in med:
        s = max(spread.get("afterstates_base", 0.0), spread["afterstates_bcts"])
        held[f"(b) afterstates_bcts + spread {round(s, 2)} < parent_boards_torch"] = \
            "reached" if med["afterstates_bcts"] + s < med["parent_boards_torch"] else "not reached"
    res["held_against"] = held
    cost = {}
    for base, ext in (("afterstates_base", "afterstates_bcts"), ("policy_linear_base", "policy_linear_bcts"),
                      ("play_base", "play_bcts"), ("policy_linear_bcts", "policy_linear_bcts_allowed")):
        if base in med and ext in med:
            cost[f"{ext} - {base}"] = round(med[ext] - med[base], 2)
    res["cost_us"] = cost
    if not args.no_players:
        res["players"] = players(n, W, H, K)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
