"""Routes in the oracle's terms (simpletetris.h, "Routes"), shared by
test_cpu_routes.py and test_gpu_routes.py.  A plain module imported by name,
like reach_ref.py; it runs no engine code and needs no GPU.

For one env the piece-state graph (rot, x, y, l) is explored once from the
start state with reach_ref's helpers, every transition one oracle step.  D(x),
the length of the shortest sequence from x that locks at a target, comes from a
backward relaxation over that graph; the route is the walk that takes, at each
state, the lowest-numbered action whose successor has D one lower (for D = 1:
that locks at the target).
"""
import numpy as np

import feature_ref as FR
import placement_ref as PR
import reach_ref as R
from oracle import oracle as O

ROUTE_MAX, ROUTE_WORDS, FIELDS = 42, 2, 21
NONE_WORD = (1 << 63) - 1  # every field 7, bit 63 clear


def pack(actions):
    """The header's encoding of a route, as Python ints [ROUTE_WORDS]."""
    words = [NONE_WORD] * ROUTE_WORDS
    for i, a in enumerate(actions[:ROUTE_MAX]):
        words[i // FIELDS] ^= (7 - int(a)) << (3 * (i % FIELDS))
    return words


def explore(h, hf, board_u8, sid, rot, x, y, l):
    """{state: [(next state or None, lock position or None)] * 7} of every
    state the start can come to.  h, hf: reach_ref.helpers()."""
    h.load(board_u8, sid)
    hf.load(board_u8, sid)
    trans, todo = {}, [(rot, x, y, l)]
    while todo:
        st = todo.pop()
        if st in trans:
            continue
        r0, x0, y0, l0 = st
        out = []
        for a in range(7):
            r1, x1, y1, l1, locked, _ = h.step(r0, x0, y0, l0, a)
            if locked:  # where: from the helper that never locks (reach_ref.search holds the two together)
                out.append((None, hf.step(r0, x0, y0, 0, a)[:3]))
            else:
                out.append(((r1, x1, y1, l1), None))
                todo.append((r1, x1, y1, l1))
        trans[st] = out
    return trans


def reverse(trans):
    """preds {state: its predecessors}, lockers {lock position: the states
    with an action that locks there}."""
    preds, lockers = {}, {}
    for st, out in trans.items():
        for nx, w in out:
            if nx is None:
                lockers.setdefault(w, set()).add(st)
            else:
                preds.setdefault(nx, set()).add(st)
    return preds, lockers


def distances(preds, lockers, target):
    """D of every explored state that can lock at target = (rot, x, y), by
    backward relaxation: layer 1 holds the states with an action that locks
    there, layer k the predecessors of layer k - 1 that no earlier layer holds."""
    D = {}
    layer = set(lockers.get(target, ()))
    k = 1
    while layer:
        for st in layer:
            D[st] = k
        k += 1
        layer = {p for st in layer for p in preds.get(st, ()) if p not in D}
    return D


def walk(trans, D, start, target):
    """The route from start: at each state the lowest action one layer nearer."""
    acts, st = [], start
    while True:
        d = D[st]
        for a, (nx, w) in enumerate(trans[st]):
            if (w == target) if d == 1 else (nx is not None and D.get(nx) == d - 1):
                break
        else:
            raise AssertionError(("no action leads nearer", st, d))
        acts.append(a)
        if d == 1:
            return acts
        st = nx


class EnvRoutes:
    """One env's graph, and the route to any of its slots."""

    def __init__(self, h, hf, board_u8, sid, rot, x, y, l):
        self.board = board_u8.astype(bool)
        self.W = self.board.shape[0]
        self.start = (rot, x, y, l)
        self.valid, self.Y = R.landings(self.board, min(sid, 6))
        self.trans = explore(h, hf, board_u8, min(sid, 6), rot, x, y, l)
        self.preds, self.lockers = reverse(self.trans)

    def target(self, slot):
        per = self.W + 6
        return (slot // per, slot % per - 3, int(self.Y[slot]))

    def route(self, slot):
        """The actions of the route to `slot`; [] if it cannot be served."""
        if not 0 <= slot < 4 * (self.W + 6) or not self.valid[slot]:
            return []
        tgt = self.target(slot)
        D = distances(self.preds, self.lockers, tgt)
        return walk(self.trans, D, self.start, tgt) if self.start in D else []

    def steps(self):
        """steps int32 [S]: st_reachable's distances, from this graph."""
        out = np.zeros(4 * (self.W + 6), np.int32)
        for s in np.flatnonzero(self.valid):
            out[s] = distances(self.preds, self.lockers, self.target(int(s))).get(self.start, 0)
        return out


def env_routes(h, hf, ob, i):
    e = ob.envs[i]
    return EnvRoutes(h, hf, ob.board(i), e.shape_id, e.rot, e.ax, e.ay, e.lock)


def iterate_first(h, hf, board_u8, sid, rot, x, y, l, slot, Y):
    """The header's definition, literally: reach_ref.search's lowest first
    action for the slot's landing, one oracle step, and again until the piece
    locks.  Returns the actions and where the piece locked."""
    W = board_u8.shape[0]
    per = W + 6
    tgt = (slot // per, slot % per - 3, int(Y))
    acts = []
    while True:
        locks, _ = R.search(h, hf, board_u8, sid, rot, x, y, l)
        n, mask = locks[tgt]
        a = (mask & -mask).bit_length() - 1
        acts.append(a)
        where = hf.step(rot, x, y, 0, a)[:3]
        rot, x, y, l, locked, _ = h.step(rot, x, y, l, a)
        if locked:
            assert n == 1, ("locked early", n)
            return acts, where
        assert n > 1, "the route did not lock on its last step"


def slot_rows(hp, ob, i, features):
    """feat int32 [rows, S] of oracle env i (placement_ref / feature_ref)."""
    e = ob.envs[i]
    board = ob.board(i).astype(bool)
    if features == "bcts":
        return FR.slot_features_bcts(hp, board, e.shape_id, e.holes, e.piece_height)
    return PR.slot_features(hp, board, e.shape_id, e.holes, e.piece_height)


def play_routed(ob, kw, weights, k, features="base", autoreset="same_step"):
    """The header's loop by hand on an OracleBatch (moved in place): per step
    reward int32 [k, n] and done uint8 [k, n], pieces int32 [n], and `planned`:
    (env, step of the last action, slot, position the piece locked at, the
    slot's landing) of every route played to its end."""
    n = ob.n
    w = np.asarray(weights, np.float32)
    w = w[None] if w.ndim == 1 else w
    h, hf = R.helpers(kw)
    hp = PR.helper_oracle(kw)
    plan = [[] for _ in range(n)]
    slot_of = [-1] * n
    land_of = [None] * n
    rew, done = np.zeros((k, n), np.int32), np.zeros((k, n), np.uint8)
    pieces, planned = np.zeros(n, np.int32), []
    for t in range(k):
        for e in range(n):
            if not plan[e]:
                er = env_routes(h, hf, ob, e)
                feat = slot_rows(hp, ob, e, features)
                slot, _ = FR.choose(w[e % len(w)], feat, allowed=er.steps())
                plan[e] = er.route(slot)[:ROUTE_MAX] if slot >= 0 else []
                slot_of[e], land_of[e] = slot, er.target(slot) if slot >= 0 else None
            last = len(plan[e]) == 1
            a = plan[e].pop(0) if plan[e] else 2
            where = hf_position(hf, ob, e, a) if last else None
            _, rew[t, e], d, _ = ob.step_one(e, a)
            done[t, e] = d
            if last:
                pieces[e] += 1
                planned.append((e, t, slot_of[e], where, land_of[e]))
            if d and autoreset == "same_step":
                ob.reset(e)
    return dict(reward=rew, done=done, pieces=pieces, planned=planned)


def hf_position(hf, ob, e, a):
    """Where env e's piece stands after action a if it does not lock (the
    helper that never locks): the lock position of a locking step."""
    env = ob.envs[e]
    hf.load(ob.board(e), env.shape_id)
    return hf.step(env.rot, env.ax, env.ay, 0, a)[:3]
