"""Reachability in the oracle's terms (simpletetris.h, "Reachability"), shared
by test_cpu_reachable.py and test_gpu_reachable.py.  A plain module imported by
name, like placement_ref.py; it runs no engine code and needs no GPU.

The expectation is a layered breadth-first search over the live piece's states
(rot, x, y, l) in which every transition is one oracle step: a one-env helper
of the case's config decides whether the step locked (its shape counts moved,
or it died) and gives the new lock counter; a second helper with
lock_delay=32766, which never locks, gives the position after the step; both
must agree on every step that does not lock.  Slot landings come from
placement_ref.occupied.
"""
import ctypes

import numpy as np

import placement_ref as P
from harness import ASEED, cached_ref
from oracle import oracle as O

NEVER_LOCKS = 32766
N = 70
BOARDS = P.BOARDS
CONFIGS = dict(P.CONFIGS, lock2=dict(lock_delay=2))  # no step_reset: the counter survives a fall
CASES = [(b, c) for b in BOARDS for c in CONFIGS]


def case_kw(board, config):
    W, H = BOARDS[board]
    return dict(width=W, height=H, **CONFIGS[config])


def case_seeds(board, config):
    base = 9000 + 100 * sorted(BOARDS).index(board) + 1000 * sorted(CONFIGS).index(config)
    return [base + e for e in range(N)]


class Helper:
    """One oracle env whose board, piece id and counters are set once
    (set_state) and restored before every step, so that a step that locked
    leaves nothing behind."""

    def __init__(self, kw):
        self.ob = O.OracleBatch(1, [1], **kw)
        self.ob.reset()
        self.size = ctypes.sizeof(O.Env)
        self.obs = np.zeros(kw["width"] * kw["height"], np.uint8)
        self.done, self.rt = ctypes.c_int32(), ctypes.c_int32()
        self.saved = [None] * 4

    def load(self, board_u8, sid):
        for rot in range(4):
            self.ob.set_state(0, board=board_u8, shape_id=sid, rot=rot, ax=0, ay=0, lock=0)
            self.saved[rot] = ctypes.string_at(ctypes.addressof(self.ob.envs[0]), self.size)

    def step(self, rot, x, y, l, a):
        """step_one(a) from (rot, x, y, l) -> (rot, x, y, l, locked, reward)."""
        e = self.ob.envs[0]
        ctypes.memmove(ctypes.addressof(e), self.saved[rot], self.size)
        e.ax, e.ay, e.lock = x, y, l
        spawned = sum(e.counts)
        rew = O.lib().or_env_step(ctypes.byref(e), int(a), self.obs.ctypes.data, ctypes.byref(self.done),
                                  ctypes.byref(self.rt))
        locked = sum(e.counts) != spawned or self.done.value != 0
        return e.rot, e.ax, e.ay, e.lock, locked, rew


def helpers(kw):
    return Helper(kw), Helper(dict(kw, lock_delay=NEVER_LOCKS))


def landings(board, sid):
    """valid bool [S] and landing row int [S] of every slot (the header's
    validity rule and hard_drop from row 0)."""
    W, H = board.shape
    per = W + 6
    valid, Y = np.zeros(4 * per, bool), np.zeros(4 * per, np.int32)
    for rot in range(4):
        cells = O.rotate_cells(O.BASE_SHAPES[sid], rot)
        for x in range(-3, W + 3):
            if P.occupied(cells, x, 0, board):
                continue
            y = 0
            while not P.occupied(cells, x, y + 1, board):
                y += 1
            valid[rot * per + x + 3], Y[rot * per + x + 3] = True, y
    return valid, Y


def search(h, hf, board_u8, sid, rot, x, y, l):
    """Layered BFS from (rot, x, y, l): {(rot, x, y): (steps, mask of the
    first actions of the shortest sequences)} of every lock position."""
    h.load(board_u8, sid)
    hf.load(board_u8, sid)
    pos = {}   # (rot, x, y, a) -> position after the step, from the helper that never locks
    seen = {(rot, x, y, l): 0}
    layer = {(rot, x, y, l): 0}  # state -> mask of first actions (0: the start itself)
    locks = {}
    d = 0
    while layer:
        nxt = {}
        for (r0, x0, y0, l0), m0 in layer.items():
            for a in range(7):
                key = (r0, x0, y0, a)
                if key not in pos:
                    pos[key] = hf.step(r0, x0, y0, 0, a)[:3]
                r1, x1, y1, l1, locked, _ = h.step(r0, x0, y0, l0, a)
                m1 = m0 if d else 1 << a
                if locked:
                    where = pos[key]
                    if where not in locks:
                        locks[where] = [d + 1, 0]
                    if locks[where][0] == d + 1:
                        locks[where][1] |= m1
                    continue
                assert (r1, x1, y1) == pos[key], ("the helpers disagree", key, (r1, x1, y1), pos[key])
                st = (r1, x1, y1, l1)
                if st in seen:
                    if st in nxt:
                        nxt[st] |= m1
                    continue
                seen[st] = d + 1
                nxt[st] = m1
        layer = nxt
        d += 1
    return locks, d


def reach(h, hf, board_u8, sid, rot, x, y, l):
    """steps int32 [S], first uint8 [S], valid bool [S], Y int32 [S] and the
    number of layers the search needed, of one env."""
    board = board_u8.astype(bool)
    W = board.shape[0]
    per = W + 6
    valid, Y = landings(board, sid)
    locks, layers = search(h, hf, board_u8, sid, rot, x, y, l)
    steps, first = np.zeros(4 * per, np.int32), np.full(4 * per, 2, np.uint8)
    for s in np.flatnonzero(valid):
        hit = locks.get((s // per, s % per - 3, int(Y[s])))
        if hit:
            steps[s] = hit[0]
            first[s] = (hit[1] & -hit[1]).bit_length() - 1  # the lowest-numbered first action
    return steps, first, valid, Y, layers


def reach_env(h, hf, ob, i):
    e = ob.envs[i]
    return reach(h, hf, ob.board(i), e.shape_id, e.rot, e.ax, e.ay, e.lock)


def greedy_lands(h, hf, rot, x, y, l, W, slot, Y):
    """st_placement_actions's rule (rotate_left, then move, then hard drop)
    played out on the oracle from (rot, x, y, l): does the piece lock at the
    slot's landing?  h, hf: helpers(), loaded with the env's board and piece."""
    trot, tx = slot // (W + 6), slot % (W + 6) - 3
    for _ in range(400):
        a = 4 if rot != trot else (1 if x < tx else (0 if x > tx else 2))
        where = hf.step(rot, x, y, 0, a)[:3]
        rot, x, y, l, locked, _ = h.step(rot, x, y, l, a)
        if locked:
            return where == (trot, tx, int(Y))
    raise AssertionError("the greedy rule never locked")


# ------------------------------------------------------------------ crafted states (6x9)
CW, CH = 6, 9
T_, J_, L_, Z_, S_, I_, O_ = range(7)


def _board(cells=()):
    b = np.zeros((CW, CH), np.uint8)
    for x, y in cells:
        b[x, y] = 1
    return b


def _sl(rot, x):
    return rot * (CW + 6) + x + 3


# name, config, board, piece id, rot, x, y, lock counter, and -- for the first three -- the answer
# worked out by hand: {slot: (steps, first)} of every reachable slot.
#
# open_O: the O piece at the spawn of an empty board, lock_delay 0.  Nothing is in the way and the
# floor is 8 rows off, so a slot costs its rotations (rot 1: one rotate_left, rot 3: one rotate_right,
# rot 2: two of either), its |x - 3| moves and the hard drop that locks; any order of them is a
# shortest way, so `first` is the lowest action among them.  rot 0 / 1 span columns x - 1 .. x
# (x in 1..5), rot 2 / 3 columns x .. x + 1 (x in 0..4).
OPEN_O = {}
for _x in range(1, 6):
    OPEN_O[_sl(0, _x)] = (abs(_x - 3) + 1, 0 if _x < 3 else 1 if _x > 3 else 2)
    OPEN_O[_sl(1, _x)] = (abs(_x - 3) + 2, 0 if _x < 3 else 1 if _x > 3 else 4)
for _x in range(0, 5):
    OPEN_O[_sl(2, _x)] = (abs(_x - 3) + 3, 0 if _x < 3 else 1 if _x > 3 else 4)
    OPEN_O[_sl(3, _x)] = (abs(_x - 3) + 2, 0 if _x < 3 else 1 if _x > 3 else 5)
# resting_O_last: the O piece on the floor of an empty board at (3, 8), lock counter 3 of lock_delay
# 3: whatever the action, the piece is grounded after it and the counter wraps, so it locks in one
# step -- where it is (hard drop is the lowest action that leaves it there; rotate_left is refused:
# rot 1 reaches row 9), one column left or right, or in rot 3 (rows 7..8, columns 3..4).
RESTING_O_LAST = {_sl(0, 3): (1, 2), _sl(0, 2): (1, 0), _sl(0, 4): (1, 1), _sl(3, 3): (1, 5)}
# under_overhang: column 0 holds one block at row 4; the vertical I rests on the floor in column 1,
# lock_delay 0, so every action locks it in one step.  left tucks it under the block at (0, 8): no
# slot's landing (slot (0, 0) lands on the block at row 3 and cannot be reached from below), not
# reported.  right: (2, 8); staying: (1, 8); rotate_right: flat in columns 1..4 of row 8;
# rotate_left would span columns -2..1 and is refused.
UNDER_OVERHANG = {_sl(0, 1): (1, 2), _sl(0, 2): (1, 1), _sl(3, 1): (1, 5)}

LOCK3 = dict(P.C4, lock_delay=3, step_reset=True)
HAND = [
    ("open_O", {}, _board(), O_, 0, 3, 0, 0, OPEN_O),
    ("resting_O_last", LOCK3, _board(), O_, 0, 3, 8, 3, RESTING_O_LAST),
    ("under_overhang", {}, _board([(0, 4)]), I_, 0, 1, 8, 0, UNDER_OVERHANG),
]
_STACK = _board([(3, y) for y in range(CH)] + [(2, y) for y in range(4, CH)])
CRAFTED = HAND + [
    ("resting_O_fresh", LOCK3, _board(), O_, 0, 3, 8, 0, None),           # l = 0 under step_reset
    ("resting_O_last_lock2", dict(lock_delay=2), _board(), O_, 0, 3, 8, 2, None),
    ("spawn_in_stack", {}, _STACK, T_, 0, 3, 0, 0, None),                 # the start collides
    ("spawn_in_stack_lock3", LOCK3, _STACK, L_, 0, 3, 0, 1, None),
    ("overhang_from_above", {}, _board([(0, 4)]), I_, 0, 3, 0, 0, None),  # the tuck is no slot
    ("overhang_from_above_lock3", LOCK3, _board([(0, 4), (5, 3)]), J_, 0, 3, 0, 0, None),
    ("id7", {}, _board([(1, 8), (4, 7)]), 7, 0, 3, 0, 0, None),           # read as id 6
] + [("I_rot%d_x%d" % (r, x), cfg, _board([(2, 8)]), I_, r, x, 3, 0, None)
     for r in range(4) for x in (0, CW - 1) for cfg in ({}, LOCK3)]


def crafted_answer(case):
    """steps, first, valid, Y of a crafted state, from the oracle search."""
    name, cfg, board, sid, rot, x, y, l, _ = case
    def make():
        h, hf = helpers(dict(width=CW, height=CH, **cfg))
        return reach(h, hf, board, min(sid, 6), rot, x, y, l)[:4]
    return cached_ref(("reach_crafted", name, tuple(sorted(cfg.items()))), make)


def aged_oracle(board, config):
    """The sample: N envs, env e aged H + 2 * H * e // N + e % 3 steps of the
    splitmix64 action stream, reset on death."""
    kw = case_kw(board, config)
    H = kw["height"]
    ob = O.OracleBatch(N, case_seeds(board, config), **kw)
    ob.reset()
    ages = [H + 2 * H * e // N + e % 3 for e in range(N)]
    acts = O.splitmix64_actions(ASEED, 0, max(ages), N)
    for e in range(N):
        for t in range(ages[e]):
            if ob.step_one(e, int(acts[t, e]))[2]:
                ob.reset(e)
    return ob


def sample(board, config):
    """The aged oracle (`ob`, never stepped again: copy its state, do not move
    it) with steps / first / valid / Y [N, S], the start's lock counter and
    the layers each env's search needed."""
    def make():
        kw = case_kw(board, config)
        ob = aged_oracle(board, config)
        h, hf = helpers(kw)
        rows = [reach_env(h, hf, ob, e) for e in range(N)]
        out = {k: np.stack([r[j] for r in rows]) for j, k in enumerate(("steps", "first", "valid", "Y"))}
        out["layers"] = np.array([r[4] for r in rows])
        out["lock"] = ob.field("lock").copy()
        out["ob"] = ob
        return out
    return cached_ref(("reach_sample", board, config), make)
