"""The placement step in the oracle's terms, shared by test_gpu_placements.py
and test_cpu_placements.py.  A plain module imported by name, like harness.py
and replay.py; it runs no engine code and needs no GPU.

A placement step of env i on slot s (simpletetris.h, "Placement step") is, on
an OracleBatch: if the slot is valid, set_state(shape_id, rot, ax = x, ay = 0,
lock = max(lock_delay, 0)); then step_one(i, 2).  Validity is a few-line
restatement of is_occupied (tetris_env.py:29-36) on the oracle's board.
"""
import numpy as np

from harness import C4, cached_ref, pack_cols
from oracle import oracle as O

NF = 11
VALID, Y, LINES, HOLES, HEIGHT, ROWS, ABOVE, DEAD, REWARD, AGG, BUMP = range(NF)
GREEDY = np.zeros(NF, np.float32)
GREEDY[[LINES, HOLES, HEIGHT, ABOVE]] = 80, -12, -3, -2000
AGG_UP = np.zeros(NF, np.float32)
AGG_UP[AGG] = 1.0  # rewards height: its games end
THREE_ROWS = np.stack([GREEDY, np.zeros(NF, np.float32), AGG_UP])


def occupied(cells, x0, y0, board):
    """is_occupied (tetris_env.py:29-36) on a bool board [W, H]."""
    W, H = board.shape
    for i, j in cells:
        x, y = x0 + i, y0 + j
        if y < 0:
            continue
        if x < 0 or x >= W or y >= H or board[x, y]:
            return True
    return False


def decode(W, slot):
    """(rot, x) of a slot in [0, S), None outside."""
    per = W + 6
    if not 0 <= slot < 4 * per:
        return None
    return slot // per, slot % per - 3


def slot_valid(ob, i, slot):
    """The header's validity rule for env i of an OracleBatch."""
    rx = decode(ob.cfg.width, int(slot))
    if rx is None:
        return False
    cells = O.rotate_cells(O.BASE_SHAPES[ob.envs[i].shape_id], rx[0])
    return not occupied(cells, rx[1], 0, ob.board(i).astype(bool))


def commit(ob, i, slot):
    """The commit alone on the oracle; returns whether the slot was valid."""
    if not slot_valid(ob, i, slot):
        return False
    rot, x = decode(ob.cfg.width, int(slot))
    ob.set_state(i, shape_id=ob.envs[i].shape_id, rot=rot, ax=x, ay=0, lock=max(ob.cfg.lock_delay, 0))
    return True


def ref_place_step(ob, i, slot, autoreset):
    """One placement step of env i -> (packed obs [W] u32, reward, done,
    placed); under 'same_step' a death resets the env behind the step."""
    placed = commit(ob, i, slot)
    obs, rew, done, _ = ob.step_one(i, 2)
    if done and autoreset == "same_step":
        ob.reset(i)
    return pack_cols(obs), rew, done, placed


def place_steps(ob, slots, autoreset):
    """ref_place_step over slots [T, n]: rows as harness.check_step reads them,
    `placed` u8 [T, n], `lines` (the largest lines counter seen) and, of the
    end, packed_state() as `final` and the oracle itself as `ob`."""
    T, n = slots.shape
    out = dict(slots=slots, obs=np.empty((T, n, ob.cfg.width), np.uint32), reward=np.empty((T, n), np.int32),
               done=np.empty((T, n), np.uint8), placed=np.empty((T, n), np.uint8), lines=0)
    for t in range(T):
        for i in range(n):
            out["obs"][t, i], out["reward"][t, i], out["done"][t, i], out["placed"][t, i] = \
                ref_place_step(ob, i, slots[t, i], autoreset)
            out["lines"] = max(out["lines"], int(ob.envs[i].lines_cleared))
    out["final"] = ob.packed_state()
    out["ob"] = ob
    return out


# ------------------------------------------------------------------ test 1's sample: random slots
N, T_RANDOM = 70, 40  # one full 64-env step workgroup and a partial one; 17.5 policy workgroups of 4 waves
BOARDS = {"10x20": (10, 20),   # the specialised kernels
          "6x9": (6, 9),       # the generic path
          "11x12": (11, 12)}   # S = 68 > 64: the second slot pass
CONFIGS = {"default": dict(), "c4_lock3": dict(C4, lock_delay=3, step_reset=True)}
AUTORESETS = ("none", "same_step")
RANDOM_SEED = 4100


def case_kw(board, config):
    W, H = BOARDS[board]
    return dict(width=W, height=H, **CONFIGS[config])


def case_seeds(board, config):
    base = 5000 + 100 * sorted(BOARDS).index(board) + 1000 * sorted(CONFIGS).index(config)
    return [base + e for e in range(N)]


def random_slots(board):
    """Env e at step t takes rng.integers(-2, S + 2): valid, invalid and
    out-of-range slots mixed, the same stream for every config."""
    S = 4 * (BOARDS[board][0] + 6)
    rng = np.random.default_rng(RANDOM_SEED + sorted(BOARDS).index(board))
    return rng.integers(-2, S + 2, (T_RANDOM, N))


def random_run(board, config, autoreset):
    def make():
        ob = O.OracleBatch(N, case_seeds(board, config), **case_kw(board, config))
        ob.reset()
        return place_steps(ob, random_slots(board), autoreset)
    return cached_ref(("placements_random", board, config, autoreset), make)


# ------------------------------------------------------------------ test 5's sample: the CPU player
def scores_f32(w, feat):
    """The header's chain on rows feat [NF, S] with weights w [NF]:
    np.float32 multiply, then np.float32 add, row by row."""
    w = np.asarray(w, np.float32)
    acc = np.zeros(feat.shape[1:], np.float32)
    for r in range(NF):
        acc = acc + w[r] * feat[r].astype(np.float32)
    assert acc.dtype == np.float32
    return acc


def choose(w, feat):
    """st_policy_linear's slot of one env: feat int [NF, S], w [NF]; the
    first maximum over the valid slots, -1 without one."""
    sc = scores_f32(w, feat)
    idx = np.flatnonzero(feat[VALID] != 0)
    return int(idx[np.argmax(sc[idx])]) if len(idx) else -1


def helper_oracle(kw):
    kw = dict(kw, lock_delay=0)
    kw.pop("step_reset", None)
    ob = O.OracleBatch(1, [1], **kw)
    ob.reset()
    return ob


def slot_features(h, board, sid, holes, piece_height):
    """feat int32 [NF, S] of one env from the one-env oracle h (set_state +
    the hard drop that locks the piece in the slot): bool board [W, H], piece
    id and the env's holes / piece_height counters."""
    W, H = board.shape
    per, S = W + 6, 4 * (W + 6)
    board_u8 = board.astype(np.uint8)
    feat = np.zeros((NF, S), np.int32)
    for rot in range(4):
        cells = O.rotate_cells(O.BASE_SHAPES[sid], rot)
        for x in range(-3, W + 3):
            if occupied(cells, x, 0, board):
                continue
            y = 0
            while not occupied(cells, x, y + 1, board):
                y += 1
            h.set_state(0, board=board_u8, shape_id=sid, rot=rot, ax=x, ay=0, lock=0, holes=holes,
                        piece_height=piece_height)
            lines0 = h.envs[0].lines_cleared
            _, rew, done, _ = h.step_one(0, 2)
            b = board.copy()  # _set_piece's clipping (:323-327), then _clear_lines (:205-216)
            for i, j in cells:
                if 0 <= x + i < W and 0 <= y + j < H:
                    b[x + i, y + j] = True
            keep = b[:, ~b.all(axis=0)]
            nb = np.zeros_like(b)
            nb[:, H - keep.shape[1]:] = keep
            hcol = np.where(nb.any(axis=1), H - nb.argmax(axis=1), 0)
            row_any = nb.any(axis=0)
            feat[:, rot * per + x + 3] = (
                1, y, h.envs[0].lines_cleared - lines0, h.envs[0].holes,
                H - int(row_any.argmax()) if row_any.any() else 0, int(row_any.sum()),
                int(any(y + j < 0 for _, j in cells)), int(done), rew, int(hcol.sum()), int(np.abs(np.diff(hcol)).sum()))
    return feat


TINY = dict(n=8, kw=dict(width=6, height=8, **C4), seed0=3100, T=60)


TINY_AY = 4


def tiny_blocked_board():
    """Env 0's first state: row 0 full and the live piece at anchor row
    TINY_AY below it (a legal position: its cells lie in rows 1..4), so that no
    slot is valid, the player's slot is -1 and the step falls back to the
    hard drop of the live piece from where it is."""
    b = np.zeros((TINY["kw"]["width"], TINY["kw"]["height"]), np.uint8)
    b[:, 0] = 1
    return b


def cpu_player():
    """The numpy / oracle placement player on the tiny shape under
    'same_step': per env and step the oracle's slot features, the float32
    score, the first maximum, then ref_place_step.  Env e plays weight row
    e % 3; env 0 starts on tiny_blocked_board().  No engine call."""
    n, kw, T = TINY["n"], TINY["kw"], TINY["T"]
    ob = O.OracleBatch(n, [TINY["seed0"] + e for e in range(n)], **kw)
    ob.reset()
    ob.set_state(0, board=tiny_blocked_board(), ay=TINY_AY)
    h = helper_oracle(kw)
    slots = np.empty((T, n), np.int32)
    out = dict(slots=slots, obs=np.empty((T, n, kw["width"]), np.uint32), reward=np.empty((T, n), np.int32),
               done=np.empty((T, n), np.uint8), placed=np.empty((T, n), np.uint8), lines=0)
    for t in range(T):
        for e in range(n):
            env = ob.envs[e]
            feat = slot_features(h, ob.board(e).astype(bool), env.shape_id, env.holes, env.piece_height)
            slots[t, e] = choose(THREE_ROWS[e % 3], feat)
            out["obs"][t, e], out["reward"][t, e], out["done"][t, e], out["placed"][t, e] = \
                ref_place_step(ob, e, slots[t, e], "same_step")
            out["lines"] = max(out["lines"], int(ob.envs[e].lines_cleared))
    out["returns"] = out["reward"].astype(np.int64).sum(axis=0)
    out["episodes"] = out["done"].astype(np.int32).sum(axis=0)
    out["final"] = ob.packed_state()
    out["ob"] = ob
    return out


def tiny_ref():
    return cached_ref("placements_tiny_player", cpu_player)
