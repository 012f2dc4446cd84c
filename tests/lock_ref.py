"""Lock positions in the oracle's terms (simpletetris.h, "Lock positions"),
shared by test_cpu_locks.py and test_gpu_locks.py.  A plain module imported by
name, like reach_ref.py; it runs no engine code and needs no GPU.

The lock set is reach_ref.search's `locks` -- every (rot, x, y) an oracle step
locked the piece at -- without the positions the piece collides in
(placement_ref.occupied: a start that locks where it stands).  The rows of a
position come from a one-env oracle of the case's config: the piece is set at
(rot, x, y) with the lock counter at L and one idle step is taken; the piece is
grounded, so the counter wraps and it locks where it is.  Routes are
route_ref's, whose graph serves any target.
"""
import numpy as np

import feature_ref as FR
import placement_ref as P
import reach_ref as R
import route_ref as RT
from harness import cached_ref
from oracle import oracle as O

IDLE = 6


def lock_pos(W, rot, x, y):
    return (rot * (W + 6) + x + 3) * 32 + y


def lock_rot_x_y(W, pos):
    s, per = pos >> 5, W + 6
    return s // per, s % per - 3, pos & 31


def lock_set(h, hf, board_u8, sid, rot, x, y, l):
    """{(rot, x, y): steps} of every lock position of one env."""
    board = board_u8.astype(bool)
    locks, _ = R.search(h, hf, board_u8, sid, rot, x, y, l)
    return {k: v[0] for k, v in locks.items()
            if not P.occupied(O.rotate_cells(O.BASE_SHAPES[sid], k[0]), k[1], k[2], board)}


def rows_of(W, S, positions):
    """uint32 [S]: bit y of word s for every position (rot, x, y)."""
    rows = np.zeros(S, np.uint32)
    for r, x, y in positions:
        rows[r * (W + 6) + x + 3] |= np.uint32(1 << y)
    return rows


def pos_list(W, positions):
    return sorted(lock_pos(W, *p) for p in positions)


def is_landing(valid, Y, W, p):
    s = p[0] * (W + 6) + p[1] + 3
    return bool(valid[s]) and int(Y[s]) == p[2]


def evaluable(board, sid, W, pos):
    """The header's rule for a position word on bool board [W, H]."""
    H = board.shape[1]
    if pos < 0 or (pos >> 5) >= 4 * (W + 6) or (pos & 31) >= H:
        return False
    rot, x, y = lock_rot_x_y(W, pos)
    cells = O.rotate_cells(O.BASE_SHAPES[sid], rot)
    return not P.occupied(cells, x, y, board) and P.occupied(cells, x, y + 1, board)


def rows_oracle(kw):
    ob = O.OracleBatch(1, [1], **kw)
    ob.reset()
    return ob


def rows_at(hk, kw, board, sid, holes, piece_height, rot, x, y, features="base"):
    """(feat int32 [rows], board after the clear bool [W, H]) of the piece
    locked at (rot, x, y): hk is rows_oracle(kw)."""
    W, H = board.shape
    cells = O.rotate_cells(O.BASE_SHAPES[sid], rot)
    assert not P.occupied(cells, x, y, board) and P.occupied(cells, x, y + 1, board)
    hk.set_state(0, board=board.astype(np.uint8), shape_id=sid, rot=rot, ax=x, ay=y,
                 lock=max(kw.get("lock_delay", 0), 0), holes=holes, piece_height=piece_height)
    e = hk.envs[0]
    lines0, spawned = e.lines_cleared, sum(e.counts)
    _, rew, done, _ = hk.step_one(0, IDLE)
    assert sum(e.counts) != spawned or done, "the idle step did not lock the piece"
    ext, nb = FR.ext_features(board, cells, x, y)
    hcol = np.where(nb.any(axis=1), H - nb.argmax(axis=1), 0)
    row_any = nb.any(axis=0)
    base = (1, y, e.lines_cleared - lines0, e.holes, H - int(row_any.argmax()) if row_any.any() else 0,
            int(row_any.sum()), int(any(y + j < 0 for _, j in cells)), int(done), rew, int(hcol.sum()),
            int(np.abs(np.diff(hcol)).sum()))
    return np.array(base + (tuple(ext) if features == "bcts" else ()), np.int32), nb


def sample(board, config):
    """reach_ref.sample's aged oracle with, per env, `locks` {(rot, x, y):
    steps}; `rows` uint32 [N, S]; `count` [N]."""
    def make():
        kw = R.case_kw(board, config)
        smp = R.sample(board, config)
        ob = smp["ob"]
        W = kw["width"]
        h, hf = R.helpers(kw)
        locks = []
        for i in range(R.N):
            e = ob.envs[i]
            locks.append(lock_set(h, hf, ob.board(i), e.shape_id, e.rot, e.ax, e.ay, e.lock))
        rows = np.stack([rows_of(W, 4 * (W + 6), lk) for lk in locks])
        return dict(locks=locks, rows=rows, count=np.array([len(lk) for lk in locks], np.int32))
    return cached_ref(("lock_sample", board, config), make)


def sample_feat(board, config, features):
    """Per env {(rot, x, y): (feat [rows], board words uint32 [W])} of every
    lock position of the sample."""
    def make():
        kw = R.case_kw(board, config)
        ob = R.sample(board, config)["ob"]
        hk = rows_oracle(kw)
        out = []
        for i, lk in enumerate(sample(board, config)["locks"]):
            e = ob.envs[i]
            b = ob.board(i).astype(bool)
            d = {}
            for p in lk:
                f, nb = rows_at(hk, kw, b, e.shape_id, e.holes, e.piece_height, *p, features=features)
                d[p] = (f, O.pack_cols(nb))
            out.append(d)
        return out
    return cached_ref(("lock_feat", board, config, features), make)


def crafted_locks(case):
    """{(rot, x, y): steps} of a reach_ref.CRAFTED state."""
    name, cfg, board, sid, rot, x, y, l, _ = case
    def make():
        h, hf = R.helpers(dict(width=R.CW, height=R.CH, **cfg))
        return lock_set(h, hf, board, min(sid, 6), rot, x, y, l)
    return cached_ref(("lock_crafted", name, tuple(sorted(cfg.items()))), make)


def choose(w, feats):
    """(pos index, score) over feats [rows, K] in ascending pos order: the
    first maximum of the header's float32 chain; (-1, 0.0) for K = 0."""
    if feats.shape[1] == 0:
        return -1, np.float32(0.0)
    sc = FR.scores_f32(w, feats)
    i = int(np.argmax(sc))
    return i, sc[i]


def deep_row(rows):
    w = np.zeros(rows, np.float32)
    w[P.Y] = 1.0
    return w


def route_to(er, target):
    """The route of a route_ref.EnvRoutes to a lock position (rot, x, y)."""
    D = RT.distances(er.preds, er.lockers, target)
    return RT.walk(er.trans, D, er.start, target) if er.start in D else []
