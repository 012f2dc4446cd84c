"""st_next_piece and the two-ply player (simpletetris.h, "Next piece",
"Two-ply player") in the oracle's terms, shared by test_cpu_lookahead.py,
test_gpu_next_piece.py and test_gpu_lookahead.py.  A plain module imported by
name, like feature_ref.py and placement_ref.py; it runs no engine code and
needs no GPU.

The next piece is what the oracle's own clear() spawns on a byte copy of the
env.  The two-ply score composes the one-ply references: the first ply's rows
by placement_ref.slot_features / feature_ref.slot_features_bcts, then, for
every live candidate, the same function on the board and with the counters the
one-env oracle holds after it has locked the piece there.
"""
import ctypes

import numpy as np

import feature_ref as FR
import placement_ref as PR
from oracle import oracle as O


def next_piece(ob, i):
    """The shape id env i's next _new_piece takes: clear() (tetris_env.py:306-315)
    on a byte copy of the oracle's env, which draws with the env's counts and
    MT19937 state of the moment; the env itself is not touched."""
    e = O.Env.from_buffer_copy(ob.envs[i])
    O.lib().or_env_clear(ctypes.byref(e))
    return int(e.shape_id)


def next_pieces(ob):
    return np.array([next_piece(ob, i) for i in range(ob.n)], np.uint8)


def rows_of(features):
    return {"base": PR.slot_features, "bcts": FR.slot_features_bcts}[features]


def state_after(h, board, sid, s1, holes, piece_height):
    """X(s1) without its piece: the one-env oracle h locks piece sid in slot s1
    (valid) of bool board [W, H] with the env's counters and is read back --
    (bool board, holes, piece_height, died).  The board of a death is the
    reference's cleared one and is not used."""
    W = board.shape[0]
    rot, x = PR.decode(W, int(s1))
    h.set_state(0, board=board.astype(np.uint8), shape_id=int(sid), rot=rot, ax=x, ay=0, lock=0, holes=int(holes),
                piece_height=int(piece_height))
    _, _, done, _ = h.step_one(0, 2)
    return h.board(0).astype(bool), int(h.envs[0].holes), int(h.envs[0].piece_height), bool(done)


def plies(h, board, sid, next_sid, holes, piece_height, features="base"):
    """The rows both plies score, weights and mask apart: f1 int32 [R, S] of the
    live piece and {s1: f2 int32 [R, S]} of the next piece in X(s1), for every
    valid s1 that does not end the game."""
    rows = rows_of(features)
    f1 = rows(h, board, int(sid), int(holes), int(piece_height))
    f2 = {}
    for s1 in np.flatnonzero((f1[PR.VALID] != 0) & (f1[PR.DEAD] == 0)):
        b1, holes1, height1, died = state_after(h, board, sid, s1, holes, piece_height)
        assert not died
        f2[int(s1)] = rows(h, b1, int(next_sid), holes1, height1)
    return dict(f1=f1, f2=f2)


def score(pl, w1, w2, dead_value, allowed=None):
    """st_policy_lookahead's scores and choice on the rows of plies():
    dict(scores_all f32 [S], slots2_all i32 [S], slot, slot2, score, dead bool
    [S], cand bool [S])."""
    f1 = pl["f1"]
    S = f1.shape[1]
    cand = f1[PR.VALID] != 0
    if allowed is not None:
        cand = cand & (np.asarray(allowed) != 0)
    s1_scores = FR.scores_f32(w1, f1) if w1 is not None else np.zeros(S, np.float32)
    scores_all = np.zeros(S, np.float32)
    slots2_all = np.full(S, -1, np.int32)
    dead = cand & (f1[PR.DEAD] != 0)
    dv = np.float32(dead_value)
    for s1 in np.flatnonzero(cand):
        tail, s2 = dv, -1
        if not dead[s1]:
            f2 = pl["f2"][int(s1)]
            idx = np.flatnonzero(f2[PR.VALID] != 0)
            if len(idx):
                sc2 = FR.scores_f32(w2, f2)
                s2 = int(idx[np.argmax(sc2[idx])])  # the first maximum
                tail = sc2[s2]
        total = np.float32(s1_scores[s1]) + np.float32(tail)  # one float32 add
        assert total.dtype == np.float32
        scores_all[s1], slots2_all[s1] = total, s2
    idx = np.flatnonzero(cand)
    if len(idx):
        slot = int(idx[np.argmax(scores_all[idx])])  # the first maximum
        slot2, best = int(slots2_all[slot]), scores_all[slot]
    else:
        slot, slot2, best = -1, -1, np.float32(0.0)
    return dict(scores_all=scores_all, slots2_all=slots2_all, slot=slot, slot2=slot2, score=np.float32(best),
                dead=dead, cand=cand)


def lookahead(h, board, sid, next_sid, holes, piece_height, w1, w2, dead_value, allowed=None, features="base"):
    """st_policy_lookahead for one env: bool board [W, H], the live piece sid,
    the next piece next_sid, the env's holes / piece_height counters, weight
    rows w1 (or None) and w2 over the rows of `features`, allowed [S] or None:
    score() on plies()."""
    return score(plies(h, board, sid, next_sid, holes, piece_height, features), w1, w2, dead_value, allowed)


def helper_for(ob):
    return PR.helper_oracle({k: getattr(ob.cfg, k) for k in ("width", "height") + O.SCORING_KEYS})


def lookahead_env(h, ob, i, w1, w2, dead_value, allowed=None, features="base"):
    """lookahead() for env i of an OracleBatch in its present state."""
    env = ob.envs[i]
    return lookahead(h, ob.board(i).astype(bool), env.shape_id, next_piece(ob, i), env.holes, env.piece_height, w1, w2,
                     dead_value, allowed, features)


def plies_batch(ob, features="base"):
    """plies() of every env of an OracleBatch in its present state, and what
    the stacked result needs beside them."""
    h = helper_for(ob)
    out = []
    for i in range(ob.n):
        env = ob.envs[i]
        out.append(plies(h, ob.board(i).astype(bool), env.shape_id, next_piece(ob, i), env.holes, env.piece_height,
                         features))
    return dict(plies=out, piece=ob.packed_state()["piece"], width=ob.cfg.width)


def score_batch(pb, w1, w2, dead_value, allowed=None):
    """score() over plies_batch()'s envs (env e plays weight row e % n_w),
    stacked: scores_all [n, S], slots2_all [n, S], slots / slots2 [n], scores
    [n], dead / cand [n, S] and actions [n] (st_placement_actions's rule)."""
    w2 = np.asarray(w2, np.float32)
    w2 = w2.reshape(-1, w2.shape[-1])
    w1 = None if w1 is None else np.asarray(w1, np.float32).reshape(w2.shape)
    n = len(pb["plies"])
    rs = [score(pb["plies"][e], None if w1 is None else w1[e % len(w2)], w2[e % len(w2)], dead_value,
                None if allowed is None else allowed[e]) for e in range(n)]
    return dict(scores_all=np.stack([r["scores_all"] for r in rs]), slots2_all=np.stack([r["slots2_all"] for r in rs]),
                slots=np.array([r["slot"] for r in rs], np.int32), slots2=np.array([r["slot2"] for r in rs], np.int32),
                scores=np.array([r["score"] for r in rs], np.float32), dead=np.stack([r["dead"] for r in rs]),
                cand=np.stack([r["cand"] for r in rs]),
                actions=np.array([FR.action_for(pb["width"], pb["piece"][e], rs[e]["slot"]) for e in range(n)],
                                 np.uint8))
