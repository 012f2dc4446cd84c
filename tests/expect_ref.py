"""st_next_weights and the expectimax player (simpletetris.h, "Next-piece
odds", "Expectimax player") in the oracle's terms, shared by
test_cpu_expect.py and test_gpu_expect.py.  A plain module imported by name,
like lookahead_ref.py; it runs no engine code and needs no GPU.

The odds are tetris_env.py:186 on the oracle env's counts.  The score composes
lookahead_ref's pieces: the first ply's rows and the state behind every live
slot once (rows_of, state_after), then the one-ply rows of each of the seven
pieces in that state -- what lookahead_ref.plies computes for one known next
piece, with the first ply shared.  The chain is numpy float32 scalars, each
operation on its own.
"""
import numpy as np

import feature_ref as FR
import lookahead_ref as LR
import placement_ref as PR

NQ = 7


def weights_of(counts):
    """m of _choose_shape (tetris_env.py:184-186) for shape counts."""
    values = [int(c) for c in counts]
    maxm = max(values)
    return [5 + maxm - x for x in values]


def next_weights(ob, i):
    """The odds of the piece env i's next _new_piece takes, from the oracle
    env's counts."""
    return np.array(weights_of(ob.envs[i].counts), np.int64)


def plies(h, board, sid, holes, piece_height, features="base"):
    """The rows both plies score: f1 int32 [R, S] of the live piece and
    f2[q] = {s1: int32 [R, S]} of piece q in X(s1), for every valid s1 that
    does not end the game (lookahead_ref.plies's f2 for next_sid = q; the first
    ply and X(s1) are computed once)."""
    rows = LR.rows_of(features)
    f1 = rows(h, board, int(sid), int(holes), int(piece_height))
    f2 = [dict() for _ in range(NQ)]
    for s1 in np.flatnonzero((f1[PR.VALID] != 0) & (f1[PR.DEAD] == 0)):
        b1, holes1, height1, died = LR.state_after(h, board, sid, s1, holes, piece_height)
        assert not died
        for q in range(NQ):
            f2[q][int(s1)] = rows(h, b1, q, holes1, height1)
    return dict(f1=f1, f2=f2)


def as_lookahead(pl, q):
    """plies() as lookahead_ref.plies(.., next_sid=q) returns it."""
    return dict(f1=pl["f1"], f2=pl["f2"][q])


def chain(m, tails):
    """E of the header: acc = acc + float32(m[q]) * T[q] from 0.0f over q in
    order, then one float32 division by float32(sum(m)); every operation a
    numpy float32 scalar operation."""
    acc = np.float32(0.0)
    for q in range(NQ):
        prod = np.float32(int(m[q])) * np.float32(tails[q])
        assert prod.dtype == np.float32
        acc = acc + prod
        assert acc.dtype == np.float32
    M = sum(int(x) for x in m)  # an exact integer sum
    e = acc / np.float32(M)
    assert e.dtype == np.float32
    return e


def score(pl, m, w1, w2, dead_value, allowed=None):
    """st_policy_expect's tables and choice on the rows of plies() with odds m
    [7]: dict(scores_all f32 [S], tails f32 [7, S], slots2_all i32 [7, S],
    slot, score, dead bool [S], cand bool [S])."""
    f1 = pl["f1"]
    S = f1.shape[1]
    cand = f1[PR.VALID] != 0
    if allowed is not None:
        cand = cand & (np.asarray(allowed) != 0)
    s1_scores = FR.scores_f32(w1, f1) if w1 is not None else np.zeros(S, np.float32)
    scores_all = np.zeros(S, np.float32)
    tails = np.zeros((NQ, S), np.float32)
    slots2_all = np.full((NQ, S), -1, np.int32)
    dead = cand & (f1[PR.DEAD] != 0)
    dv = np.float32(dead_value)
    with np.errstate(over="ignore"):
        for s1 in np.flatnonzero(cand):
            for q in range(NQ):
                tail, s2 = dv, -1
                if not dead[s1]:
                    f2 = pl["f2"][q][int(s1)]
                    idx = np.flatnonzero(f2[PR.VALID] != 0)
                    if len(idx):
                        sc2 = FR.scores_f32(w2, f2)
                        s2 = int(idx[np.argmax(sc2[idx])])  # the first maximum
                        tail = sc2[s2]
                tails[q, s1], slots2_all[q, s1] = tail, s2
            total = np.float32(s1_scores[s1]) + chain(m, tails[:, s1])  # one float32 add
            assert total.dtype == np.float32
            scores_all[s1] = total
    idx = np.flatnonzero(cand)
    if len(idx):
        slot = int(idx[np.argmax(scores_all[idx])])  # the first maximum
        best = scores_all[slot]
    else:
        slot, best = -1, np.float32(0.0)
    return dict(scores_all=scores_all, tails=tails, slots2_all=slots2_all, slot=slot, score=np.float32(best),
                dead=dead, cand=cand)


def expect(h, board, sid, counts, holes, piece_height, w1, w2, dead_value, allowed=None, features="base"):
    """st_policy_expect for one env: bool board [W, H], the live piece sid, the
    seven shape counts, the env's holes / piece_height counters, weight rows w1
    (or None) and w2 over the rows of `features`, allowed [S] or None."""
    return score(plies(h, board, sid, holes, piece_height, features), weights_of(counts), w1, w2, dead_value, allowed)


def plies_batch(ob, features="base"):
    """plies() and next_weights() of every env of an OracleBatch in its present
    state, and what the stacked result needs beside them."""
    h = LR.helper_for(ob)
    out = []
    for i in range(ob.n):
        env = ob.envs[i]
        out.append(plies(h, ob.board(i).astype(bool), env.shape_id, env.holes, env.piece_height, features))
    return dict(plies=out, m=np.stack([next_weights(ob, i) for i in range(ob.n)]), piece=ob.packed_state()["piece"],
                width=ob.cfg.width)


def score_batch(pb, w1, w2, dead_value, allowed=None, m=None):
    """score() over plies_batch()'s envs (env e plays weight row e % n_w; m
    [n, 7] replaces the oracle's own odds), stacked: scores_all [n, S], tails /
    slots2_all [n, 7, S], slots / scores [n], dead / cand [n, S] and actions
    [n] (st_placement_actions's rule)."""
    w2 = np.asarray(w2, np.float32)
    w2 = w2.reshape(-1, w2.shape[-1])
    w1 = None if w1 is None else np.asarray(w1, np.float32).reshape(w2.shape)
    m = pb["m"] if m is None else np.asarray(m)
    n = len(pb["plies"])
    rs = [score(pb["plies"][e], m[e], None if w1 is None else w1[e % len(w2)], w2[e % len(w2)], dead_value,
                None if allowed is None else allowed[e]) for e in range(n)]
    out = {k: np.stack([r[k] for r in rs]) for k in ("scores_all", "tails", "slots2_all", "dead", "cand")}
    out["slots"] = np.array([r["slot"] for r in rs], np.int32)
    out["scores"] = np.array([r["score"] for r in rs], np.float32)
    out["actions"] = np.array([FR.action_for(pb["width"], pb["piece"][e], rs[e]["slot"]) for e in range(n)], np.uint8)
    return out
