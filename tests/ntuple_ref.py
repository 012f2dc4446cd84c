"""The n-tuple network and its player (simpletetris.h, "N-tuple network") in
numpy and the oracle's terms, shared by test_cpu_ntuple.py and
test_gpu_ntuple.py.  A plain module imported by name, like lookahead_ref.py; it
runs no engine code and needs no GPU.

The index and the chain are restated on bool boards [W, H].  The player's
reference composes the one-ply references: the rows of every slot by
placement_ref.slot_features / feature_ref.slot_features_bcts, the board of
every valid live slot by lookahead_ref.state_after (the one-env oracle locks
the piece there), V = dead_value for dead slots, and feature_ref.choose's rule
(the first maximum over the candidates) on S1 + V.
"""
import numpy as np

import feature_ref as FR
import lookahead_ref as LR
import placement_ref as PR

MAX_TUPLES, MAX_BITS = 4096, 16


# ------------------------------------------------------------------ networks, tables, weights
def systematic(W, H, w, h, share=False, mirror=False):
    """The double loop NTupleNet.systematic is held to: every position of a
    w x h window, x outermost, one table per position or one shared table; with
    mirror each tuple is followed by its mirror image on the same base."""
    rows, k = [], 0
    for x in range(W - w + 1):
        for y in range(H - h + 1):
            base = 0 if share else k << (w * h)
            rows.append((x, y, w, h, 0, base))
            if mirror:
                rows.append((W - x - w, y, w, h, 1, base))
            k += 1
    return np.array(rows, np.int32)


def hand_mix(W, H):
    """A hand-made mix: a 1x1 and a 16x1 tuple (4 <= W < 16: as wide as the
    board allows), a 1-wide column, flipped and unflipped 2x3 windows on
    overlapping bases, and a 4x4 window in the bottom-right corner."""
    wide = min(W, 16)
    return np.array([(0, H - 1, 1, 1, 0, 0),
                     (W - wide, H - 1, wide, 1, 0, 1),
                     (W - 1, 0, 1, min(H, 16), 0, 7),
                     (0, H - 3, 2, 3, 0, 40),
                     (W - 2, H - 3, 2, 3, 1, 40),
                     (1, H - 4, 2, 3, 1, 50),
                     (W - 4, H - 4, 4, 4, 0, 3),
                     (W - 4, H - 4, 4, 4, 1, 11)], np.int32)


def table_len(tuples):
    t = np.asarray(tuples, np.int64)
    return int((t[:, 5] + (1 << (t[:, 2] * t[:, 3]))).max())


def make_table(n, seed):
    """float32 [n]: uniform +-1 times 10^(-2..2), mixed per entry."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-2, 3, n)).astype(np.float32)


def mixed_weights(n_w, nf, seed=5):
    """n_w rows of mixed-sign float32 weights whose products do not fit a
    float32 exactly (test_gpu_features's rows, for either feature set)."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 3.0, (n_w, nf)).astype(np.float32)
    w[:, PR.REWARD] *= 0.01
    return w


# ------------------------------------------------------------------ index, chain
def index_cells(tuples, board):
    """base_t + idx_t of one bool board [W, H], cell by cell: int64 [T]."""
    out = np.empty(len(tuples), np.int64)
    for t, (x, y, w, h, flip, base) in enumerate(np.asarray(tuples).tolist()):
        idx = 0
        for i in range(w):
            c = x + (w - 1 - i if flip else i)
            for j in range(h):
                idx |= int(board[c, y + j]) << (i * h + j)
        out[t] = base + idx
    return out


def pack(boards):
    """bool [..., W, H] -> column words uint32 [..., W] (bit r = row r)."""
    b = np.asarray(boards, bool)
    return (b.astype(np.uint64) << np.arange(b.shape[-1], dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


def index_words(tuples, words):
    """base_t + idx_t of column words uint32 [M, W]: int64 [M, T], by the
    header's formula on the words."""
    words = np.asarray(words, np.uint32).astype(np.int64)
    out = np.empty((words.shape[0], len(tuples)), np.int64)
    for t, (x, y, w, h, flip, base) in enumerate(np.asarray(tuples).tolist()):
        idx = np.zeros(words.shape[0], np.int64)
        for i in range(w):
            c = x + (w - 1 - i if flip else i)
            idx |= ((words[:, c] >> y) & ((1 << h) - 1)) << (i * h)
        out[:, t] = base + idx
    return out


def chain(table, index, reverse=False):
    """N over index int64 [M, T]: float32 acc = acc + table[index[:, t]] for
    t in order (reverse: from the last tuple down) from 0.0f."""
    table = np.asarray(table, np.float32)
    acc = np.zeros(index.shape[0], np.float32)
    order = range(index.shape[1] - 1, -1, -1) if reverse else range(index.shape[1])
    for t in order:
        acc = acc + table[index[:, t]]
    assert acc.dtype == np.float32
    return acc


# ------------------------------------------------------------------ the player
def env_plies(h, board, sid, holes, piece_height):
    """What the player's reference needs of one env, network and weights
    apart: the rows of both feature sets, f int32 [R, S], and the packed
    afterstate board uint32 [W] of every valid slot that does not end the game
    (the one-env oracle h locks the piece there)."""
    fb = FR.slot_features_bcts(h, board, int(sid), int(holes), int(piece_height))
    f = {"base": fb[:PR.NF].copy(), "bcts": fb}
    words = {}
    for s in np.flatnonzero((fb[PR.VALID] != 0) & (fb[PR.DEAD] == 0)):
        b1, _, _, died = LR.state_after(h, board, sid, s, holes, piece_height)
        assert not died
        words[int(s)] = pack(b1)
    return dict(f=f, words=words)


def plies_of_state(kw, state):
    """env_plies of every env of an engine state (get_state's board uint32
    [W, n], piece uint32 [n], stats int32 [>= 5, n]) under the settings kw."""
    h = PR.helper_oracle(kw)
    W, H = kw["width"], kw["height"]
    n = state["piece"].shape[0]
    out = []
    for e in range(n):
        cols = state["board"][:, e].astype(np.uint32)
        board = ((cols[:, None] >> np.arange(H, dtype=np.uint32)) & 1).astype(bool)
        out.append(env_plies(h, board, int(state["piece"][e]) & 7, int(state["stats"][3, e]),
                             int(state["stats"][4, e])))
    return dict(plies=out, piece=state["piece"].copy(), width=W)


def index_batch(pb, tuples):
    """base_t + idx_t of every live slot's board of plies_of_state()'s envs:
    per env {slot: int64 [T]} (computed once per network, shared by the
    scorings)."""
    out = []
    for pl in pb["plies"]:
        slots = sorted(pl["words"])
        idx = index_words(tuples, np.stack([pl["words"][s] for s in slots])) if slots else []
        out.append({s: idx[k] for k, s in enumerate(slots)})
    return out


def score_env(pl, idx_of, T, table, w, dead_value, allowed, features):
    """st_policy_ntuple for one env on env_plies() and its index_batch() entry:
    dict(slot, score, value, best [R], index [T], values_all [S], cand [S],
    dead [S], s1_slot)."""
    f = pl["f"][features]
    S = f.shape[1]
    cand = f[PR.VALID] != 0
    if allowed is not None:
        cand = cand & (np.asarray(allowed) != 0)
    dead = cand & (f[PR.DEAD] != 0)
    s1 = FR.scores_f32(w, f) if w is not None else np.zeros(S, np.float32)
    V = np.zeros(S, np.float32)
    V[dead] = np.float32(dead_value)
    live = np.flatnonzero(cand & ~dead)
    if len(live):
        V[live] = chain(table, np.stack([idx_of[int(s)] for s in live]))
    total = (s1 + V).astype(np.float32)  # one float32 add
    assert total.dtype == s1.dtype == np.float32
    ci = np.flatnonzero(cand)
    out = dict(values_all=V, cand=cand, dead=dead, index=np.full(T, -1, np.int32), best=np.zeros(f.shape[0], np.int32),
               slot=-1, score=np.float32(0.0), value=np.float32(0.0), s1_slot=-1)
    if len(ci):
        s = int(ci[np.argmax(total[ci])])  # the first maximum
        out.update(slot=s, score=total[s], value=V[s], best=f[:, s].astype(np.int32),
                   s1_slot=int(ci[np.argmax(s1[ci])]))
        if not dead[s]:
            out["index"] = idx_of[s].astype(np.int32)
    return out


def score_batch(pb, ib, T, table, w, dead_value, allowed=None, features="base"):
    """score_env over plies_of_state()'s envs and their index_batch() (env e
    plays weight row e % n_w; w None: no weights), stacked as the kernel lays
    them out: slots / actions / scores / values [n], best [R, n], index [T, n],
    values_all [n, S], cand / dead [n, S], s1_slots [n]."""
    n = len(pb["plies"])
    if w is not None:
        w = np.asarray(w, np.float32)
        w = w.reshape(-1, w.shape[-1])
    rs = [score_env(pb["plies"][e], ib[e], T, table, None if w is None else w[e % len(w)], dead_value,
                    None if allowed is None else allowed[e], features) for e in range(n)]
    return dict(slots=np.array([r["slot"] for r in rs], np.int32),
                actions=np.array([FR.action_for(pb["width"], pb["piece"][e], rs[e]["slot"]) for e in range(n)], np.uint8),
                scores=np.array([r["score"] for r in rs], np.float32),
                values=np.array([r["value"] for r in rs], np.float32),
                best=np.stack([r["best"] for r in rs], axis=1), index=np.stack([r["index"] for r in rs], axis=1),
                values_all=np.stack([r["values_all"] for r in rs]), cand=np.stack([r["cand"] for r in rs]),
                dead=np.stack([r["dead"] for r in rs]), s1_slots=np.array([r["s1_slot"] for r in rs], np.int32))
