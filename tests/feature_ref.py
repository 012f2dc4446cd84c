"""The rows of ST_FEATS_BCTS (simpletetris.h, "Feature sets") cell by cell,
shared by test_cpu_features.py and test_gpu_features.py.  A plain module
imported by name, like harness.py and placement_ref.py; it runs no engine code
and needs no GPU.

Rows 0..10 come from placement_ref.slot_features (the oracle plays the slot);
the seven extension rows are counted here from a bool board [W, H] (column x,
row y, y = 0 the top) with loops over cells -- no column words, no popcounts:
independent of the kernel's formulation.
"""
import numpy as np

import placement_ref as PR
from oracle import oracle as O

NF = 18
NBASE = PR.NF
LANDING2, ERODED, ROW_TRANS, COL_TRANS, WELLS, HOLE_DEPTH, HOLE_ROWS = range(NBASE, NF)
EXT_NAMES = ("landing2", "eroded", "row_trans", "col_trans", "wells", "hole_depth", "hole_rows")


def board_rows(text):
    """A bool board [W, H] from rows of '.' / 'X', the top row first."""
    rows = text.split()
    return np.array([[ch == "X" for ch in r] for r in rows], bool).T.copy()


def row_transitions(nb):
    W, H = nb.shape
    t = 0
    for y in range(H):
        prev = True  # the left wall
        for x in range(W):
            t += int(bool(nb[x, y]) != prev)
            prev = bool(nb[x, y])
        t += int(not prev)  # the right wall
    return t


def col_transitions(nb):
    W, H = nb.shape
    t = 0
    for x in range(W):
        for y in range(H):
            below = True if y + 1 == H else bool(nb[x, y + 1])  # the floor
            t += int(bool(nb[x, y]) != below)
    return t


def wells(nb):
    W, H = nb.shape
    total = 0
    for x in range(W):
        d = 0
        for y in range(H + 1):
            cell = y < H and not nb[x, y] and (x == 0 or nb[x - 1, y]) and (x == W - 1 or nb[x + 1, y])
            if cell:
                d += 1
            else:
                total += d * (d + 1) // 2
                d = 0
    return total


def holes(nb):
    """[(x, y, filled cells above)] of every hole."""
    W, H = nb.shape
    out = []
    for x in range(W):
        above = 0
        for y in range(H):
            if nb[x, y]:
                above += 1
            elif above:
                out.append((x, y, above))
    return out


def board_features(nb):
    """(ROW_TRANS, COL_TRANS, WELLS, HOLE_DEPTH, HOLE_ROWS) of a bool board."""
    hs = holes(nb)
    return (row_transitions(nb), col_transitions(nb), wells(nb), sum(h[2] for h in hs), len({h[1] for h in hs}))


def ext_features(board, cells, x, y):
    """The seven extension rows of the placement of `cells` at anchor (x, y)
    (the landing position) on bool board [W, H], and the board after it."""
    W, H = board.shape
    b = board.copy()
    inside = [(x + i, y + j) for i, j in cells if 0 <= x + i < W and 0 <= y + j < H]
    for p in inside:
        b[p] = True
    full = b.all(axis=0)
    keep = b[:, ~full]
    nb = np.zeros_like(b)
    nb[:, H - keep.shape[1]:] = keep
    ys = [y + j for _, j in cells]
    lines = int(full.sum())
    gone = sum(1 for (_, py) in inside if full[py])
    return (2 * H - 1 - (min(ys) + max(ys)), lines * gone) + board_features(nb), nb


def slot_features_bcts(h, board, sid, holes_ctr, piece_height):
    """feat int32 [18, S] of one env: placement_ref.slot_features' rows, then
    the seven extension rows of each valid slot."""
    W, H = board.shape
    per = W + 6
    base = PR.slot_features(h, board, sid, holes_ctr, piece_height)
    feat = np.zeros((NF, base.shape[1]), np.int32)
    feat[:NBASE] = base
    for s in np.flatnonzero(base[PR.VALID]):
        rot, x = s // per, s % per - 3
        cells = O.rotate_cells(O.BASE_SHAPES[sid], rot)
        ext, nb = ext_features(board, cells, x, int(base[PR.Y, s]))
        feat[NBASE:, s] = ext
        assert ext[1] == 0 or base[PR.LINES, s] > 0
        assert int(nb.any(axis=0).sum()) == base[PR.ROWS, s] and len(holes(nb)) == base[PR.HOLES, s]
    return feat


def scores_f32(w, feat):
    """The header's chain over the rows of feat [R, ...] with weights w [R]:
    np.float32 multiply, then np.float32 add, row by row."""
    w = np.asarray(w, np.float32)
    assert len(w) == feat.shape[0]
    acc = np.zeros(feat.shape[1:], np.float32)
    for r in range(len(w)):
        acc = acc + w[r] * feat[r].astype(np.float32)
    assert acc.dtype == np.float32
    return acc


def scores_fused(w, feat):
    """The same sum with each product unrounded (float64 products added into a
    float32 accumulator): what a fused multiply-add chain computes."""
    w = np.asarray(w, np.float32)
    acc = np.zeros(feat.shape[1:], np.float32)
    for r in range(len(w)):
        acc = (acc.astype(np.float64) + np.float64(w[r]) * feat[r].astype(np.float64)).astype(np.float32)
    return acc


def choose(w, feat, allowed=None):
    """(slot, score) of one env: feat int [R, S], w [R], allowed [S] or None;
    the first maximum over the valid and allowed slots, (-1, 0.0) without one."""
    sc = scores_f32(w, feat)
    ok = feat[PR.VALID] != 0
    if allowed is not None:
        ok = ok & (np.asarray(allowed) != 0)
    idx = np.flatnonzero(ok)
    if not len(idx):
        return -1, np.float32(0.0)
    s = int(idx[np.argmax(sc[idx])])
    return s, sc[s]


def action_for(W, piece_word, slot):
    """st_placement_actions's rule for a piece word and a slot."""
    if slot < 0:
        return 2
    per = W + 6
    rot, ax = (int(piece_word) >> 3) & 3, (int(piece_word) >> 5) & 63
    trot, tx = slot // per, slot % per - 3
    return 4 if rot != trot else (1 if ax < tx else (0 if ax > tx else 2))
