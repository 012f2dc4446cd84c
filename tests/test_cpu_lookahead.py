"""The parts of st_next_piece / st_policy_lookahead / st_play_lookahead that
need no GPU: the two-ply reference (lookahead_ref) held to the oracle's own
placement step, hand-made boards, the ABI, and the host layer's argument
checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import feature_ref as FR
import lookahead_ref as LR
import placement_ref as PR
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("st_next_piece", "st_policy_lookahead", "st_play_lookahead")
W, H = 6, 9
O_ID, I_ID = 6, 5


def _kw(config):
    return dict(width=W, height=H, **PR.CONFIGS[config])


def _copy_env(ob, i, kw):
    """Env i of an oracle batch as a one-env batch of its own (a byte copy)."""
    one = O.OracleBatch(1, [0], **kw)
    ctypes.memmove(ctypes.byref(one.envs[0]), ctypes.byref(ob.envs[i]), ctypes.sizeof(O.Env))
    return one


# ------------------------------------------------------------------ X(s1) is the oracle's placement step
@pytest.mark.parametrize("config", sorted(PR.CONFIGS))
def test_the_state_behind_a_slot_is_the_oracles_placement_step(config):
    """4 envs on 6x9, aged 10 greedy placement steps: for every live s1 the
    board and counters lookahead_ref evaluates the second ply on, and the piece
    it places there (next_piece), are what the oracle itself holds after
    ref_place_step(s1) -- the oracle draws that piece, which pins the
    next-piece definition."""
    kw, n = _kw(config), 4
    ob = O.OracleBatch(n, [7300 + e for e in range(n)], **kw)
    ob.reset()
    h = PR.helper_oracle(kw)
    for _ in range(10):
        for i in range(n):
            env = ob.envs[i]
            feat = PR.slot_features(h, ob.board(i).astype(bool), env.shape_id, env.holes, env.piece_height)
            PR.ref_place_step(ob, i, PR.choose(PR.GREEDY, feat), "same_step")
    checked = dead = 0
    for i in range(n):
        env = ob.envs[i]
        board, sid, holes, height = ob.board(i).astype(bool), env.shape_id, env.holes, env.piece_height
        nxt = LR.next_piece(ob, i)
        assert LR.next_piece(ob, i) == nxt and ob.envs[i].shape_id == sid  # the env is not touched
        f1 = PR.slot_features(h, board, sid, holes, height)
        for s1 in np.flatnonzero(f1[PR.VALID]):
            if f1[PR.DEAD, s1]:
                dead += 1
                continue
            b1, holes1, height1, died = LR.state_after(h, board, sid, s1, holes, height)
            one = _copy_env(ob, i, kw)
            _, rew, done, placed = PR.ref_place_step(one, 0, s1, "none")
            assert placed and not done and not died and rew == f1[PR.REWARD, s1]
            assert np.array_equal(one.board(0).astype(bool), b1), (i, s1)
            assert one.envs[0].shape_id == nxt, (i, s1)
            assert (one.envs[0].holes, one.envs[0].piece_height) == (holes1, height1), (i, s1)
            checked += 1
    print("X(s1)", config, "live slots", checked, "dead slots", dead)
    assert checked >= 4 * 9


def test_next_piece_follows_a_reset_too():
    """The piece a reset spawns is the one next_piece named before it."""
    kw = _kw("default")
    ob = O.OracleBatch(3, [7400, 7401, 7402], **kw)
    ob.reset()
    for t in range(12):
        for i in range(3):
            want = LR.next_piece(ob, i)
            if (t + i) % 3 == 0:
                ob.reset(i)
                assert ob.envs[i].shape_id == want
            else:
                counts = sum(ob.envs[i].counts)
                ob.step_one(i, 2)
                if sum(ob.envs[i].counts) != counts:  # the drop locked and spawned
                    assert ob.envs[i].shape_id == want


# ------------------------------------------------------------------ hand-made boards
def _tall_board():
    """Rows 1..8 filled but for two covered gaps each (no row can be completed
    by one piece): only row 0 is free, so whatever locks reaches into row 0."""
    b = np.ones((W, H), bool)
    b[:, 0] = False
    for y in range(1, H):
        b[(y % 2) * 1, y] = False
        b[3 + (y % 2), y] = False
    return b


def test_every_first_ply_slot_dies():
    h = PR.helper_oracle(_kw("default"))
    w = PR.GREEDY
    for sid in range(7):
        r = LR.lookahead(h, _tall_board(), sid, I_ID, 0, 0, w, w, -1.0e6)
        assert r["cand"].any() and np.array_equal(r["dead"], r["cand"]), sid
        assert (r["slots2_all"] == -1).all() and r["slot2"] == -1
        f1 = PR.slot_features(h, _tall_board(), sid, 0, 0)
        s1 = FR.scores_f32(w, f1)
        for s in np.flatnonzero(r["cand"]):
            assert r["scores_all"][s] == np.float32(s1[s]) + np.float32(-1.0e6)
        # the choice is the one-ply choice: the tail is one constant (up to the add's rounding)
        assert r["slot"] == int(np.flatnonzero(r["cand"])[np.argmax(r["scores_all"][r["cand"]])])
        assert r["score"] == r["scores_all"][r["slot"]]
        # without first-ply weights every candidate scores dead_value: the lowest slot
        r0 = LR.lookahead(h, _tall_board(), sid, I_ID, 0, 0, None, w, -5.0)
        assert r0["slot"] == int(np.flatnonzero(r0["cand"])[0]) and r0["score"] == np.float32(-5.0)


def test_a_live_first_ply_slot_always_leaves_a_valid_second_ply_slot():
    """The case "s1 is not dead but no s2 is valid" cannot be built: a lock
    that does not kill leaves row 0 empty (tetris_env.py:277), and every
    shape in its spawn rotation has all its cells in rows <= 0 of its anchor,
    so at anchor row 0 it is unoccupied at some column of any board with row 0
    empty.  Held here on the tallest boards the game allows: every live s1 of
    every piece on a board whose rows 1.. are filled up to two gaps has a valid
    s2 for every next piece; the kernel's dead_value for that case is defence."""
    h = PR.helper_oracle(_kw("default"))
    b = _tall_board()
    b[:, 1:5] = False  # four free rows over a ragged stack: live and dead first-ply slots
    b[0, 3:5] = True
    seen = 0
    for sid in range(7):
        f1 = PR.slot_features(h, b, sid, 0, 0)
        for s1 in np.flatnonzero(f1[PR.VALID] & (f1[PR.DEAD] == 0)):
            b1, holes1, height1, died = LR.state_after(h, b, sid, s1, 0, 0)
            assert not died and not b1[:, 0].any()
            for nxt in range(7):
                cells = O.BASE_SHAPES[nxt]
                assert any(not PR.occupied(cells, x, 0, b1) for x in range(W)), (sid, s1, nxt)
            seen += 1
    assert seen > 20


def test_lookahead_and_one_ply_disagree():
    """Four rows complete but for column 0, the O in play and the I next,
    weights on LINES alone: no O placement clears a line, so one ply takes the
    lowest valid slot -- which covers the well; two plies keep the well open
    for the I and its four lines."""
    h = PR.helper_oracle(_kw("default"))
    b = np.zeros((W, H), bool)
    b[1:, H - 4:] = True
    w = np.zeros(PR.NF, np.float32)
    w[PR.LINES] = 1.0
    f1 = PR.slot_features(h, b, O_ID, 0, 0)
    one_ply = PR.choose(w, f1)
    assert one_ply == 0 * (W + 6) + 1 + 3  # rotation 0 at x = 1: columns 0 and 1
    r = LR.lookahead(h, b, O_ID, I_ID, 0, 0, None, w, -1.0e6)
    assert r["slot"] != one_ply and r["score"] == 4.0 and r["scores_all"][one_ply] == 1.0  # (an I across the O's top row)
    rot, x = PR.decode(W, r["slot"])
    cols = {x + i for i, _ in O.rotate_cells(O.BASE_SHAPES[O_ID], rot)}
    assert 0 not in cols
    rot2, x2 = PR.decode(W, r["slot2"])
    assert {x2 + i for i, _ in O.rotate_cells(O.BASE_SHAPES[I_ID], rot2)} == {0}
    # with the mask on the two-ply choice alone, the next candidate wins; a mask of zeros leaves none
    allowed = np.ones(4 * (W + 6), np.int32)
    allowed[r["slot"]] = 0
    r2 = LR.lookahead(h, b, O_ID, I_ID, 0, 0, None, w, -1.0e6, allowed)
    assert r2["slot"] > r["slot"] and r2["score"] == 4.0 and r2["scores_all"][r["slot"]] == 0.0
    r3 = LR.lookahead(h, b, O_ID, I_ID, 0, 0, None, w, -1.0e6, np.zeros_like(allowed))
    assert (r3["slot"], r3["slot2"], float(r3["score"])) == (-1, -1, 0.0) and not r3["scores_all"].any()
    # the bcts rows give the same choice under the same weights (rows 0..10 are the base rows)
    w18 = np.zeros(FR.NF, np.float32)
    w18[PR.LINES] = 1.0
    rb = LR.lookahead(h, b, O_ID, I_ID, 0, 0, None, w18, -1.0e6, features="bcts")
    assert (rb["slot"], rb["slot2"]) == (r["slot"], r["slot2"])


# ------------------------------------------------------------------ the ABI
def _lib():
    from gym_simpletetris_amd import _lib as C
    return C, C.load()


def _call(L, call, ctx, fset=0, w2=None, n_w=1, dead=-1.0, out=True):
    buf = (ctypes.c_uint32 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p) if out else None
    if call == "st_next_piece":
        return L.st_next_piece(ctx, p, None)
    if call == "st_policy_lookahead":
        return L.st_policy_lookahead(ctx, fset, None, w2, n_w, dead, None, p, None, None, None, None, None, None)
    return L.st_play_lookahead(ctx, fset, None, w2, n_w, dead, 1, p, None, None, None, None, None)


@pytest.mark.parametrize("call", NEW_CALLS)
def test_argument_errors_come_before_any_gpu_call(call):
    """A zeroed block stands in for a context: were it used, it would say
    "not seeded" (ST_ESTATE), which is what good arguments then give."""
    C, L = _lib()
    w = ctypes.cast((ctypes.c_float * 18)(), ctypes.c_void_p)
    assert _call(L, call, None, 0, w) == C.ST_EINVAL
    assert call.encode() in L.st_last_error()
    ctx = ctypes.cast((ctypes.c_uint64 * 512)(), ctypes.c_void_p)
    assert _call(L, call, ctx, 0, w) == C.ST_ESTATE
    assert call.encode() in L.st_last_error()
    if call == "st_next_piece":
        assert _call(L, call, ctx, out=False) == C.ST_EINVAL
        return
    assert _call(L, call, ctx, 1, w) == C.ST_ESTATE
    for bad in (-1, 2, 77):
        assert _call(L, call, ctx, bad, w) == C.ST_EINVAL
        assert b"feature set" in L.st_last_error()
    assert _call(L, call, ctx, 0, None) == C.ST_EINVAL
    assert _call(L, call, ctx, 0, w, 0) == C.ST_EINVAL
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert _call(L, call, ctx, 0, w, 1, bad) == C.ST_EINVAL
        assert b"dead_value" in L.st_last_error() and call.encode() in L.st_last_error()
    if call == "st_policy_lookahead":
        assert _call(L, call, ctx, 0, w, out=False) == C.ST_EINVAL
        assert b"output" in L.st_last_error()


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    C, L = _lib()
    assert L.st_abi_version() == C.ABI_VERSION == 4
    text = open(os.path.join(ROOT, "include", "simpletetris.h")).read()
    for name in NEW_CALLS:
        assert name in C.SIG and hasattr(L, name) and getattr(L, name).argtypes == C.SIG[name][0]
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    head = text[:text.index("#define ST_ABI_VERSION")]
    assert all(name in head for name in NEW_CALLS)  # the version comment lists them


# ------------------------------------------------------------------ the host layer
def test_methods_reject_bad_arguments_before_any_device_call():
    import torch
    from gym_simpletetris_amd.engine import LookaheadChoice, TetrisBatch

    class Stub:
        n, width, n_slots, device = 4, 10, 64, torch.device("cpu")
        _weights = TetrisBatch._weights
        _lookahead_weights = TetrisBatch._lookahead_weights

    stub = Stub()
    w11, w18 = [0.0] * 11, [0.0] * 18
    calls = (lambda **k: TetrisBatch.policy_lookahead(stub, **k), lambda **k: TetrisBatch.play_lookahead(stub, k=1, **k))
    for call in calls:
        for bad in ("dellacherie", "BCTS", None, 1):
            with pytest.raises(ValueError, match="features"):
                call(weights=w11, features=bad)
        with pytest.raises(ValueError):  # eleven weights for eighteen rows
            call(weights=w11, features="bcts")
        with pytest.raises(ValueError, match="first_weights"):  # another shape
            call(weights=[w11, w11], first_weights=w11)
        with pytest.raises(ValueError):
            call(weights=w18, first_weights=w11, features="bcts")
        for bad in (float("inf"), float("nan"), 1.0e39):
            with pytest.raises(ValueError, match="dead_value"):
                call(weights=w11, dead_value=bad)
        for bad in ("0", None, True):
            with pytest.raises(TypeError, match="dead_value"):
                call(weights=w11, dead_value=bad)
        with pytest.raises((ValueError, TypeError)):  # a float64 tensor is not converted
            call(weights=torch.zeros(11, dtype=torch.float64))
    for bad in (torch.ones((4, 63), dtype=torch.int32), torch.ones((3, 64), dtype=torch.int32),
                torch.ones((4, 64), dtype=torch.int64), np.ones((4, 64), np.int32)):
        with pytest.raises((ValueError, TypeError)):
            TetrisBatch.policy_lookahead(stub, w11, allowed=bad)
    i32, f32 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float32)
    u8 = torch.zeros(4, dtype=torch.uint8)
    for bad in ((i32, i32, u8), (None, None, None, None), (i32, i32, u8, f32, None, None), (f32, i32, u8, f32),
                (i32, i32, u8, torch.zeros(5, dtype=torch.float32))):
        with pytest.raises(ValueError):
            TetrisBatch.policy_lookahead(stub, w11, out=bad)
    with pytest.raises(ValueError):  # the table's tensors have S columns
        TetrisBatch.policy_lookahead(stub, w11, table=True, out=(i32, i32, u8, f32, torch.zeros((4, 63)), None))
    for bad_k in (-1, 1.5, True):
        with pytest.raises(ValueError):
            TetrisBatch.play_lookahead(stub, w11, bad_k)
    with pytest.raises(ValueError):
        TetrisBatch.play_lookahead(stub, w11, 1, obs="f32")
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)):
        with pytest.raises(ValueError):
            TetrisBatch.play_lookahead(stub, w11, 1, returns=bad)
    with pytest.raises(ValueError):
        TetrisBatch.next_piece(stub, out=torch.zeros(4, dtype=torch.int32))
    c = LookaheadChoice(1, 2, 3, 4)
    assert (c.slots, c.slots2, c.actions, c.scores, c.scores_all, c.slots2_all) == (1, 2, 3, 4, None, None)
