"""The parts of st_next_weights / st_policy_expect / st_play_expect that need
no GPU: the odds held to the oracle's own draw, the expectimax reference
(expect_ref) on hand-made boards, the ABI, and the host layer's argument
checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import expect_ref as EX
import feature_ref as FR
import lookahead_ref as LR
import placement_ref as PR
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("st_next_weights", "st_policy_expect", "st_play_expect")
W, H = 6, 9
O_ID, I_ID = 6, 5


def _kw(config="default"):
    return dict(width=W, height=H, **PR.CONFIGS[config])


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the odds
def test_weights_are_the_reference_rule_on_hand_written_counts():
    assert EX.weights_of([0] * 7) == [5] * 7
    assert EX.weights_of([3] * 7) == [5] * 7  # equal counts: all 5s, whatever the count
    assert EX.weights_of([40, 0, 0, 0, 0, 0, 0]) == [5, 45, 45, 45, 45, 45, 45]
    assert EX.weights_of([2, 0, 1, 5, 3, 4, 5]) == [8, 10, 9, 5, 7, 6, 5]
    assert min(EX.weights_of([7, 1, 9, 0, 2, 2, 30])) == 5


def test_weights_reproduce_the_piece_the_oracle_draws():
    """On byte copies of aged oracle envs: randint(1, sum(m)) from the env's own
    MT19937 state, walked down the weight list (tetris_env.py:187-191), names
    the piece the oracle's clear() spawns -- so m is the distribution of the
    next piece, behind a lock or a reset."""
    kw, n = _kw(), 6
    ob = O.OracleBatch(n, [9100 + e for e in range(n)], **kw)
    ob.reset()
    seen = set()
    for t in range(40):
        for i in range(n):
            m = EX.next_weights(ob, i)
            assert m.min() == 5 and list(m) == EX.weights_of(ob.envs[i].counts)
            e = O.Env.from_buffer_copy(ob.envs[i])
            r = 1 + int(O.lib().or_mt_randbelow(ctypes.byref(e.rng), int(m.sum())))
            pick = next(q for q in range(7) if r <= int(m[:q + 1].sum()))
            assert pick == LR.next_piece(ob, i), (t, i)
            seen.add(tuple(m))
            ob.step_one(i, 2)
    assert len(seen) > 10  # the odds moved


# ------------------------------------------------------------------ hand-made boards
def well_board():
    """Four rows complete but for column 0 (test_cpu_lookahead's board)."""
    b = np.zeros((W, H), bool)
    b[1:, H - 4:] = True
    return b


WELL_COUNTS = (9, 9, 9, 9, 9, 0, 9)   # the I is overdue: m = 5 but for the I's 14
LINES_ONLY = np.zeros(PR.NF, np.float32)
LINES_ONLY[PR.LINES] = 1.0


def test_expectimax_one_ply_and_known_piece_disagree():
    """The O in play on well_board(), weights on LINES alone: one ply takes the
    lowest valid slot, which covers the well; the expectimax keeps the well open
    (every piece but the O can clear there, the I four lines); and with the O
    known to come next every slot scores 0, so the known-piece player covers the
    well too.  The GPU test runs the same input."""
    h = PR.helper_oracle(_kw())
    b, w = well_board(), LINES_ONLY
    f1 = PR.slot_features(h, b, O_ID, 0, 0)
    one_ply = PR.choose(w, f1)
    pl = EX.plies(h, b, O_ID, 0, 0)
    m = EX.weights_of(WELL_COUNTS)
    assert m == [5, 5, 5, 5, 5, 14, 5]
    r = EX.score(pl, m, None, w, -1.0e6)
    assert r["slot"] != one_ply
    rot, x = PR.decode(W, r["slot"])
    assert 0 not in {x + i for i, _ in O.rotate_cells(O.BASE_SHAPES[O_ID], rot)}  # the well stays open
    assert r["tails"][I_ID, r["slot"]] == 4.0 and r["tails"][O_ID, r["slot"]] == 0.0
    assert 0.0 < r["score"] < 4.0 and r["scores_all"][one_ply] < r["score"]
    # the known-next-piece player's choices, piece by piece
    known = [LR.score(EX.as_lookahead(pl, q), None, w, -1.0e6)["slot"] for q in range(7)]
    assert known[O_ID] == one_ply != r["slot"]
    print("expectimax", r["slot"], float(r["score"]), "one ply", one_ply, "known piece", known)
    # each piece's tail is the known-piece player's table (float32 values: 0.0f + T)
    for q in range(7):
        la = LR.score(EX.as_lookahead(pl, q), None, w, -1.0e6)
        assert np.array_equal(la["scores_all"], r["tails"][q]) and np.array_equal(la["slots2_all"], r["slots2_all"][q])
    # the score is the chain, not a float64 mean
    s = r["slot"]
    assert _bits(r["scores_all"][s]) == _bits(np.float32(0.0) + EX.chain(m, r["tails"][:, s]))
    # the odds decide: with the I just as likely as the rest the margin shrinks but the order of E is the chain's
    r5 = EX.score(pl, [5] * 7, None, w, -1.0e6)
    assert r5["scores_all"][s] < r["scores_all"][s]
    # a mask on the chosen slot moves the choice on; a mask of zeros leaves none
    allowed = np.ones(4 * (W + 6), np.int32)
    allowed[s] = 0
    r2 = EX.score(pl, m, None, w, -1.0e6, allowed)
    assert r2["slot"] not in (-1, s) and r2["scores_all"][s] == 0.0 and (r2["slots2_all"][:, s] == -1).all()
    r3 = EX.score(pl, m, None, w, -1.0e6, np.zeros_like(allowed))
    assert (r3["slot"], float(r3["score"])) == (-1, 0.0) and not r3["scores_all"].any() and not r3["tails"].any()


def tall_board():
    """Rows 1..8 filled but for two covered gaps each (test_cpu_lookahead's):
    whatever locks reaches into row 0."""
    b = np.ones((W, H), bool)
    b[:, 0] = False
    for y in range(1, H):
        b[(y % 2) * 1, y] = False
        b[3 + (y % 2), y] = False
    return b


TALL_COUNTS = (2, 0, 1, 5, 3, 4, 5)   # m = 8 10 9 5 7 6 5, M = 50
TALL_DEAD = -123.456
TALL_CHAIN_BITS = 0xC2F6E978


def test_chain_of_a_constant_is_not_the_constant():
    """chain(dead_value) with m = 8 10 9 5 7 6 5 and dead_value = -123.456f =
    0xc2f6e979 is 0xc2f6e978, one unit in the last place off; with equal odds
    and -1.0e6 it is -1.0e6 exactly."""
    m = EX.weights_of(TALL_COUNTS)
    assert m == [8, 10, 9, 5, 7, 6, 5]
    e = EX.chain(m, [np.float32(TALL_DEAD)] * 7)
    assert _bits(np.float32(TALL_DEAD)) == 0xC2F6E979
    assert _bits(e) == TALL_CHAIN_BITS != 0xC2F6E979
    assert EX.chain([5] * 7, [np.float32(-1.0e6)] * 7) == np.float32(-1.0e6)


def test_every_first_ply_slot_dies():
    """Every score is S1 + chain(dead_value), every tail dead_value, every
    second-ply slot -1."""
    h = PR.helper_oracle(_kw())
    w = PR.GREEDY
    m = EX.weights_of(TALL_COUNTS)
    e = EX.chain(m, [np.float32(TALL_DEAD)] * 7)
    for sid in range(7):
        r = EX.expect(h, tall_board(), sid, TALL_COUNTS, 0, 0, w, w, TALL_DEAD)
        assert r["cand"].any() and np.array_equal(r["dead"], r["cand"]), sid
        assert (r["slots2_all"] == -1).all()
        s1 = FR.scores_f32(w, PR.slot_features(h, tall_board(), sid, 0, 0))
        for s in np.flatnonzero(r["cand"]):
            assert _bits(r["scores_all"][s]) == _bits(np.float32(s1[s]) + e)
            assert (_bits(r["tails"][:, s]) == _bits(np.float32(TALL_DEAD))).all()
        assert r["slot"] == int(np.flatnonzero(r["cand"])[np.argmax(r["scores_all"][r["cand"]])])
        # without first-ply weights every candidate scores the chain's value: the lowest slot
        r0 = EX.expect(h, tall_board(), sid, TALL_COUNTS, 0, 0, None, w, TALL_DEAD)
        assert r0["slot"] == int(np.flatnonzero(r0["cand"])[0]) and _bits(r0["score"]) == TALL_CHAIN_BITS


# ------------------------------------------------------------------ the ABI
def _lib():
    from gym_simpletetris_amd import _lib as C
    return C, C.load()


def _call(L, call, ctx, fset=0, w2=None, n_w=1, dead=-1.0, out=True):
    buf = (ctypes.c_uint32 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p) if out else None
    if call == "st_next_weights":
        return L.st_next_weights(ctx, p, None)
    if call == "st_policy_expect":
        return L.st_policy_expect(ctx, fset, None, w2, n_w, dead, None, p, None, None, None, None, None, None)
    return L.st_play_expect(ctx, fset, None, w2, n_w, dead, 1, p, None, None, None, None, None)


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
    if call == "st_next_weights":
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
    if call == "st_policy_expect":
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
    assert len(C.SIG["st_policy_expect"][0]) == 14 and len(C.SIG["st_play_expect"][0]) == 13


# ------------------------------------------------------------------ the host layer
def test_methods_reject_bad_arguments_before_any_device_call():
    import torch
    from gym_simpletetris_amd.engine import ExpectChoice, TetrisBatch

    class Stub:
        n, width, n_slots, device = 4, 10, 64, torch.device("cpu")
        _weights = TetrisBatch._weights
        _lookahead_weights = TetrisBatch._lookahead_weights

    stub = Stub()
    w11, w18 = [0.0] * 11, [0.0] * 18
    calls = (lambda **k: TetrisBatch.policy_expect(stub, **k), lambda **k: TetrisBatch.play_expect(stub, k=1, **k))
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
            TetrisBatch.policy_expect(stub, w11, allowed=bad)
    i32, f32 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float32)
    u8 = torch.zeros(4, dtype=torch.uint8)
    for bad in ((i32, u8), (None, None, None), (i32, u8, f32, None, None, None), (f32, u8, f32),
                (i32, u8, torch.zeros(5, dtype=torch.float32)), (i32, i32, f32)):
        with pytest.raises(ValueError):
            TetrisBatch.policy_expect(stub, w11, out=bad)
    with pytest.raises(ValueError):  # the six-tuple goes with table=True
        TetrisBatch.policy_expect(stub, w11, table=True, out=(i32, u8, f32))
    with pytest.raises(ValueError):  # the tails are [n, 7, S]
        TetrisBatch.policy_expect(stub, w11, table=True, out=(i32, u8, f32, None, torch.zeros((4, 64)), None))
    with pytest.raises(ValueError):
        TetrisBatch.policy_expect(stub, w11, table=True,
                                  out=(None, None, None, None, None, torch.zeros((4, 7, 63), dtype=torch.int32)))
    for bad_k in (-1, 1.5, True):
        with pytest.raises(ValueError):
            TetrisBatch.play_expect(stub, w11, bad_k)
    with pytest.raises(ValueError):
        TetrisBatch.play_expect(stub, w11, 1, obs="f32")
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)):
        with pytest.raises(ValueError):
            TetrisBatch.play_expect(stub, w11, 1, returns=bad)
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros((7, 4), dtype=torch.uint8),
                torch.zeros((4, 7), dtype=torch.int32)):
        with pytest.raises(ValueError):
            TetrisBatch.next_weights(stub, out=bad)
    c = ExpectChoice(1, 2, 3)
    assert (c.slots, c.actions, c.scores, c.scores_all, c.tails, c.slots2_all) == (1, 2, 3, None, None, None)
