"""The lock-position reference (lock_ref.py) on the CPU: the sample holds what
the GPU tests of st_lock_set / st_policy_locks rely on -- tucks that are no
slot's landing in every case, two lock rows in one slot word, a player whose
choice is a tuck -- and the crafted states' lock sets are the ones worked out
by hand."""
import numpy as np
import pytest

import lock_ref as LR
import placement_ref as P
import reach_ref as R


def _tucks(board, config):
    """Per env the lock positions that are no slot's landing."""
    smp, ls = R.sample(board, config), LR.sample(board, config)
    W = R.BOARDS[board][0]
    return [[p for p in lk if not LR.is_landing(smp["valid"][e], smp["Y"][e], W, p)]
            for e, lk in enumerate(ls["locks"])]


@pytest.mark.parametrize("board,config", R.CASES)
def test_sample_has_tucks_and_agrees_with_the_slot_search(board, config):
    smp, ls = R.sample(board, config), LR.sample(board, config)
    W = R.BOARDS[board][0]
    tucks = sum(len(t) for t in _tucks(board, config))
    assert tucks >= 4, tucks
    if board in ("10x20", "11x12"):
        assert tucks >= 90, tucks
    # a slot is reachable iff its landing is a lock position, at the same distance
    for e, lk in enumerate(ls["locks"]):
        for s in np.flatnonzero(smp["valid"][e]):
            p = (int(s) // (W + 6), int(s) % (W + 6) - 3, int(smp["Y"][e, s]))
            assert lk.get(p, 0) == smp["steps"][e, s], (e, s)
        for (r, x, y) in lk:
            assert 0 <= x < W and 0 <= y < R.BOARDS[board][1]
    assert np.array_equal(ls["count"], [sum(bin(int(w)).count("1") for w in row) for row in ls["rows"]])


def test_two_lock_rows_in_one_slot_word():
    rows = LR.sample("10x20", "default")["rows"]
    multi = [(w & (w - 1)).any() for w in rows]
    assert sum(multi) >= 25, sum(multi)


def test_the_deep_player_chooses_tucks():
    total = 0
    for board, config in R.CASES:
        W = R.BOARDS[board][0]
        smp, ls = R.sample(board, config), LR.sample(board, config)
        n = 0
        for e, lk in enumerate(ls["locks"]):
            if not lk:
                continue
            # the deep row: +1 on ST_AFTER_Y, so the score is y; ties to the lowest pos
            best = min(lk, key=lambda p: (-p[2], LR.lock_pos(W, *p)))
            n += not LR.is_landing(smp["valid"][e], smp["Y"][e], W, best)
        if board in ("10x20", "11x12"):
            assert n >= 2, (board, config, n)
        total += n
    assert total >= 30, total


def _crafted(name):
    return next(c for c in R.CRAFTED if c[0] == name)


def _landing_split(case):
    name, cfg, board, sid, rot, x, y, l, _ = case
    valid, Y = R.landings(board.astype(bool), min(sid, 6))
    lk = LR.crafted_locks(case)
    land = {p for p in lk if LR.is_landing(valid, Y, R.CW, p)}
    return lk, land, set(lk) - land


def test_crafted_under_overhang():
    case = _crafted("under_overhang")
    lk, land, tuck = _landing_split(case)
    per = R.CW + 6
    assert {(s // per, s % per - 3) for s in R.UNDER_OVERHANG} == {p[:2] for p in land} and len(land) == 3
    assert tuck == {(0, 0, 8)} and all(v == 1 for v in lk.values())


def test_crafted_spawn_in_stack():
    assert LR.crafted_locks(_crafted("spawn_in_stack")) == {}  # its only lock is the colliding start
    lk, land, tuck = _landing_split(_crafted("spawn_in_stack_lock3"))
    assert len(lk) == 1 and len(land) == 1 and not tuck


def test_crafted_overhang_from_above():
    lk, land, tuck = _landing_split(_crafted("overhang_from_above"))
    assert len(lk) == 19 and tuck == {(1, 3, 8), (3, 0, 8)}
    lk, land, tuck = _landing_split(_crafted("overhang_from_above_lock3"))
    assert len(lk) == 24 and len(tuck) == 8


def test_rows_at_a_landing_are_the_slot_rows():
    """lock_ref.rows_at at a slot's landing equals placement_ref / feature_ref's
    slot rows (the GPU test holds st_afterstates_at to st_afterstates_set there)."""
    import feature_ref as FR
    for board, config in (("6x9", "c4_lock3"), ("10x20", "default")):
        kw = R.case_kw(board, config)
        W = kw["width"]
        smp = R.sample(board, config)
        ob = smp["ob"]
        hk, hp = LR.rows_oracle(kw), P.helper_oracle(kw)
        for e in range(0, R.N, 9):
            env = ob.envs[e]
            b = ob.board(e).astype(bool)
            want = FR.slot_features_bcts(hp, b, env.shape_id, env.holes, env.piece_height)
            for s in np.flatnonzero(smp["valid"][e]):
                got, _ = LR.rows_at(hk, kw, b, env.shape_id, env.holes, env.piece_height, int(s) // (W + 6),
                                    int(s) % (W + 6) - 3, int(smp["Y"][e, s]), features="bcts")
                assert np.array_equal(got, want[:, s]), (board, config, e, s)


def test_position_words():
    for W in (6, 10, 11):
        for rot, x, y in ((0, 0, 0), (3, W - 1, 27), (1, 3, 8)):
            pos = LR.lock_pos(W, rot, x, y)
            assert LR.lock_rot_x_y(W, pos) == (rot, x, y)
            assert pos == (rot * (W + 6) + x + 3) * 32 + y
