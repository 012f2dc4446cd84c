"""The ST_FEATS_BCTS feature set on the device (st_afterstates_set,
st_policy_linear_set, st_play_linear_set; TetrisBatch.afterstates /
policy_linear / play_linear with features='bcts', and policy_linear's
`allowed` mask) against feature_ref.py: rows 0..10 from the oracle playing
every slot, rows 11..17 counted cell by cell.
"""
import ctypes

import numpy as np
import pytest

import feature_ref as FR
import placement_ref as PR
from harness import (C4, assert_same_state, cached_ref, check_engine_state, check_mt_state, check_step,
                     engine as _engine, engine_state, pack_cols)
from oracle import oracle as O

NF, NB = FR.NF, FR.NBASE
NAMES = ("valid", "y", "lines", "holes", "height", "rows", "above", "dead", "reward", "agg_height",
         "bumpiness") + FR.EXT_NAMES


def _bool_board(words, H):
    return ((np.asarray(words, np.uint64)[:, None] >> np.arange(H, dtype=np.uint64)) & 1).astype(bool)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def mixed_actions(b, t, aseed):
    """Step t's actions: the first half of the envs play policy_greedy
    (explore 30 per mille), the second half uniform gen_actions."""
    import torch
    g = b.policy_greedy(t, seed=aseed, explore=30).clone()
    u = b.gen_actions(t, aseed)
    return torch.where(torch.arange(b.n, device=b.device) < b.n // 2, g, u)


def aged(n, kw, seed0, aseed, steps, autoreset="same_step"):
    b = _engine().TetrisBatch(n, autoreset=autoreset, seeds=[seed0 + e for e in range(n)], **kw)
    b.reset()
    for t in range(steps):
        b.step(mixed_actions(b, t, aseed), obs="none")
    return b


# ------------------------------------------------------------------ 1. evolved states
EVOLVED = {
    "10x20_c4": (48, dict(width=10, height=20, **C4), 4200, 11, (40, 90, 140, 199)),
    "7x12_holes_step": (48, dict(width=7, height=12, penalise_holes=True, reward_step=True), 5200, 12,
                        (40, 90, 140, 199)),
    "13x26_height_adv": (48, dict(width=13, height=26, penalise_height_increase=True, advanced_clears=True), 6200,
                         13, (60, 110, 160, 199)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EVOLVED))
def test_oracle_parity_on_evolved_states(name):
    """All 18 rows of every slot of every third env at four checkpoints of a
    half-greedy, half-uniform run; the boards are the base call's."""
    n, kw, seed0, aseed, cps = EVOLVED[name]
    H = kw["height"]
    h = PR.helper_oracle(kw)
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[seed0 + e for e in range(n)], **kw)
    seen = np.zeros(NF, np.int64)
    try:
        b.reset()
        for t in range(cps[-1] + 1):
            if t in cps:
                st = b.get_state(("board", "piece", "stats"))
                a = b.afterstates(features="bcts")
                assert a.feat.shape == (n, NF, b.n_slots)
                feat = a.feat.cpu().numpy()
                for e in range(0, n, 3):
                    want = FR.slot_features_bcts(h, _bool_board(st["board"][:, e], H), int(st["piece"][e] & 7),
                                                 int(st["stats"][3, e]), int(st["stats"][4, e]))
                    for r in range(NF):
                        assert np.array_equal(feat[e, r], want[r]), (name, t, "env", e, NAMES[r], feat[e, r], want[r])
                    seen = np.maximum(seen, want.max(axis=1))
                old = b.afterstates()
                assert (a.boards == old.boards).all() and (a.feat[:, :NB] == old.feat).all()
            b.step(mixed_actions(b, t, aseed), obs="none")
    finally:
        b.close()
    print(name, "largest value per row:", dict(zip(NAMES, seen.tolist())))
    assert (seen[NB:] >= 1).all(), seen  # (the crafted boards hold the larger values)


# ------------------------------------------------------------------ 2. crafted boards
def crafted_cases(W, H):
    """[(name, board u8 [W, H], piece id)], for W >= 4 and H >= 12."""
    cases = []
    c = W // 2
    for k, rows in enumerate((0b0100, 0b0101, 0b1011, 0b1111), start=1):
        # an upright I into a one-column well under four rows, k of them full but for the well:
        # k rows clear with k of the I's cells in them, ERODED k * k
        b = np.zeros((W, H), np.uint8)
        for r in range(4):
            b[:, H - 4 + r] = 1
            if not (rows >> r) & 1:
                b[(c + 1) % W, H - 4 + r] = 0
        b[c, H - 4:] = 0
        cases.append(("clear%d" % k, b, 5))
    # a clear that removes a hole: the hole (3, H-1) lies under the row that clears
    b = np.zeros((W, H), np.uint8)
    b[:, H - 2:] = 1
    b[0, H - 2] = 0
    b[3, H - 1] = 0
    cases.append(("hole_clear", b, 5))
    # a well of depth 5 at the left wall, and a covered well of depth 3 in column 2 (its three cells are holes)
    b = np.zeros((W, H), np.uint8)
    b[1, H - 5:] = 1
    b[3, H - 5:] = 1
    b[2, H - 4] = 1
    cases.append(("wells", b, 6))
    # two holes in column 1, one and two filled cells above them
    b = np.zeros((W, H), np.uint8)
    b[1, H - 2] = b[1, H - 4] = 1
    cases.append(("holes2", b, 6))
    # a stack to rows 2 / 1 with two free columns: an upright I lands with cells above row 0
    b = np.zeros((W, H), np.uint8)
    b[: W // 2, 2:] = 1
    b[W // 2:, 1:] = 1
    b[W - 2:, :] = 0
    cases.append(("stack", b, 5))
    # row 0 blocks every slot
    b = np.zeros((W, H), np.uint8)
    b[:, 0] = 1
    cases.append(("blocked", b, 1))
    return cases


def crafted_ref(W, H):
    """{case name: feat int32 [18, S]} by the reference, with counters holes =
    5, piece_height = 3 (what crafted_batch writes), computed once."""
    def make():
        h = PR.helper_oracle(dict(width=W, height=H, **C4))
        return {name: FR.slot_features_bcts(h, board.astype(bool), sid, 5, 3)
                for name, board, sid in crafted_cases(W, H)}
    return cached_ref(("features_crafted", W, H), make)


def crafted_batch(W, H, n, first=0, **extra):
    """Env i holds case (first + i) mod the number of cases."""
    cases = crafted_cases(W, H)
    pick = [cases[(first + i) % len(cases)] for i in range(n)]
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[77 + e for e in range(n)], width=W, height=H, **C4,
                              **extra)
    b.reset()
    st = b.get_state(("board", "piece", "stats"))
    st["board"][:] = np.stack([pack_cols(c[1]) for c in pick], axis=1)
    st["piece"][:] = (st["piece"] & ~np.uint32(7)) | np.array([c[2] for c in pick], np.uint32)
    st["stats"][3], st["stats"][4] = 5, 3
    b.set_state(**st)
    return b, [c[0] for c in pick]


def test_crafted_cases_reach_what_they_are_for():
    """Needs no GPU: by the reference alone the crafted set holds clears of
    1..4 rows with ERODED 1, 4, 9, 16, a hole removed by a clear, a well run of
    depth >= 3, a covered well cell, two holes of different depth in one
    column, a placement with cells above row 0, a board without a valid slot,
    and a value >= 2 in every new row."""
    for W, H in ((4, 12), (10, 20)):
        got = crafted_ref(W, H)
        per, c = W + 6, W // 2
        upright = [r for r in range(4) if len({i for i, _ in O.rotate_cells(O.BASE_SHAPES[5], r)}) == 1]
        for k in range(1, 5):
            f = got["clear%d" % k]
            for r in upright:
                s = r * per + c + 3
                assert f[PR.VALID, s] == 1 and f[PR.LINES, s] == k and f[FR.ERODED, s] == k * k, (W, k, r)
        f = got["hole_clear"]
        s = upright[0] * per + 3
        assert f[PR.LINES, s] == 1 and f[PR.HOLES, s] == 0 and f[FR.HOLE_ROWS, s] == 0 and f[FR.HOLE_DEPTH, s] == 0
        assert f[PR.HOLES][f[PR.VALID] == 1].max() > 0 and f[FR.ERODED, s] == 1
        # the wells board itself: 5 * 6 / 2 at the wall + 3 * 4 / 2 covered; its three holes lie one cell deep
        wb = dict((n_, b_) for n_, b_, _ in crafted_cases(W, H))["wells"].astype(bool)
        assert FR.wells(wb) >= 15 + 6 and [h_[2] for h_ in FR.holes(wb)] == [1, 1, 1]
        f = got["wells"]
        assert f[FR.WELLS].max() >= 21 and f[FR.WELLS][f[PR.VALID] == 1].min() >= 3
        hb = dict((n_, b_) for n_, b_, _ in crafted_cases(W, H))["holes2"].astype(bool)
        assert sorted(h_[2] for h_ in FR.holes(hb)) == [1, 2] and len({h_[0] for h_ in FR.holes(hb)}) == 1
        f = got["holes2"]
        assert f[FR.HOLE_DEPTH].max() >= 3 and f[FR.HOLE_ROWS].max() >= 2
        f = got["stack"]
        neg = (f[PR.VALID] == 1) & (f[PR.ABOVE] == 1)
        assert neg.any() and (f[FR.LANDING2][neg] >= 2 * H - 1 - (-1 + 2)).all()  # ymin <= -1 over a top at row <= 2
        assert f[FR.LANDING2][neg].max() >= 2 * H  # the upright I on the stack: rows -2..1
        assert not got["blocked"].any()
        top = np.max([f_.max(axis=1) for f_ in got.values()], axis=0)
        assert (top[NB:] >= 2).all(), top


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,n,first", [(4, 12, 70, 0), (10, 20, 70, 0), (10, 20, 1, 3), (32, 28, 70, 0),
                                         (32, 28, 1, 3)],
                         ids=["4x12_n70", "10x20_n70", "10x20_n1", "32x28_n70", "32x28_n1"])
def test_crafted_boards(W, H, n, first):
    """Every crafted case, all slots and all 18 rows, into caller tensors with
    room behind them (nothing is written past n envs); n = 1 is the four-row
    clear.  4x12 has S = 40 (lanes without a slot), 32x28 three passes and the
    floor bit at bit 28."""
    import torch
    b, names = crafted_batch(W, H, n, first)
    try:
        S = b.n_slots
        pad = 3 * S
        fbuf = torch.full((n * NF * S + pad,), -7, dtype=torch.int32, device=b.device)
        bbuf = torch.full((n * W * S + pad,), -7, dtype=torch.int32, device=b.device)
        out = (fbuf[: n * NF * S].view(n, NF, S), bbuf[: n * W * S].view(n, W, S))
        a = b.afterstates(out=out, features="bcts")
        assert a.feat is out[0] and a.boards is out[1]
        feat = a.feat.cpu().numpy()
        ref = crafted_ref(W, H)
        for e, name in enumerate(names):
            for r in range(NF):
                assert np.array_equal(feat[e, r], ref[name][r]), (name, "env", e, NAMES[r], feat[e, r], ref[name][r])
        assert (fbuf[n * NF * S:] == -7).all() and (bbuf[n * W * S:] == -7).all()
        assert n > 1 or names == ["clear4"]
        old = b.afterstates()
        assert torch.equal(a.boards, old.boards)
        no_boards = b.afterstates(boards=False, features="bcts")
        assert no_boards.boards is None and torch.equal(no_boards.feat, a.feat)
        assert torch.equal(no_boards.wells, a.feat[:, FR.WELLS]) and torch.equal(no_boards.lines, old.lines)
    finally:
        b.close()


# ------------------------------------------------------------------ 3. the base set through the new entry point
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(10, 20), (13, 26)])
def test_base_set_through_the_new_entry_point_is_the_old_call(W, H):
    """st_afterstates_set(ST_FEATS_BASE) and st_afterstates: features and
    boards bit for bit, into guarded buffers."""
    import torch
    n = 70
    b = aged(n, dict(width=W, height=H, **C4), 4300, 21, 120)
    try:
        S = b.n_slots
        old = b.afterstates()
        fbuf = torch.full((n * NB * S + 64,), -7, dtype=torch.int32, device=b.device)
        bbuf = torch.full((n * W * S + 64,), -7, dtype=torch.int32, device=b.device)
        assert b._L.st_afterstates_set(b._ctx, 0, _ptr(fbuf), _ptr(bbuf), b._stream()) == 0
        assert torch.equal(fbuf[: n * NB * S].view(n, NB, S), old.feat) and (fbuf[n * NB * S:] == -7).all()
        assert torch.equal(bbuf[: n * W * S].view(n, W, S), old.boards) and (bbuf[n * W * S:] == -7).all()
        new = b.afterstates(features="bcts")
        assert torch.equal(new.boards, old.boards) and torch.equal(new.feat[:, :NB], old.feat)
    finally:
        b.close()


# ------------------------------------------------------------------ 4. policy_linear over 18 rows
def mixed_weights(n_w, seed=5):
    """n_w rows of mixed-sign float32 weights whose products do not fit a
    float32 exactly (so that a fused chain rounds differently)."""
    rng = np.random.default_rng(seed)
    w = rng.normal(0.0, 3.0, (n_w, NF)).astype(np.float32)
    w[:, PR.REWARD] *= 0.01
    return w


def restate(b, w, feat, piece, allowed=None, scores=FR.scores_f32):
    """(slots, actions, scores, best [R, n]) by numpy from feat [n, R, S]."""
    n, R, S = feat.shape
    slots, acts = np.empty(n, np.int32), np.empty(n, np.uint8)
    sc, best = np.zeros(n, np.float32), np.zeros((R, n), np.int32)
    for e in range(n):
        we = w[e % len(w)]
        all_sc = scores(we, feat[e])
        ok = feat[e, PR.VALID] != 0
        if allowed is not None:
            ok &= allowed[e] != 0
        idx = np.flatnonzero(ok)
        s = int(idx[np.argmax(all_sc[idx])]) if len(idx) else -1
        slots[e], acts[e] = s, FR.action_for(b.width, piece[e], s)
        if s >= 0:
            sc[e], best[:, e] = all_sc[s], feat[e, :, s]
    return slots, acts, sc, best


def check_choice(c, want, what):
    slots, acts, sc, best = want
    assert np.array_equal(c.slots.cpu().numpy(), slots), (what, "slots", c.slots.cpu().numpy(), slots)
    assert np.array_equal(c.actions.cpu().numpy(), acts), (what, "actions")
    assert np.array_equal(c.scores.cpu().numpy().view(np.uint32), sc.view(np.uint32)), (what, "score bits")
    assert np.array_equal(c.feat.cpu().numpy(), best), (what, "best rows")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(4, 12), (10, 20), (13, 26), (32, 28)], ids=["4x12", "10x20", "13x26", "32x28"])
def test_policy_linear_bcts_against_the_restatement(W, H):
    """70 per-env weight rows, 3 rows and 1 row of mixed-sign weights on an
    aged batch: slots, actions, score bits and best rows equal the numpy chain
    over the kernel's own afterstates(features='bcts') rows (test 1 and 2 hold
    those to the reference); a fused chain gives other bits somewhere."""
    import torch
    n = 70
    b = aged(n, dict(width=W, height=H, **C4), 4400 + W, 31, 60)
    try:
        feat = b.afterstates(boards=False, features="bcts").feat.cpu().numpy()
        piece = b.get_state(("piece",))["piece"]
        fused_differs = 0
        for n_w in (70, 3, 1):
            w = mixed_weights(n_w, seed=n_w)
            c = b.policy_linear(torch.as_tensor(w, device=b.device), features="bcts")
            assert c.feat.shape == (NF, n)
            want = restate(b, w, feat, piece)
            check_choice(c, want, (W, H, n_w))
            fused = restate(b, w, feat, piece, scores=FR.scores_fused)
            fused_differs += int((fused[2].view(np.uint32) != want[2].view(np.uint32)).sum())
            assert torch.equal(c.wells, c.feat[FR.WELLS]) and torch.equal(c.holes, c.feat[PR.HOLES])
        assert fused_differs > 0  # (the rule can tell the two chains apart on this sample)
        # host weights by name, and a single output
        c = b.policy_linear(_engine().BCTS_WEIGHTS, features="bcts")
        wb = _engine().engine.weight_rows(_engine().BCTS_WEIGHTS, features="bcts")
        check_choice(c, restate(b, wb, feat, piece), "BCTS_WEIGHTS")
        only = torch.full((n,), -9, dtype=torch.int32, device=b.device)
        c2 = b.policy_linear(_engine().BCTS_WEIGHTS, out=(only, None, None, None), features="bcts")
        assert c2.slots is only and c2.feat is None and torch.equal(only, c.slots)
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(4, 12), (10, 20), (32, 28)], ids=["4x12", "10x20", "32x28"])
def test_policy_linear_ties_on_crafted_boards_against_the_reference(W, H):
    """On the crafted boards, with weights that tie many slots (all zero; LINES
    alone; ERODED and HOLE_ROWS), the choice is the lowest tied slot by the
    reference's rows; the blocked board gives slot -1, action 2, score 0, zero
    rows."""
    import torch
    n = 70
    b, names = crafted_batch(W, H, n)
    try:
        ref = crafted_ref(W, H)
        feat = np.stack([ref[name] for name in names])
        piece = b.get_state(("piece",))["piece"]
        rows = np.zeros((3, NF), np.float32)
        rows[1, PR.LINES] = 1.0
        rows[2, FR.ERODED], rows[2, FR.HOLE_ROWS] = 0.5, -2.0
        for w in (rows[:1], rows[1:2], rows):
            c = b.policy_linear(torch.as_tensor(w, device=b.device), features="bcts")
            check_choice(c, restate(b, w, feat, piece), (W, H, len(w)))
        e = names.index("blocked")
        assert int(c.slots[e]) == -1 and int(c.actions[e]) == 2 and float(c.scores[e]) == 0.0
        assert not c.feat[:, e].any()
    finally:
        b.close()


@pytest.mark.gpu
def test_base_set_through_policy_linear_set_is_policy_linear():
    """ST_FEATS_BASE through st_policy_linear_set -- without a mask (the old
    kernel) and with an all-ones mask (the new kernel's base instantiation) --
    equals policy_linear bit for bit."""
    import torch
    n = 70
    b = aged(n, dict(width=13, height=26, **C4), 4500, 41, 80)
    try:
        w = torch.as_tensor(mixed_weights(7)[:, :NB].copy(), device=b.device)
        old = b.policy_linear(w)
        ones = torch.ones((n, b.n_slots), dtype=torch.int32, device=b.device)
        for mask in (None, ones):
            sl = torch.full((n,), -9, dtype=torch.int32, device=b.device)
            ac = torch.full((n,), 9, dtype=torch.uint8, device=b.device)
            sc = torch.full((n,), -9.0, dtype=torch.float32, device=b.device)
            ft = torch.full((NB, n), -9, dtype=torch.int32, device=b.device)
            assert b._L.st_policy_linear_set(b._ctx, 0, _ptr(w), 7, _ptr(mask), _ptr(sl), _ptr(ac), _ptr(sc), _ptr(ft),
                                             b._stream()) == 0
            assert torch.equal(sl, old.slots) and torch.equal(ac, old.actions) and torch.equal(ft, old.feat)
            assert torch.equal(sc.view(torch.int32), old.scores.view(torch.int32))
        masked = b.policy_linear(w, allowed=ones)
        assert torch.equal(masked.slots, old.slots) and torch.equal(masked.feat, old.feat)
    finally:
        b.close()


# ------------------------------------------------------------------ 5. the mask
@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(10, 20), (32, 28)], ids=["10x20", "32x28"])
def test_mask(W, H):
    import torch
    n = 70
    b = aged(n, dict(width=W, height=H, **C4), 4600 + W, 51, 100)
    try:
        S, dev = b.n_slots, b.device
        a = b.afterstates(boards=False, features="bcts")
        feat = a.feat.cpu().numpy()
        piece = b.get_state(("piece",))["piece"]
        wn = mixed_weights(5, seed=9)
        w = torch.as_tensor(wn, device=dev)
        free = b.policy_linear(w, features="bcts")
        ones = torch.ones((n, S), dtype=torch.int32, device=dev)
        c = b.policy_linear(w, features="bcts", allowed=ones)
        for x, y in ((c.slots, free.slots), (c.actions, free.actions), (c.feat, free.feat),
                     (c.scores.view(torch.int32), free.scores.view(torch.int32))):
            assert torch.equal(x, y)
        # confined to the slots the live piece can reach
        r = b.reachable(first=False)
        steps = r.steps.cpu().numpy()
        c = b.policy_linear(w, features="bcts", allowed=r)
        check_choice(c, restate(b, wn, feat, piece, allowed=steps), "reachable")
        got = c.slots.cpu().numpy()
        assert (got >= 0).sum() > n // 2 and (steps[np.arange(n), got][got >= 0] > 0).all()
        assert torch.equal(b.policy_linear(w, features="bcts", allowed=r.steps).slots, c.slots)
        print("mask", (W, H), "reachable mask moved", int((got != free.slots.cpu().numpy()).sum()), "choices of", n)

        def nothing(c, what):
            assert (c.slots == -1).all() and (c.actions == 2).all() and (c.scores == 0).all(), what
            assert not c.feat.any(), what
        nothing(b.policy_linear(w, features="bcts", allowed=torch.zeros_like(ones)), "all-zero mask")
        invalid_only = (a.valid == 0).to(torch.int32).contiguous()
        assert invalid_only.any()
        nothing(b.policy_linear(w, features="bcts", allowed=invalid_only), "only invalid slots allowed")
        # negative and large mask words count as allowed; single envs can be masked out
        odd = torch.where(torch.arange(n, device=dev)[:, None] % 2 == 1, torch.full_like(ones, -5), torch.zeros_like(ones))
        c = b.policy_linear(w, features="bcts", allowed=odd)
        assert (c.slots[0::2] == -1).all() and torch.equal(c.slots[1::2], free.slots[1::2])
        if S > 128:  # the winner moved into the second and into the third slot pass
            for lo, hi in ((64, 128), (128, S)):
                m = torch.zeros_like(ones)
                m[:, lo:hi] = 1
                c = b.policy_linear(w, features="bcts", allowed=m)
                check_choice(c, restate(b, wn, feat, piece, allowed=m.cpu().numpy()), ("pass", lo))
                got = c.slots.cpu().numpy()
                assert ((got >= lo) & (got < hi)).all()
    finally:
        b.close()


# ------------------------------------------------------------------ 6. play
PLAY_ROWS = np.zeros((3, NF), np.float32)
PLAY_ROWS[0, [FR.LANDING2, FR.ERODED, FR.ROW_TRANS, FR.COL_TRANS, PR.HOLES, FR.WELLS, FR.HOLE_DEPTH, FR.HOLE_ROWS]] = \
    (-6.315, 6.60, -9.22, -19.77, -13.08, -10.49, -1.61, -24.04)
PLAY_ROWS[1, [FR.LANDING2, FR.WELLS, PR.LINES]] = (1.0, 0.5, -3.0)  # builds upward: its games end
PLAY_ROWS[2, [FR.HOLE_DEPTH, FR.COL_TRANS, PR.REWARD]] = (-1.0, -0.25, 0.125)
TINY = dict(n=8, kw=dict(width=6, height=8, **C4), seed0=3300, T=60)


def cpu_player():
    """The numpy / oracle placement player over the 18 rows on 6x8 under
    'same_step': per env and step the reference's slot features, the float32
    chain, the first maximum, then ref_place_step.  Env e plays row e % 3; env
    0 starts on placement_ref.tiny_blocked_board().  No engine call."""
    n, kw, T = TINY["n"], TINY["kw"], TINY["T"]
    ob = O.OracleBatch(n, [TINY["seed0"] + e for e in range(n)], **kw)
    ob.reset()
    ob.set_state(0, board=PR.tiny_blocked_board(), ay=PR.TINY_AY)
    h = PR.helper_oracle(kw)
    slots = np.empty((T, n), np.int32)
    out = dict(slots=slots, obs=np.empty((T, n, kw["width"]), np.uint32), reward=np.empty((T, n), np.int32),
               done=np.empty((T, n), np.uint8))
    for t in range(T):
        for e in range(n):
            env = ob.envs[e]
            feat = FR.slot_features_bcts(h, ob.board(e).astype(bool), env.shape_id, env.holes, env.piece_height)
            slots[t, e] = FR.choose(PLAY_ROWS[e % 3], feat)[0]
            out["obs"][t, e], out["reward"][t, e], out["done"][t, e], _ = PR.ref_place_step(ob, e, slots[t, e],
                                                                                           "same_step")
    out["returns"] = out["reward"].astype(np.int64).sum(axis=0)
    out["episodes"] = out["done"].astype(np.int32).sum(axis=0)
    out["final"] = ob.packed_state()
    out["ob"] = ob
    return out


def tiny_ref():
    return cached_ref("features_tiny_player", cpu_player)


def test_the_cpu_player_sees_deaths_clears_and_a_blocked_board():
    """Needs no GPU: the game the engine is held to has episode ends, line
    clears and a step without a valid slot."""
    ref = tiny_ref()
    assert ref["episodes"].sum() > 0 and ref["slots"][0, 0] == -1 and (ref["slots"][1:] >= 0).all()
    assert ref["reward"].max() > 0  # (C4 pays only for clears)
    assert len({tuple(ref["slots"][:, e]) for e in range(3)}) == 3  # the three weight rows play differently


def _tiny_batch():
    n, kw = TINY["n"], TINY["kw"]
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[TINY["seed0"] + e for e in range(n)], **kw)
    b.reset()
    st = b.get_state(("board", "piece"))
    st["board"][:, 0] = pack_cols(PR.tiny_blocked_board())
    st["piece"][0] |= np.uint32(PR.TINY_AY << 11)
    b.set_state(**st)
    return b


@pytest.mark.gpu
def test_engine_play_equals_the_cpu_player():
    import torch
    ref = tiny_ref()
    T = TINY["T"]
    b, hand = _tiny_batch(), _tiny_batch()
    try:
        w = torch.as_tensor(PLAY_ROWS, device=b.device)
        ret, eps = b.play_linear(w, T, obs="packed", placements=True, features="bcts")
        assert np.array_equal(ret.cpu().numpy(), ref["returns"]), (ret, ref["returns"])
        assert np.array_equal(eps.cpu().numpy(), ref["episodes"])
        check_step(ref, T - 1, b.obs, b.reward, b.done)
        check_engine_state(b, ref["final"])
        check_mt_state(b, ref["ob"])
        for t in range(T):
            c = hand.policy_linear(w, features="bcts")
            assert np.array_equal(c.slots.cpu().numpy(), ref["slots"][t]), ("slot", t)
            check_step(ref, t, *hand.step_placements(c.slots))
        check_engine_state(hand, ref["final"], "by hand")
    finally:
        b.close()
        hand.close()


@pytest.mark.gpu
@pytest.mark.parametrize("placements", [False, True], ids=["primitive", "placements"])
@pytest.mark.parametrize("autoreset", ["none", "same_step"])
def test_play_linear_bcts_equals_the_loop_by_hand(autoreset, placements):
    """k = 37 (it crosses the 32-row ring) in one call, as 20 + 17 chained,
    k = 1 and k = 0, against policy_linear(features='bcts') -> step /
    step_placements by hand: returns, episodes, last outputs, engine state."""
    import torch
    n, K = 70, 37
    kw = dict(width=6, height=9, **C4)
    seeds = [6900 + e for e in range(n)]
    G = _engine()
    one, two, twin = (G.TetrisBatch(n, autoreset=autoreset, seeds=seeds, **kw) for _ in range(3))
    try:
        for x in (one, two, twin):
            x.reset()
        w = torch.as_tensor(np.concatenate([PLAY_ROWS, mixed_weights(4)]), device=one.device)
        rsum, dsum = np.zeros(n, np.int64), np.zeros(n, np.int32)
        last = None

        def loop(k):
            nonlocal last
            for _ in range(k):
                c = twin.policy_linear(w, features="bcts")
                last = tuple(x.clone() for x in (twin.step_placements(c.slots) if placements else twin.step(c.actions)))
                rsum[:] += last[1].cpu().numpy()
                dsum[:] += last[2].cpu().numpy()

        def same(b, ret, eps, what):
            assert_same_state(b, twin, what)
            assert np.array_equal(ret.cpu().numpy(), rsum) and np.array_equal(eps.cpu().numpy(), dsum), what
            assert torch.equal(b.reward, last[1]) and torch.equal(b.done, last[2]) and torch.equal(b.obs, last[0]), what

        loop(K)
        ret, eps = one.play_linear(w, K, obs="packed", placements=placements, features="bcts")
        same(one, ret, eps, "k = 37")
        assert dsum.sum() > 0
        r2, e2 = two.play_linear(w, 20, placements=placements, features="bcts")
        r2b, e2b = two.play_linear(w, 17, returns=r2, episodes=e2, obs="packed", placements=placements, features="bcts")
        assert r2b is r2 and e2b is e2
        same(two, r2, e2, "k = 20 + 17")
        loop(1)
        one.play_linear(w, 1, returns=ret, episodes=eps, obs="packed", placements=placements, features="bcts")
        same(one, ret, eps, "k = 1")
        before = (ret.clone(), eps.clone(), one.reward.clone())
        one.play_linear(w, 0, returns=ret, episodes=eps, placements=placements, features="bcts")
        assert_same_state(one, twin, "k = 0")
        assert torch.equal(ret, before[0]) and torch.equal(eps, before[1]) and torch.equal(one.reward, before[2])
    finally:
        for x in (one, two, twin):
            x.close()


# ------------------------------------------------------------------ 7. no side effects, errors, checks
@pytest.mark.gpu
def test_the_calls_change_no_state():
    import torch
    b = aged(70, dict(width=11, height=12, **C4), 4700, 61, 50)
    try:
        before = engine_state(b)
        w = torch.as_tensor(mixed_weights(3), device=b.device)
        b.afterstates(features="bcts")
        b.afterstates(boards=False, features="bcts")
        r = b.reachable(first=False)
        b.policy_linear(w, features="bcts")
        b.policy_linear(w, features="bcts", allowed=r)
        b.policy_linear(w[:, :NB].contiguous(), allowed=r)
        b.play_linear(w, 0, features="bcts")
        assert b._L.st_feature_rows(1) == NF
        assert_same_state(before, b, "a read-only call changed the state")
    finally:
        b.close()


@pytest.mark.gpu
def test_abi_errors_on_a_live_context():
    import torch
    from gym_simpletetris_amd import _lib as C
    L = C.load()
    ctx = ctypes.c_void_p()
    n, S = 8, 64
    assert L.st_create(ctypes.byref(ctx), ctypes.byref(C.Config(10, 20, 0, 0, 0)), 0, n) == C.ST_OK
    try:
        w = torch.zeros((1, NF), dtype=torch.float32, device="cuda")
        ft = torch.full((n, NF, S), -7, dtype=torch.int32, device="cuda")
        sl = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        ret = torch.zeros(n, dtype=torch.int64, device="cuda")
        pw, pf, ps, pt = (_ptr(x) for x in (w, ft, sl, ret))

        def all_estate():
            for name, rc in (("st_afterstates_set", L.st_afterstates_set(ctx, 1, pf, None, None)),
                             ("st_policy_linear_set", L.st_policy_linear_set(ctx, 1, pw, 1, None, ps, None, None, None,
                                                                             None)),
                             ("st_play_linear_set", L.st_play_linear_set(ctx, 1, pw, 1, 1, 1, pt, None, None, None, None,
                                                                         None))):
                assert rc == C.ST_ESTATE, name
        all_estate()
        seeds = np.arange(n, dtype=np.uint64)
        assert L.st_seed(ctx, ctypes.c_void_p(seeds.ctypes.data), None) == C.ST_OK
        all_estate()
        assert L.st_reset(ctx, None, None) == C.ST_OK
        for bad_set in (-1, 2):
            assert L.st_afterstates_set(ctx, bad_set, pf, None, None) == C.ST_EINVAL
            assert b"st_afterstates_set" in L.st_last_error()
            assert L.st_policy_linear_set(ctx, bad_set, pw, 1, None, ps, None, None, None, None) == C.ST_EINVAL
            assert b"st_policy_linear_set" in L.st_last_error()
            assert L.st_play_linear_set(ctx, bad_set, pw, 1, 1, 0, pt, None, None, None, None, None) == C.ST_EINVAL
            assert b"st_play_linear_set" in L.st_last_error()
        assert L.st_afterstates_set(ctx, 1, None, None, None) == C.ST_EINVAL
        assert L.st_policy_linear_set(ctx, 1, None, 1, None, ps, None, None, None, None) == C.ST_EINVAL
        assert L.st_policy_linear_set(ctx, 1, pw, 0, None, ps, None, None, None, None) == C.ST_EINVAL
        assert L.st_policy_linear_set(ctx, 1, pw, 1, None, None, None, None, None, None) == C.ST_EINVAL
        assert L.st_play_linear_set(ctx, 1, None, 1, 1, 0, pt, None, None, None, None, None) == C.ST_EINVAL
        assert L.st_play_linear_set(ctx, 1, pw, -2, 1, 0, pt, None, None, None, None, None) == C.ST_EINVAL
        torch.cuda.synchronize()
        assert (ft == -7).all() and (sl == -7).all() and (ret == 0).all()
        assert L.st_play_linear_set(ctx, 1, pw, 1, -3, 1, pt, None, None, None, None, None) == C.ST_OK  # k <= 0
        assert L.st_afterstates_set(ctx, 1, pf, None, None) == C.ST_OK
        assert L.st_policy_linear_set(ctx, 1, pw, 1, None, ps, None, None, None, None) == C.ST_OK
        assert L.st_play_linear_set(ctx, 1, pw, 1, 2, 1, None, None, None, None, None, None) == C.ST_OK
        torch.cuda.synchronize()
        assert (ret == 0).all() and (sl >= 0).all() and (ft[:, 0] >= 0).all()
    finally:
        L.st_destroy(ctx)


@pytest.mark.gpu
def test_out_and_weight_tensors_are_checked():
    import torch
    n = 8
    b = _engine().TetrisBatch(n, seeds=list(range(n)))
    try:
        b.reset()
        dev, S = b.device, b.n_slots
        before = engine_state(b)
        w18 = torch.zeros((2, NF), dtype=torch.float32, device=dev)
        for bad in (torch.zeros((2, NB), dtype=torch.float32, device=dev), torch.zeros((2, NF), dtype=torch.float64, device=dev),
                    torch.zeros((2, NF), dtype=torch.float32), torch.zeros((0, NF), dtype=torch.float32, device=dev)):
            with pytest.raises((ValueError, TypeError)):
                b.policy_linear(bad, features="bcts")
            with pytest.raises((ValueError, TypeError)):
                b.play_linear(bad, 1, features="bcts")
        with pytest.raises((ValueError, TypeError)):  # 18 weights for the base set
            b.policy_linear(w18)
        for bad in ((torch.zeros((n, NB, S), dtype=torch.int32, device=dev), None),
                    (torch.zeros((n, NF, S), dtype=torch.int64, device=dev), None),
                    (torch.zeros((n, NF, S), dtype=torch.int32), None)):
            with pytest.raises((ValueError, TypeError)):
                b.afterstates(boards=False, out=bad, features="bcts")
        with pytest.raises((ValueError, TypeError)):  # an 18-row tensor for the base set
            b.afterstates(boards=False, out=(torch.zeros((n, NF, S), dtype=torch.int32, device=dev), None))
        with pytest.raises((ValueError, TypeError)):
            b.policy_linear(w18, out=(None, None, None, torch.zeros((NB, n), dtype=torch.int32, device=dev)),
                            features="bcts")
        for bad in (torch.ones((n, S), dtype=torch.int64, device=dev), torch.ones((n, S - 1), dtype=torch.int32, device=dev),
                    torch.ones((n, S), dtype=torch.int32), torch.ones((n, 2 * S), dtype=torch.int32, device=dev)[:, ::2]):
            with pytest.raises((ValueError, TypeError)):
                b.policy_linear(w18, features="bcts", allowed=bad)
        with pytest.raises(ValueError):
            b.policy_linear(w18, features="dellacherie")
        assert_same_state(before, b, "an error changed the state")
        good = torch.full((NF, n), -9, dtype=torch.int32, device=dev)
        c = b.policy_linear(w18, out=(None, None, None, good), features="bcts")
        assert c.feat is good and c.slots is None and (good[0] == 1).all()
    finally:
        b.close()


@pytest.mark.gpu
def test_vec_env_pass_through():
    import torch
    G = _engine()
    env = G.TetrisVecEnv(16, seed=3, obs_format="packed")
    twin = G.TetrisVecEnv(16, seed=3, obs_format="packed")
    try:
        env.reset()
        twin.reset()
        a = env.afterstates(boards=False, features="bcts")
        assert a.feat.shape == (16, NF, 64) and torch.equal(a.feat, twin.engine.afterstates(False, features="bcts").feat)
        r = env.engine.reachable(first=False)
        c = env.policy_linear(G.DELLACHERIE_WEIGHTS, features="bcts", allowed=r)
        c2 = twin.engine.policy_linear(G.DELLACHERIE_WEIGHTS, features="bcts", allowed=r.steps)
        assert torch.equal(c.slots, c2.slots) and c.feat.shape == (NF, 16)
        ret, eps = env.play_linear(G.BCTS_WEIGHTS, 10, placements=True, features="bcts")
        r2, e2 = twin.engine.play_linear(G.BCTS_WEIGHTS, 10, placements=True, features="bcts")
        assert torch.equal(ret, r2) and torch.equal(eps, e2)
        assert_same_state(env, twin, "play_linear(features='bcts')")
    finally:
        env.close()
        twin.close()
