"""st_policy_linear / st_play_linear (TetrisBatch.policy_linear, .play_linear).

The new kernel's outputs are never their own expectation.  The expectations:

- choose(): a numpy restatement of the header's rule -- the float32 chain
  acc = acc + w[r] * feat[r] in enum order with every product and sum rounded
  to float32 on its own, the first maximum over the valid slots, slot -1 /
  score 0 / zero features without one -- evaluated on feature rows that are
  either st_afterstates's (parent code, checked against the oracle by
  test_gpu_afterstates.py) or slot_features()'s below;
- slot_features(): the rows of one env from a one-env OracleBatch (set_state +
  step_one(0, 2), the hard drop that locks the piece in the slot) and a
  few-line restatement of is_occupied, as test_gpu_afterstates.py documents;
- st_policy_greedy, an independent kernel pinned by tests/golden/greedy.npz;
- the oracle's rollout of recorded actions.
"""
import ctypes

import numpy as np
import pytest

from harness import C4, assert_same_state, cached_ref, check_step, engine as _engine, engine_state, pack_cols
from oracle import oracle as O

NF = 11
NAMES = ("valid", "y", "lines", "holes", "height", "rows", "above", "dead", "reward", "agg_height", "bumpiness")
VALID, Y, LINES, HOLES, HEIGHT, ROWS, ABOVE, DEAD, REWARD, AGG, BUMP = range(NF)
GREEDY = np.zeros(NF, np.float32)
GREEDY[[LINES, HOLES, HEIGHT, ABOVE]] = 80, -12, -3, -2000


# ------------------------------------------------------------------ the rule (numpy, no GPU)
def scores_f32(w, feat):
    """The header's chain on rows feat [NF, ...] with weights w [NF] (or
    [NF, ...]): np.float32 multiply, then np.float32 add, row by row."""
    w = np.asarray(w, np.float32)
    acc = np.zeros(feat.shape[1:], np.float32)
    for r in range(NF):
        prod = w[r] * feat[r].astype(np.float32)
        assert prod.dtype == np.float32
        acc = acc + prod
        assert acc.dtype == np.float32
    return acc


def scores_fused(w, feat):
    """What a contracted multiply-add would give: every step rounded once,
    round32(float64(acc) + float64(w) * float64(f))."""
    w = np.asarray(w, np.float32)
    acc = np.zeros(feat.shape[1:], np.float32)
    for r in range(NF):
        acc = (acc.astype(np.float64) + w[r].astype(np.float64) * feat[r].astype(np.float64)).astype(np.float32)
    return acc


def choose(w, feat, score_fn=scores_f32):
    """(slot, score, feature column) of one env: feat int [NF, S], w [NF]."""
    sc = score_fn(w, feat)
    idx = np.flatnonzero(feat[VALID] != 0)
    if len(idx) == 0:
        return -1, np.float32(0.0), np.zeros(NF, np.int32)
    s = int(idx[np.argmax(sc[idx])])  # (the first maximum)
    return s, sc[s], feat[:, s].astype(np.int32)


def placement_action(W, slot, rot, ax):
    """st_placement_actions's rule."""
    if slot < 0:
        return 2
    trot, tx = slot // (W + 6), slot % (W + 6) - 3
    return 4 if rot != trot else (1 if ax < tx else (0 if ax > tx else 2))


def expect_choices(W, feat, piece, wrows, score_fn=scores_f32):
    """choose() and placement_action() for every env: feat [n, NF, S] (slot
    innermost, as afterstates gives it), piece words [n], env e on weight row
    e % len(wrows) -> slots, actions, scores, feat [NF, n]."""
    n = feat.shape[0]
    sl, ac = np.empty(n, np.int32), np.empty(n, np.uint8)
    sc, bf = np.empty(n, np.float32), np.empty((NF, n), np.int32)
    for e in range(n):
        sl[e], sc[e], bf[:, e] = choose(wrows[e % len(wrows)], feat[e], score_fn)
        ac[e] = placement_action(W, sl[e], int(piece[e] >> 3) & 3, int(piece[e] >> 5) & 63)
    return sl, ac, sc, bf


def check_choice(c, want, what=""):
    """A LinearChoice against expect_choices's tuple, bit for bit."""
    sl, ac, sc, bf = want
    assert np.array_equal(c.slots.cpu().numpy(), sl), (what, "slots", np.nonzero(c.slots.cpu().numpy() != sl)[0])
    assert np.array_equal(c.actions.cpu().numpy(), ac), (what, "actions")
    got = c.scores.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), sc.view(np.uint32)), (what, "scores", got, sc)
    assert np.array_equal(c.feat.cpu().numpy(), bf), (what, "feat")
    for r, name in enumerate(NAMES):
        assert np.array_equal(getattr(c, name).cpu().numpy(), bf[r]), (what, name)


def mixed_weights(seed, n):
    """[n, NF] float32: uniform in +-1 times 10^(-2..2), scales mixed per entry."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (n, NF)) * 10.0 ** rng.integers(-2, 3, (n, NF))).astype(np.float32)


WSEED = 20240


def test_the_rule_can_tell_a_fused_multiply_add():
    """Needs no GPU: on synthetic integer features of the sizes the engine
    produces, the test weights' plain and fused chains differ in the chosen
    score of most envs -- so a contracted kernel cannot pass test 2."""
    rng = np.random.default_rng(1)
    n, S = 70, 64
    feat = rng.integers(0, 40, (n, NF, S)).astype(np.int32)
    feat[:, VALID] = 1
    w = mixed_weights(WSEED, n)
    piece = np.zeros(n, np.uint32)
    plain = expect_choices(10, feat, piece, w)
    fused = expect_choices(10, feat, piece, w, scores_fused)
    differ = plain[2].view(np.uint32) != fused[2].view(np.uint32)
    assert differ.sum() >= n // 4, differ.sum()
    # and the chain is sequential: a pairwise or reversed sum is another number
    assert scores_f32(w[0], feat[0]).dtype == np.float32


# ------------------------------------------------------------------ oracle features (no GPU)
def _occupied(cells, x0, y0, board):
    """is_occupied (tetris_env.py:29-36) on a bool board [W, H]."""
    W, H = board.shape
    for i, j in cells:
        x, y = x0 + i, y0 + j
        if y < 0:
            continue
        if x < 0 or x >= W or y >= H or board[x, y]:
            return True
    return False


def helper_oracle(kw):
    kw = dict(kw, lock_delay=0)
    kw.pop("step_reset", None)
    ob = O.OracleBatch(1, [1], **kw)
    ob.reset()
    return ob


def slot_features(h, board, sid, holes, piece_height):
    """feat int32 [NF, S] of one env from the one-env oracle h: bool board
    [W, H], piece id and the env's holes / piece_height counters."""
    W, H = board.shape
    per, S = W + 6, 4 * (W + 6)
    board_u8 = board.astype(np.uint8)
    feat = np.zeros((NF, S), np.int32)
    for rot in range(4):
        cells = O.rotate_cells(O.BASE_SHAPES[sid], rot)
        for x in range(-3, W + 3):
            if _occupied(cells, x, 0, board):
                continue
            y = 0
            while not _occupied(cells, x, y + 1, board):
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
            if not done:  # (a death step erases the piece again, :303)
                assert np.array_equal(h.board(0).astype(bool), nb), ("numpy placement vs oracle", sid, rot, x)
            hcol = np.where(nb.any(axis=1), H - nb.argmax(axis=1), 0)
            row_any = nb.any(axis=0)
            feat[:, rot * per + x + 3] = (
                1, y, h.envs[0].lines_cleared - lines0, h.envs[0].holes,
                H - int(row_any.argmax()) if row_any.any() else 0, int(row_any.sum()),
                int(any(y + j < 0 for _, j in cells)), int(done), rew, int(hcol.sum()), int(np.abs(np.diff(hcol)).sum()))
    return feat


# ------------------------------------------------------------------ 1. equals the greedy kernel
EVOLVE_10x20 = (128, dict(width=10, height=20, **C4), 4200, 11, (40, 90, 140, 199))


def mixed_actions(b, t, aseed):
    """Step t's actions: the first half of the envs play policy_greedy
    (explore 30 per mille), the second half uniform gen_actions."""
    import torch
    g = b.policy_greedy(t, seed=aseed, explore=30).clone()
    u = b.gen_actions(t, aseed)
    return torch.where(torch.arange(b.n, device=b.device) < b.n // 2, g, u)


def evolved(n, kw, seed0, aseed, steps):
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[seed0 + e for e in range(n)], **kw)
    b.reset()
    for t in range(steps):
        b.step(mixed_actions(b, t, aseed), obs="none")
    return b


@pytest.mark.gpu
def test_greedy_weights_equal_the_greedy_kernel():
    import torch
    from gym_simpletetris_amd import GREEDY_WEIGHTS
    n, kw, seed0, aseed, cps = EVOLVE_10x20
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[seed0 + e for e in range(n)], **kw)
    try:
        b.reset()
        checked, seen = 0, set()
        for t in range(200):
            if t in cps:
                c = b.policy_linear(GREEDY_WEIGHTS)
                want = b.policy_greedy(t, seed=0, explore=0).cpu().numpy()
                assert np.array_equal(c.actions.cpu().numpy(), want), (t, np.nonzero(c.actions.cpu().numpy() != want)[0])
                seen |= set(want.tolist())
                a = b.afterstates(boards=False)
                isc = (80 * a.lines - 12 * a.holes - 3 * a.height - 2000 * a.above).cpu().numpy().astype(np.int64)
                valid = a.valid.cpu().numpy() != 0
                assert valid.any(axis=1).all()
                first = np.where(valid, isc, np.iinfo(np.int64).min).argmax(axis=1)  # (the first maximum)
                assert np.array_equal(c.slots.cpu().numpy(), first), t
                assert torch.equal(c.scores, torch.as_tensor(isc[np.arange(n), first].astype(np.float32), device=b.device))
                checked += 1
            b.step(mixed_actions(b, t, aseed), obs="none")
        assert checked == 4 and len(seen) >= 3, (checked, seen)
    finally:
        b.close()


# ------------------------------------------------------------------ 2. exact float32 semantics
SHAPES = {
    "4x12": dict(width=4, height=12, penalise_holes=True, reward_step=True),        # S = 40: lanes past the last slot
    "10x20": dict(width=10, height=20, **C4),                                       # S = 64: exactly one pass
    "13x26": dict(width=13, height=26, penalise_height_increase=True, advanced_clears=True),  # S = 76: two passes
    "32x28": dict(width=32, height=28, **C4),                                       # S = 152: three passes
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact_float32_semantics(name):
    """Per-env weights of mixed scales on 70 envs: scores, slots, actions and
    feature rows equal the sequential float32 restatement on afterstates rows
    of the same state, bit for bit; the fused variant of the restatement
    differs on this very sample, so a contracted kernel fails here.  Then
    three rows: env e uses row e % 3.  Weights as a device tensor and as a
    host array are the same call."""
    import torch
    n, kw = 70, SHAPES[name]
    W = kw["width"]
    b = evolved(n, kw, 7300, 17, 60)
    try:
        st = b.get_state(("piece",))
        feat = b.afterstates(boards=False).feat.cpu().numpy()
        assert feat.shape == (n, NF, 4 * (W + 6))
        w = mixed_weights(WSEED, n)
        want = expect_choices(W, feat, st["piece"], w)
        c = b.policy_linear(torch.as_tensor(w, device=b.device))
        check_choice(c, want, (name, "n_w = n"))
        fused = expect_choices(W, feat, st["piece"], w, scores_fused)
        assert (fused[2].view(np.uint32) != want[2].view(np.uint32)).any(), "the sample cannot tell an FMA"
        check_choice(b.policy_linear(w), want, (name, "host weights"))
        w3 = w[:3]
        want3 = expect_choices(W, feat, st["piece"], w3)
        check_choice(b.policy_linear(torch.as_tensor(w3, device=b.device)), want3, (name, "n_w = 3"))
        assert not np.array_equal(want3[2], want[2])  # (the row matters)
        one = expect_choices(W, feat, st["piece"], w[:1])
        check_choice(b.policy_linear(torch.as_tensor(w[0], device=b.device)), one, (name, "n_w = 1"))
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_one_env(name):
    """n = 1: one live wave in a workgroup whose other waves leave at once,
    and weight row 0 whatever n_w is.  n_w = 1 and n_w = 3 (more rows than
    envs), at four states of one game, bit for bit against the restatement on
    afterstates rows of the same state, into guarded buffers."""
    import torch
    kw = SHAPES[name]
    W, n, pad = kw["width"], 1, 6
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[9100], **kw)
    try:
        b.reset()
        w3 = mixed_weights(WSEED + 1, 3)
        for t in range(40):
            if t % 10 == 9:
                st = b.get_state(("piece",))
                feat = b.afterstates(boards=False).feat.cpu().numpy()
                for w in (w3[:1], w3):
                    bufs = [torch.full((n + pad,), 249 if dt == torch.uint8 else -7, dtype=dt, device=b.device)
                            for dt in (torch.int32, torch.uint8, torch.float32)]
                    fbuf = torch.full((NF * n + pad,), -7, dtype=torch.int32, device=b.device)
                    out = (bufs[0][:n], bufs[1][:n], bufs[2][:n], fbuf[:NF * n].view(NF, n))
                    c = b.policy_linear(torch.as_tensor(w, device=b.device), out=out)
                    check_choice(c, expect_choices(W, feat, st["piece"], w[:1]), (name, t, len(w)))
                    for buf in bufs:
                        assert (buf[n:] == (249 if buf.dtype == torch.uint8 else -7)).all(), buf.dtype
                    assert (fbuf[NF * n:] == -7).all()
            b.step(mixed_actions(b, t, 23), obs="none")
    finally:
        b.close()


@pytest.mark.gpu
def test_one_env_play_linear():
    """play_linear on one env (n_w = 3 > n) equals the loop by hand."""
    import torch
    kw = SHAPES["10x20"]
    G = _engine()
    b = G.TetrisBatch(1, autoreset="same_step", seeds=[9100], **kw)
    twin = G.TetrisBatch(1, autoreset="same_step", seeds=[9100], **kw)
    try:
        b.reset()
        twin.reset()
        wd = torch.as_tensor(THREE_ROWS, device=b.device)
        rsum = 0
        for _ in range(40):
            _, r, _ = twin.step(twin.policy_linear(wd).actions, obs="none")
            rsum += int(r[0])
        ret, _ = b.play_linear(wd, 40)
        assert int(ret[0]) == rsum
        assert_same_state(b, twin, "n = 1 play_linear")
    finally:
        b.close()
        twin.close()


# ------------------------------------------------------------------ 3. ties and empties
def _set_boards(b, boards, ids):
    """Boards u8 [n][W, H] and piece ids into a reset batch (set_state)."""
    st = b.get_state(("board", "piece", "stats"))
    st["board"][:] = np.stack([pack_cols(x) for x in boards], axis=1)
    st["piece"][:] = (st["piece"] & ~np.uint32(7)) | np.asarray(ids, np.uint32)
    b.set_state(**st)


def basic_cases(W, H):
    """(boards, piece ids, weight rows): the empty board under all-zero
    weights, the empty board under the greedy weights, row 0 full."""
    blocked = np.zeros((W, H), np.uint8)
    blocked[:, 0] = 1
    return [np.zeros((W, H), np.uint8), np.zeros((W, H), np.uint8), blocked], [0, 5, 1], \
        np.stack([np.zeros(NF, np.float32), GREEDY, GREEDY])


def pass_cases(W=32, H=28):
    """Three ragged boards whose winner lies in pass 1, 2 and 3 (slot < 64,
    64..127, >= 128) under weights on y and agg_height."""
    def ragged(seed, k):  # the k-th board of column heights 0..8 drawn from `seed`
        rng = np.random.default_rng(seed)
        for _ in range(k + 1):
            hts = rng.integers(0, 9, W)
        b = np.zeros((W, H), np.uint8)
        for x in range(W):
            b[x, H - hts[x]:] = 1
        return b
    # (picked by a search over seeds, pieces and weights with slot_features)
    boards, ids = [ragged(5, 0), ragged(5, 0), ragged(6, 1)], [0, 0, 2]
    w = np.zeros((3, NF), np.float32)
    w[:, Y], w[:, AGG] = (3.0, -1.0, -1.0), (-0.25, 0.5, 0.5)
    return boards, ids, w


def test_crafted_cases_reach_what_they_are_for():
    """Needs no GPU: by the oracle's features the basic cases tie (the lowest
    valid slot wins, under zero weights and under the greedy weights) or have
    no valid slot, and the ragged boards' winners lie in passes 1, 2 and 3."""
    for W, H in ((10, 20), (32, 28)):
        kw = dict(width=W, height=H, **C4)
        h = helper_oracle(kw)
        boards, ids, w = basic_cases(W, H)
        feats = [slot_features(h, bd.astype(bool), sid, 0, 0) for bd, sid in zip(boards, ids)]
        s0, sc0, _ = choose(w[0], feats[0])
        assert s0 == int(np.flatnonzero(feats[0][VALID])[0]) and sc0 == 0
        s1, _, _ = choose(w[1], feats[1])
        sc = scores_f32(w[1], feats[1])
        ties = np.flatnonzero((feats[1][VALID] != 0) & (sc == sc[s1]))
        assert len(ties) >= 4 and s1 == ties[0], ties
        assert choose(w[2], feats[2])[0] == -1 and not feats[2].any()
    boards, ids, w = pass_cases()
    h = helper_oracle(dict(width=32, height=28, **C4))
    got = [choose(w[e], slot_features(h, boards[e].astype(bool), ids[e], 0, 0))[0] for e in range(3)]
    assert 0 <= got[0] < 64 <= got[1] < 128 <= got[2] < 152, got


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,which", [(10, 20, "basic"), (32, 28, "basic"), (32, 28, "passes")],
                         ids=["10x20_basic", "32x28_basic", "32x28_passes"])
def test_ties_and_empties(W, H, which):
    """n = 3, one case per env and one weight row per env, into views of
    larger -7-filled buffers: nothing is written past n.  The expectation is
    the oracle's features (slot_features), not the engine's."""
    import torch
    kw = dict(width=W, height=H, **C4)
    boards, ids, w = basic_cases(W, H) if which == "basic" else pass_cases(W, H)
    n = 3
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[77 + e for e in range(n)], **kw)
    try:
        b.reset()
        _set_boards(b, boards, ids)
        st = b.get_state(("piece", "stats"))
        h = helper_oracle(kw)
        feat = np.stack([slot_features(h, boards[e].astype(bool), ids[e], int(st["stats"][3, e]), int(st["stats"][4, e]))
                         for e in range(n)])
        want = expect_choices(W, feat, st["piece"], w)
        pad = 5
        bufs = [torch.full((n + pad,), 249 if dt == torch.uint8 else -7, dtype=dt, device=b.device)
                for dt in (torch.int32, torch.uint8, torch.float32)]
        fbuf = torch.full((NF * n + pad,), -7, dtype=torch.int32, device=b.device)
        out = (bufs[0][:n], bufs[1][:n], bufs[2][:n], fbuf[:NF * n].view(NF, n))
        c = b.policy_linear(torch.as_tensor(w, device=b.device), out=out)
        assert c.slots is out[0] and c.actions is out[1] and c.scores is out[2] and c.feat is out[3]
        check_choice(c, want, (W, H, which))
        for t in bufs:
            assert (t[n:] == (249 if t.dtype == torch.uint8 else -7)).all(), t.dtype
        assert (fbuf[NF * n:] == -7).all()
        sl = c.slots.cpu().numpy()
        if which == "basic":
            assert sl[2] == -1 and int(c.actions[2]) == 2 and float(c.scores[2]) == 0.0
            assert not c.feat[:, 2].any()
            assert sl[0] == int(np.flatnonzero(feat[0][VALID])[0]) and float(c.scores[0]) == 0.0
        else:
            assert 0 <= sl[0] < 64 <= sl[1] < 128 <= sl[2] < 152, sl
    finally:
        b.close()


# ------------------------------------------------------------------ 4. no side effects
@pytest.mark.gpu
def test_no_side_effects():
    import torch
    n, kw, seed0, aseed, _ = EVOLVE_10x20
    G = _engine()
    b = evolved(n, kw, seed0, aseed, 60)
    twin = evolved(n, kw, seed0, aseed, 60)
    try:
        w = torch.as_tensor(mixed_weights(3, 5), device=b.device)
        before = engine_state(b)
        b.policy_linear(w)
        b.policy_linear(G.GREEDY_WEIGHTS)
        torch.cuda.synchronize()
        assert_same_state(before, b, "policy_linear changed the state")
        assert_same_state(before, twin, "twin")
        # steps after it: bit-exact against the twin that never called it
        for t in range(60, 80):
            acts = mixed_actions(twin, t, aseed).clone()
            b.policy_linear(w)
            got = [x.clone() for x in b.step(acts)]
            want = twin.step(acts)
            for g, x, k in zip(got, want, ("obs", "reward", "done")):
                assert torch.equal(g, x), (k, t)
        assert_same_state(b, twin, "after 20 more steps")
    finally:
        b.close()
        twin.close()


# ------------------------------------------------------------------ 5. an independent player
TINY = dict(n=8, kw=dict(width=6, height=8, **C4), seed0=3100, T=100)
AGG_UP = np.zeros(NF, np.float32)
AGG_UP[AGG] = 1.0  # rewards height: its games end
THREE_ROWS = np.stack([GREEDY, np.zeros(NF, np.float32), AGG_UP])


def cpu_player():
    """The numpy / oracle player on the tiny shape: per env and step the
    oracle's slot features, the float32 score, the argmax and the placement
    rule; the action is stepped on the n-env oracle.  No engine call."""
    n, kw, T = TINY["n"], TINY["kw"], TINY["T"]
    W = kw["width"]
    ob = O.OracleBatch(n, [TINY["seed0"] + e for e in range(n)], **kw)
    ob.reset()
    h = helper_oracle(kw)
    memo = {}  # (a board and piece stay for the several steps that steer the piece)
    out = dict(acts=np.empty((T, n), np.uint8), obs=np.empty((T, n, W), np.uint32), reward=np.empty((T, n), np.int32),
               done=np.empty((T, n), np.uint8), lines=0)
    for t in range(T):
        for e in range(n):
            env = ob.envs[e]
            board = ob.board(e).astype(bool)
            key = (board.tobytes(), env.shape_id, env.holes, env.piece_height)
            if key not in memo:
                memo[key] = slot_features(h, board, env.shape_id, env.holes, env.piece_height)
            slot, _, _ = choose(THREE_ROWS[e % 3], memo[key])
            out["acts"][t, e] = placement_action(W, slot, env.rot, env.ax)
        r = ob.rollout(out["acts"][t:t + 1])
        for k in ("obs", "reward", "done"):
            out[k][t] = r[k][0]
        out["lines"] = max(out["lines"], int(r["stats"][0, :, 2].max()))
    return out


def _tiny_ref():
    return cached_ref("policy_linear_tiny_player", cpu_player)


def test_cpu_player_sample_holds_an_episode_end_and_a_line():
    """Needs no GPU: the seeds were picked so that it does."""
    ref = _tiny_ref()
    assert ref["done"].sum() >= 1 and ref["lines"] >= 1, (ref["done"].sum(), ref["lines"])
    assert len(set(ref["acts"].ravel().tolist())) >= 3


@pytest.mark.gpu
def test_engine_loop_equals_the_cpu_player():
    import torch
    ref = _tiny_ref()
    n, kw, T = TINY["n"], TINY["kw"], TINY["T"]
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[TINY["seed0"] + e for e in range(n)], **kw)
    try:
        b.reset()
        w = torch.as_tensor(THREE_ROWS, device=b.device)
        for t in range(T):
            c = b.policy_linear(w)
            assert np.array_equal(c.actions.cpu().numpy(), ref["acts"][t]), ("action", t)
            check_step(ref, t, *b.step(c.actions))
        assert ref["done"].sum() >= 1 and ref["lines"] >= 1
    finally:
        b.close()


# ------------------------------------------------------------------ 6. play_linear
@pytest.mark.gpu
def test_play_linear_equals_the_python_loop():
    import torch
    n, K, K2 = 70, 120, 30
    kw = dict(width=10, height=20, **C4)
    seeds = [8100 + e for e in range(n)]
    G = _engine()
    b = G.TetrisBatch(n, autoreset="same_step", seeds=seeds, **kw)
    twin = G.TetrisBatch(n, autoreset="same_step", seeds=seeds, **kw)
    try:
        b.reset()
        twin.reset()
        w = torch.as_tensor(THREE_ROWS, device=b.device)
        acts, outs = [], []

        def loop(k):
            for _ in range(k):
                a = twin.policy_linear(w).actions
                acts.append(a.cpu().numpy())
                outs.append(tuple(x.clone() for x in twin.step(a)))

        def sums():
            return (sum(o[1].cpu().numpy().astype(np.int64) for o in outs),
                    sum(o[2].cpu().numpy().astype(np.int32) for o in outs))

        def same_last(obs="packed"):
            assert torch.equal(b.reward, outs[-1][1]) and torch.equal(b.done, outs[-1][2])
            if obs == "packed":
                assert torch.equal(b.obs, outs[-1][0])

        loop(K)
        ret, eps = b.play_linear(w, K, obs="packed")
        assert ret.dtype == torch.int64 and eps.dtype == torch.int32
        assert_same_state(b, twin, "after k = 120")
        assert np.array_equal(ret.cpu().numpy(), sums()[0]) and np.array_equal(eps.cpu().numpy(), sums()[1])
        same_last()
        assert int(eps.sum()) > 0
        # the twin's recorded actions, replayed by the oracle, give every twin output
        ob = O.OracleBatch(n, seeds, **kw)
        ob.reset()
        ref = ob.rollout(np.stack(acts))
        for t in range(K):
            check_step(ref, t, *outs[t])
        # a second call continues the accumulators
        loop(K2)
        r2, e2 = b.play_linear(w, K2, returns=ret, episodes=eps)
        assert r2 is ret and e2 is eps
        assert_same_state(b, twin, "after k = 30 more")
        assert np.array_equal(ret.cpu().numpy(), sums()[0]) and np.array_equal(eps.cpu().numpy(), sums()[1])
        same_last(obs="none")
        # k = 0 changes nothing
        before = (ret.clone(), eps.clone(), b.reward.clone())
        b.play_linear(w, 0, returns=ret, episodes=eps)
        assert_same_state(b, twin, "k = 0")
        assert torch.equal(ret, before[0]) and torch.equal(eps, before[1]) and torch.equal(b.reward, before[2])
        # an armed gate (it saw an action outside 0..6) is still armed afterwards:
        # play_linear's steps run, the next st_step is the one that is skipped
        L, s = b._L, b._stream()
        bad = torch.full((n,), 9, dtype=torch.uint8, device=b.device)
        assert L.st_gate_actions(b._ctx, ctypes.c_void_p(bad.data_ptr()), s) == 0
        loop(5)
        b.play_linear(w, 5, returns=ret, episodes=eps)
        assert_same_state(b, twin, "play_linear behind an armed gate")
        assert np.array_equal(ret.cpu().numpy(), sums()[0])
        rew = torch.full((n,), -7, dtype=torch.int32, device=b.device)
        assert L.st_step(b._ctx, ctypes.c_void_p(bad.data_ptr()), None, ctypes.c_void_p(rew.data_ptr()),
                         ctypes.c_void_p(b.done.data_ptr()), s) == 0
        assert L.st_gate_wait(b._ctx) == 1
        torch.cuda.synchronize()
        assert (rew == -7).all()
        assert_same_state(b, twin, "the gated step was skipped")
        # only one accumulator, no last-step outputs: raw call
        only = torch.zeros(n, dtype=torch.int32, device=b.device)
        loop(3)
        assert L.st_play_linear(b._ctx, ctypes.c_void_p(w.data_ptr()), 3, 3, None, ctypes.c_void_p(only.data_ptr()),
                                None, None, None, s) == 0
        assert_same_state(b, twin, "episodes alone")
        assert np.array_equal(only.cpu().numpy(), sum(o[2].cpu().numpy().astype(np.int32) for o in outs[-3:]))
    finally:
        b.close()
        twin.close()


@pytest.mark.gpu
def test_play_linear_without_autoreset_equals_the_loop_by_hand():
    """autoreset='none': dead envs keep being stepped, as the loop does."""
    import torch
    n, K = 20, 60
    kw = dict(width=6, height=8, **C4)
    seeds = [3100 + e for e in range(n)]
    G = _engine()
    b = G.TetrisBatch(n, autoreset="none", seeds=seeds, **kw)
    twin = G.TetrisBatch(n, autoreset="none", seeds=seeds, **kw)
    try:
        b.reset()
        twin.reset()
        w = torch.as_tensor(THREE_ROWS, device=b.device)
        rsum, dsum = np.zeros(n, np.int64), np.zeros(n, np.int32)
        for _ in range(K):
            _, r, d = twin.step(twin.policy_linear(w).actions, obs="none")
            rsum += r.cpu().numpy()
            dsum += d.cpu().numpy()
        ret, eps = b.play_linear(w, K)
        assert_same_state(b, twin, "autoreset none")
        assert np.array_equal(ret.cpu().numpy(), rsum) and np.array_equal(eps.cpu().numpy(), dsum)
        assert dsum.sum() > 0
    finally:
        b.close()
        twin.close()


# ------------------------------------------------------------------ 7. errors
@pytest.mark.gpu
def test_abi_errors():
    import torch
    from gym_simpletetris_amd import _lib as C
    L = C.load()
    ctx = ctypes.c_void_p()
    n = 8
    assert L.st_create(ctypes.byref(ctx), ctypes.byref(C.Config(10, 20, 0, 0, 0)), 0, n) == C.ST_OK
    try:
        w = torch.zeros((1, NF), dtype=torch.float32, device="cuda")
        sl = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        ac = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
        sc = torch.full((n,), -7, dtype=torch.float32, device="cuda")
        bf = torch.full((NF, n), -7, dtype=torch.int32, device="cuda")
        ret = torch.zeros(n, dtype=torch.int64, device="cuda")
        pw, ps, pa, pc, pb, pr = (ctypes.c_void_p(x.data_ptr()) for x in (w, sl, ac, sc, bf, ret))

        def both_estate():
            assert L.st_policy_linear(ctx, pw, 1, ps, None, None, None, None) == C.ST_ESTATE
            assert b"st_policy_linear" in L.st_last_error()
            assert L.st_play_linear(ctx, pw, 1, 1, pr, None, None, None, None, None) == C.ST_ESTATE
            assert b"st_play_linear" in L.st_last_error()
        both_estate()                                                              # before seed
        seeds = np.arange(n, dtype=np.uint64)
        assert L.st_seed(ctx, ctypes.c_void_p(seeds.ctypes.data), None) == C.ST_OK
        both_estate()                                                              # before reset
        assert L.st_reset(ctx, None, None) == C.ST_OK
        assert L.st_policy_linear(ctx, pw, 1, None, None, None, None, None) == C.ST_EINVAL  # every output NULL
        assert L.st_policy_linear(ctx, None, 1, ps, None, None, None, None) == C.ST_EINVAL
        assert L.st_policy_linear(ctx, pw, 0, ps, None, None, None, None) == C.ST_EINVAL
        assert L.st_play_linear(ctx, None, 1, 1, pr, None, None, None, None, None) == C.ST_EINVAL
        assert L.st_play_linear(ctx, pw, 0, 1, pr, None, None, None, None, None) == C.ST_EINVAL
        # each single output works alone
        for k, args in enumerate(((ps, None, None, None), (None, pa, None, None), (None, None, pc, None),
                                  (None, None, None, pb))):
            assert L.st_policy_linear(ctx, pw, 1, *args, None) == C.ST_OK, k
        torch.cuda.synchronize()
        assert (sl >= 0).all() and (sl < 64).all() and (ac <= 6).all() and (sc == 0).all()
        assert (bf[VALID] == 1).all()
        assert L.st_play_linear(ctx, pw, 1, -3, pr, None, None, None, None, None) == C.ST_OK  # k <= 0
        assert L.st_play_linear(ctx, pw, 1, 2, None, None, None, None, None, None) == C.ST_OK  # no output at all
    finally:
        L.st_destroy(ctx)


@pytest.mark.gpu
def test_weights_and_out_tensors_are_checked():
    import torch
    b = _engine().TetrisBatch(8, seeds=list(range(8)))
    try:
        b.reset()
        n, dev = 8, b.device
        w = torch.zeros((2, NF), dtype=torch.float32, device=dev)
        good = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                torch.empty(n, dtype=torch.float32, device=dev), torch.empty((NF, n), dtype=torch.int32, device=dev))
        assert b.policy_linear(w, out=good).feat is good[3]
        only = b.policy_linear(w, out=(None, good[1], None, None))
        assert only.slots is None and only.actions is good[1] and only.scores is None and only.feat is None
        for bad_w in (torch.zeros((2, NF + 1), dtype=torch.float32, device=dev),            # shape
                      torch.zeros((1, 2, NF), dtype=torch.float32, device=dev),
                      torch.zeros((0, NF), dtype=torch.float32, device=dev),
                      torch.zeros((2, NF), dtype=torch.float64, device=dev),                # dtype
                      torch.zeros((2, NF), dtype=torch.float32),                            # device
                      torch.zeros((NF, 2), dtype=torch.float32, device=dev).t(),            # not contiguous
                      torch.zeros(2 * NF, dtype=torch.float32, device=dev)[::2]):
            with pytest.raises(ValueError):
                b.policy_linear(bad_w)
            with pytest.raises(ValueError):
                b.play_linear(bad_w, 1)
        with pytest.raises(TypeError):
            b.policy_linear(1.0)
        with pytest.raises(ValueError):
            b.policy_linear(dict(no_such_row=1.0))
        bads = {0: (torch.empty(n + 1, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
                    torch.empty(n, dtype=torch.int32), torch.empty(2 * n, dtype=torch.int32, device=dev)[::2]),
                1: (torch.empty(n, dtype=torch.int32, device=dev),),
                2: (torch.empty(n, dtype=torch.float64, device=dev),),
                3: (torch.empty((n, NF), dtype=torch.int32, device=dev),
                    torch.empty((n, NF), dtype=torch.int32, device=dev).t())}
        for k, ts in bads.items():
            for t in ts:
                with pytest.raises(ValueError):
                    b.policy_linear(w, out=tuple(t if i == k else g for i, g in enumerate(good)))
        with pytest.raises(ValueError):
            b.policy_linear(w, out=(None, None, None, None))
        with pytest.raises(ValueError):
            b.policy_linear(w, out=good[:3])
        for kwargs in (dict(returns=torch.zeros(n, dtype=torch.int32, device=dev)),
                       dict(returns=torch.zeros(n + 1, dtype=torch.int64, device=dev)),
                       dict(episodes=torch.zeros(n, dtype=torch.int64, device=dev)),
                       dict(episodes=torch.zeros(n, dtype=torch.int32))):
            with pytest.raises(ValueError):
                b.play_linear(w, 1, **kwargs)
    finally:
        b.close()


@pytest.mark.gpu
def test_vec_env_pass_through():
    """TetrisVecEnv.policy_linear / play_linear are its engine's."""
    import torch
    G = _engine()
    env = G.TetrisVecEnv(16, seed=3, obs_format="packed")
    try:
        env.reset()
        c, e = env.policy_linear(G.GREEDY_WEIGHTS), env.engine.policy_linear(G.GREEDY_WEIGHTS)
        for k in ("slots", "actions", "scores", "feat"):
            assert torch.equal(getattr(c, k), getattr(e, k)), k
        ret, eps = env.play_linear(G.GREEDY_WEIGHTS, 10)
        assert ret.shape == (16,) and eps.shape == (16,)
        obs, rew, done, info = env.step(env.policy_linear(G.GREEDY_WEIGHTS).actions)
        assert obs.shape == (10, 16)
    finally:
        env.close()
