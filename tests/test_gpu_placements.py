"""st_place / st_step_placements / st_play_linear_placements (TetrisBatch.place,
.step_placements, .play_linear(placements=True)).

The expectation is always the oracle, never the new kernels: a placement step
is placement_ref.ref_place_step -- OracleBatch.set_state on a valid slot (a
few-line restatement of is_occupied decides), then step_one(i, 2) -- or, where
two engine paths are compared, a loop by hand over calls that are themselves
checked against it.  The conditions on the oracle samples (deaths, lines,
valid fractions) are tests of their own in test_cpu_placements.py.
"""
import ctypes

import numpy as np
import pytest

import placement_ref as P
from harness import (C4, assert_same_state, check_engine_state, check_mt_state, check_step, engine as _engine,
                     engine_state, pack_cols)
from oracle import oracle as O

NF = P.NF


# ------------------------------------------------------------------ 1. step_placements against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("autoreset", P.AUTORESETS)
@pytest.mark.parametrize("config", sorted(P.CONFIGS))
@pytest.mark.parametrize("board", sorted(P.BOARDS))
def test_step_placements_against_the_oracle(board, config, autoreset):
    """40 consecutive placement steps of 70 envs on random slots in
    [-2, S + 2): obs, reward, done and the commit flags of every step, then the
    whole engine state and the MT19937 state."""
    ref = P.random_run(board, config, autoreset)
    b = _engine().TetrisBatch(P.N, autoreset=autoreset, seeds=P.case_seeds(board, config), **P.case_kw(board, config))
    try:
        b.reset()
        for t in range(P.T_RANDOM):
            obs, rew, done = b.step_placements(ref["slots"][t])
            check_step(ref, t, obs, rew, done)
            assert np.array_equal(b.placed.cpu().numpy(), ref["placed"][t]), ("placed", t)
        check_engine_state(b, ref["final"])
        check_mt_state(b, ref["ob"])
    finally:
        b.close()


# ------------------------------------------------------------------ 2. place changes only the piece row
@pytest.mark.gpu
@pytest.mark.parametrize("board", sorted(P.BOARDS))
def test_place_changes_only_the_piece_row(board):
    """lock_delay = 3 and a resting piece (one hard drop: lock counter 1):
    after place(), board, every counter row but the piece's and the MT state
    are bit-equal; the piece words equal the oracle's after its commit; an
    invalid slot leaves its word, nonzero lock counter included, as it was."""
    import torch
    kw, n = P.case_kw(board, "c4_lock3"), P.N
    W = kw["width"]
    S = 4 * (W + 6)
    seeds = [6200 + e for e in range(n)]
    b = _engine().TetrisBatch(n, autoreset="none", seeds=seeds, **kw)
    ob = O.OracleBatch(n, seeds, **kw)
    try:
        b.reset()
        ob.reset()
        drop = torch.full((n,), 2, dtype=torch.uint8, device=b.device)
        for _ in range(5):  # a piece locks (four hard drops), the next one rests
            b.step(drop, obs="none")
            for i in range(n):
                ob.step_one(i, 2)
        check_engine_state(b, ob.packed_state(), "before place")
        before = engine_state(b)
        assert ((before["piece"] >> 17) == 1).all()  # every piece rests, lock counter 1
        slots = np.random.default_rng(77).integers(-2, S + 2, n)
        slots[:4] = (-1, S, 0, S - 1)  # (slots 0 and S - 1: anchors off the board, never valid)
        want_placed = np.array([P.commit(ob, i, slots[i]) for i in range(n)], np.uint8)
        assert 0 < want_placed.sum() < n and not want_placed[:4].any()
        guard = torch.full((n + 6,), 249, dtype=torch.uint8, device=b.device)
        placed = b.place(torch.as_tensor(slots, device=b.device), out=guard[:n])
        assert placed.data_ptr() == guard.data_ptr() and (guard[n:] == 249).all()
        assert np.array_equal(placed.cpu().numpy(), want_placed)
        after = engine_state(b)
        assert np.array_equal(after["board"], before["board"])
        assert np.array_equal(after["mt"], before["mt"])
        rows = [r for r in range(after["stats"].shape[0]) if r != 14]
        assert np.array_equal(after["stats"][rows], before["stats"][rows])
        assert np.array_equal(after["piece"], ob.packed_state()["piece"])
        keep = want_placed == 0
        assert np.array_equal(after["piece"][keep], before["piece"][keep])
        ok = ~keep
        assert ((after["piece"][ok] >> 17) == 3).all() and (((after["piece"][ok] >> 11) & 63) == 0).all()
        assert np.array_equal(after["piece"][ok] & 7, before["piece"][ok] & 7)
        # the reused buffer, and a host sequence: the same commit again (valid slots stay valid)
        again = b.place(slots.tolist())
        assert again is b.placed and np.array_equal(again.cpu().numpy(), want_placed)
        assert_same_state(after, b, "a second place of the same slots")
    finally:
        b.close()


# ------------------------------------------------------------------ 3. the afterstate promise holds
@pytest.mark.gpu
@pytest.mark.parametrize("board,config", [("10x20", "c4_lock3"), ("6x9", "default"), ("11x12", "c4_lock3")])
def test_the_afterstate_promise_holds(board, config):
    """afterstates(boards=True), then step_placements on valid slots under
    autoreset 'none': the reward is the slot's REWARD, done its DEAD, the board
    of an env that lives its afterstate board, time + 1 and lines + LINES.
    Even envs take the greedy weights' slot, odd envs a random valid one; dead
    envs are reset between the rounds."""
    import torch
    kw, n = P.case_kw(board, config), P.N
    G = _engine()
    b = G.TetrisBatch(n, autoreset="none", seeds=[6400 + e for e in range(n)], **kw)
    rng = np.random.default_rng(5)
    try:
        b.reset()
        deaths = lines = 0
        for t in range(30):
            a = b.afterstates(boards=True)
            feat, boards = a.feat.cpu().numpy(), a.boards.cpu().numpy().view(np.uint32)
            greedy = b.policy_linear(G.GREEDY_WEIGHTS).slots.cpu().numpy()
            slots = greedy.copy()
            for e in range(1, n, 2):
                slots[e] = rng.choice(np.flatnonzero(feat[e, P.VALID]))
            assert (slots >= 0).all()
            st0 = b.get_state(("stats",))["stats"]
            _, rew, done = b.step_placements(slots, obs="none")
            rew, done = rew.cpu().numpy(), done.cpu().numpy()
            st1 = b.get_state(("board", "stats"))
            env = np.arange(n)
            assert b.placed.all()
            assert np.array_equal(rew, feat[env, P.REWARD, slots]), t
            assert np.array_equal(done, feat[env, P.DEAD, slots] != 0), t
            live = ~done
            assert np.array_equal(st1["board"][:, live], boards[env, :, slots].T[:, live]), t
            assert np.array_equal(st1["stats"][0], st0[0] + 1), t
            assert np.array_equal(st1["stats"][2], st0[2] + feat[env, P.LINES, slots]), t
            deaths += int(done.sum())
            lines += int(feat[env, P.LINES, slots].sum())
            if done.any():
                b.reset(torch.as_tensor(done.astype(np.uint8), device=b.device))
        print("afterstate promise", board, config, "deaths", deaths, "lines", lines)
        assert deaths >= 1 or board != "6x9", deaths  # (nine rows, thirty pieces)
    finally:
        b.close()


# ------------------------------------------------------------------ 4. play_linear(placements=True) = the loop by hand
def _weights(n_w):
    if n_w == 1:
        return P.GREEDY[None].copy()
    rng = np.random.default_rng(31)
    w = (rng.uniform(-1, 1, (n_w, NF)) * 10.0 ** rng.integers(-2, 3, (n_w, NF))).astype(np.float32)
    w[:3] = P.THREE_ROWS
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("autoreset", P.AUTORESETS)
@pytest.mark.parametrize("n_w", [1, 7])
@pytest.mark.parametrize("board", [(6, 9), (13, 12)], ids=["6x9", "13x12"])
def test_play_linear_placements_equals_the_loop_by_hand(board, n_w, autoreset):
    """k = 37 (it crosses the 32-row ring) in one call, as 20 + 17 chained, and
    as 37 rounds of policy_linear -> step_placements(its slots) by hand: the
    same returns, episodes, last outputs and engine state; then k = 1.  The
    loop by hand is policy_linear (the parent's kernel) and step_placements
    (test 1 holds it to the oracle), so the committing policy kernel is never
    its own expectation.  13x12 has S = 76: rotation 3 at x >= 4 are slots
    64..72, which the kernel finds in its second slot pass -- the committed
    word of such a winner is decoded from a slot number past the first pass."""
    import torch
    n, K = P.N, 37
    kw = dict(width=board[0], height=board[1], **C4)
    seeds = [6600 + e for e in range(n)]
    G = _engine()
    one, two, twin = (G.TetrisBatch(n, autoreset=autoreset, seeds=seeds, **kw) for _ in range(3))
    try:
        for x in (one, two, twin):
            x.reset()
        w = torch.as_tensor(_weights(n_w), device=one.device)
        rsum, dsum = np.zeros(n, np.int64), np.zeros(n, np.int32)
        last, none_seen, second_pass = None, 0, 0

        def loop(k):
            nonlocal last, none_seen, second_pass
            for _ in range(k):
                c = twin.policy_linear(w)
                none_seen += int((c.slots < 0).sum())
                second_pass += int((c.slots >= 64).sum())
                last = tuple(x.clone() for x in twin.step_placements(c.slots))
                assert torch.equal(twin.placed != 0, c.slots >= 0)
                rsum[:] += last[1].cpu().numpy()
                dsum[:] += last[2].cpu().numpy()

        def same(b, ret, eps, what, obs=True):
            assert_same_state(b, twin, what)
            assert np.array_equal(ret.cpu().numpy(), rsum) and np.array_equal(eps.cpu().numpy(), dsum), what
            assert torch.equal(b.reward, last[1]) and torch.equal(b.done, last[2]), what
            if obs:
                assert torch.equal(b.obs, last[0]), what

        loop(K)
        ret, eps = one.play_linear(w, K, obs="packed", placements=True)
        assert ret.dtype == torch.int64 and eps.dtype == torch.int32
        same(one, ret, eps, "k = 37")
        print("placement play", board, n_w, autoreset, "episode ends", int(dsum.sum()), "second-pass winners", second_pass)
        if board == (6, 9):
            assert dsum.sum() > 0  # (nine rows, 37 pieces)
        elif n_w == 7:  # mixed weight rows on 70 envs x 37 pieces: some winner is a rotation 3 in the right half
            assert second_pass > 0
        r2, e2 = two.play_linear(w, 20, placements=True)
        r2b, e2b = two.play_linear(w, 17, returns=r2, episodes=e2, obs="packed", placements=True)
        assert r2b is r2 and e2b is e2
        same(two, r2, e2, "k = 20 + 17")
        loop(1)
        one.play_linear(w, 1, returns=ret, episodes=eps, obs="packed", placements=True)
        same(one, ret, eps, "k = 1")
        before = (ret.clone(), eps.clone(), one.reward.clone())
        one.play_linear(w, 0, returns=ret, episodes=eps, placements=True)  # k = 0 changes nothing
        assert_same_state(one, twin, "k = 0")
        assert torch.equal(ret, before[0]) and torch.equal(eps, before[1]) and torch.equal(one.reward, before[2])
        # without accumulators the steps write the caller's outputs themselves: raw call
        loop(2)
        L, s = one._L, one._stream()
        assert L.st_play_linear_placements(one._ctx, ctypes.c_void_p(w.data_ptr()), n_w, 2, None, None, None,
                                           ctypes.c_void_p(one.reward.data_ptr()),
                                           ctypes.c_void_p(one.done.data_ptr()), s) == 0
        assert_same_state(one, twin, "no accumulators")
        assert torch.equal(one.reward, last[1]) and torch.equal(one.done, last[2])
    finally:
        for x in (one, two, twin):
            x.close()


# ------------------------------------------------------------------ 5. the engine loop equals the CPU player
def _tiny_batch(autoreset="same_step"):
    n, kw = P.TINY["n"], P.TINY["kw"]
    b = _engine().TetrisBatch(n, autoreset=autoreset, seeds=[P.TINY["seed0"] + e for e in range(n)], **kw)
    b.reset()
    st = b.get_state(("board", "piece"))
    st["board"][:, 0] = pack_cols(P.tiny_blocked_board())
    st["piece"][0] |= np.uint32(P.TINY_AY << 11)
    b.set_state(**st)
    return b


@pytest.mark.gpu
def test_engine_loop_equals_the_cpu_player():
    """The oracle plays THREE_ROWS with ref_place_step on slots chosen by the
    numpy rule from oracle-derived feature rows; play_linear(placements=True)
    gives its returns, episodes, last outputs and final state, and the loop by
    hand every one of its steps and slots."""
    import torch
    ref = P.tiny_ref()
    T = P.TINY["T"]
    b, hand = _tiny_batch(), _tiny_batch()
    try:
        w = torch.as_tensor(P.THREE_ROWS, device=b.device)
        ret, eps = b.play_linear(w, T, obs="packed", placements=True)
        assert np.array_equal(ret.cpu().numpy(), ref["returns"]), (ret, ref["returns"])
        assert np.array_equal(eps.cpu().numpy(), ref["episodes"])
        check_step(ref, T - 1, b.obs, b.reward, b.done)
        check_engine_state(b, ref["final"])
        check_mt_state(b, ref["ob"])
        for t in range(T):
            c = hand.policy_linear(w)
            assert np.array_equal(c.slots.cpu().numpy(), ref["slots"][t]), ("slot", t)
            check_step(ref, t, *hand.step_placements(c.slots))
            assert np.array_equal(hand.placed.cpu().numpy(), ref["placed"][t]), ("placed", t)
        check_engine_state(hand, ref["final"], "by hand")
    finally:
        b.close()
        hand.close()


# ------------------------------------------------------------------ 6. the default keyword is unchanged
@pytest.mark.gpu
@pytest.mark.parametrize("autoreset", P.AUTORESETS)
def test_play_linear_default_is_the_primitive_action_loop(autoreset):
    """Passes before and after the placement step was added: play_linear
    without the keyword is policy_linear -> step on primitive actions, bit
    for bit (the COMMIT = false instantiation of the policy kernel)."""
    import torch
    n, K = P.N, 37
    kw = dict(width=10, height=20, **C4)
    seeds = [6800 + e for e in range(n)]
    G = _engine()
    b = G.TetrisBatch(n, autoreset=autoreset, seeds=seeds, **kw)
    twin = G.TetrisBatch(n, autoreset=autoreset, seeds=seeds, **kw)
    try:
        b.reset()
        twin.reset()
        w = torch.as_tensor(P.THREE_ROWS, device=b.device)
        rsum, dsum = np.zeros(n, np.int64), np.zeros(n, np.int32)
        for _ in range(K):
            obs, r, d = twin.step(twin.policy_linear(w).actions)
            rsum += r.cpu().numpy()
            dsum += d.cpu().numpy()
        ret, eps = b.play_linear(w, K, obs="packed")
        assert_same_state(b, twin, "default play_linear")
        assert np.array_equal(ret.cpu().numpy(), rsum) and np.array_equal(eps.cpu().numpy(), dsum)
        assert torch.equal(b.obs, obs) and torch.equal(b.reward, r) and torch.equal(b.done, d)
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
        sl = torch.full((n,), 7, dtype=torch.int32, device="cuda")  # rot 0, x = 4: free on the empty board
        pl = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
        rew = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        ret = torch.zeros(n, dtype=torch.int64, device="cuda")
        pw, ps, pp, pr, pt = (ctypes.c_void_p(x.data_ptr()) for x in (w, sl, pl, rew, ret))

        def all_estate():
            assert L.st_place(ctx, ps, pp, None) == C.ST_ESTATE
            assert b"st_place" in L.st_last_error()
            assert L.st_step_placements(ctx, ps, pp, None, pr, None, None) == C.ST_ESTATE
            assert b"st_step_placements" in L.st_last_error()
            assert L.st_play_linear_placements(ctx, pw, 1, 1, pt, None, None, pr, None, None) == C.ST_ESTATE
            assert b"st_play_linear_placements" in L.st_last_error()
        all_estate()                                                               # before seed
        seeds = np.arange(n, dtype=np.uint64)
        assert L.st_seed(ctx, ctypes.c_void_p(seeds.ctypes.data), None) == C.ST_OK
        all_estate()                                                               # before reset
        assert L.st_reset(ctx, None, None) == C.ST_OK
        views = C.StateViews()
        assert L.st_state(ctx, ctypes.byref(views)) == C.ST_OK

        def pieces():
            t = torch.empty(n, dtype=torch.int32, device="cuda")
            assert L.st_copy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(views.piece), 4 * n, None) == C.ST_OK
            torch.cuda.synchronize()
            return t.cpu().numpy()
        p0 = pieces()
        assert L.st_place(ctx, None, pp, None) == C.ST_EINVAL
        assert L.st_step_placements(ctx, None, pp, None, pr, None, None) == C.ST_EINVAL
        assert L.st_play_linear_placements(ctx, None, 1, 1, pt, None, None, pr, None, None) == C.ST_EINVAL
        assert L.st_play_linear_placements(ctx, pw, 0, 1, pt, None, None, pr, None, None) == C.ST_EINVAL
        torch.cuda.synchronize()
        assert np.array_equal(pieces(), p0) and (pl == 77).all() and (rew == -7).all() and (ret == 0).all()
        # d_placed and every step output may be NULL; k <= 0 does nothing
        assert L.st_place(ctx, ps, None, None) == C.ST_OK
        assert L.st_play_linear_placements(ctx, pw, 1, -3, pt, None, None, pr, None, None) == C.ST_OK
        torch.cuda.synchronize()
        assert (rew == -7).all() and (ret == 0).all()
        got = pieces()
        assert np.array_equal(got, (p0 & 7) | (4 << 5))  # rot 0, anchor (4, 0), lock counter max(lock_delay, 0) = 0
        assert L.st_step_placements(ctx, ps, None, None, None, None, None) == C.ST_OK
        assert L.st_play_linear_placements(ctx, pw, 1, 2, None, None, None, None, None, None) == C.ST_OK
        torch.cuda.synchronize()
    finally:
        L.st_destroy(ctx)


@pytest.mark.gpu
def test_slots_and_out_tensors_are_checked():
    import torch
    n = 8
    b = _engine().TetrisBatch(n, seeds=list(range(n)))
    try:
        b.reset()
        dev = b.device
        before = engine_state(b)
        good = torch.full((n,), -1, dtype=torch.int32, device=dev)
        for call in (b.place, b.step_placements):
            for bad in (torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.bool, device=dev),
                        torch.zeros(n, dtype=torch.complex64, device=dev)):
                with pytest.raises(TypeError):
                    call(bad)
            for bad in (torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros((1, n), dtype=torch.int32),
                        [0] * (n - 1), np.zeros((n, 2), np.int64)):
                with pytest.raises(ValueError):
                    call(bad)
        for bad_out in (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.uint8, device=dev),
                        torch.zeros(n, dtype=torch.uint8), torch.zeros(2 * n, dtype=torch.uint8, device=dev)[::2]):
            with pytest.raises(ValueError):
                b.place(good, out=bad_out)
        with pytest.raises(ValueError):
            b.step_placements(good, obs="f32")
        with pytest.raises(ValueError):
            b.step_placements(good, out=(b.obs, b.reward, torch.zeros(n, dtype=torch.int32, device=dev)))
        assert_same_state(before, b, "an error changed the state")
        # an int64 tensor on the host is converted, like placement_actions's slots
        assert not b.place(torch.full((n,), -1, dtype=torch.int64)).any()
        # 10x20, spawn piece on an empty board: slot(0, 4) is free
        assert b.place(np.full(n, b.slot(0, 4))).all()
        out = (torch.empty_like(b.obs), torch.empty_like(b.reward), torch.empty_like(b.done))
        o, r, d = b.step_placements(good, out=out)
        assert o is out[0] and r is out[1] and d is out[2] and not b.placed.any()
        assert b.step_placements(good, obs="none")[0] is None
    finally:
        b.close()


# ------------------------------------------------------------------ 8. the vector env passes them through
@pytest.mark.gpu
def test_vec_env_pass_through():
    import torch
    G = _engine()
    env = G.TetrisVecEnv(16, seed=3, obs_format="packed")
    twin = G.TetrisVecEnv(16, seed=3, obs_format="packed")
    try:
        env.reset()
        twin.reset()
        slots = env.policy_linear(G.GREEDY_WEIGHTS).slots
        assert torch.equal(env.place(slots), twin.engine.place(slots))
        assert_same_state(env, twin, "place")
        obs, rew, done = env.step_placements(slots)
        want = twin.engine.step_placements(slots)
        assert obs.shape == (10, 16) and env.engine.placed.all()
        for g, x in zip((obs, rew, done), want):
            assert torch.equal(g, x)
        ret, eps = env.play_linear(G.GREEDY_WEIGHTS, 10, placements=True)
        r2, e2 = twin.engine.play_linear(G.GREEDY_WEIGHTS, 10, placements=True)
        assert torch.equal(ret, r2) and torch.equal(eps, e2)
        assert_same_state(env, twin, "play_linear(placements=True)")
        counts = env.engine.get_state(("stats",))["stats"][6:13].sum(axis=0)
        assert (counts >= 11).all()  # a piece per iteration (and the one in play)
    finally:
        env.close()
        twin.close()
