"""st_policy_lookahead / st_play_lookahead (TetrisBatch.policy_lookahead,
.play_lookahead) on the device.

The expectation is never the new kernel: it is lookahead_ref (the oracle plays
every first-ply slot, then every second-ply slot on the board and with the
counters it holds after the first), or a composition by hand of calls that
other modules hold to the oracle (afterstates, step_placements, policy_linear),
or, for the fused loop, the rounds by hand over policy_lookahead itself, which
the tests above it pin."""
import ctypes

import numpy as np
import pytest
import torch

import feature_ref as FR
import lookahead_ref as LR
import placement_ref as PR
from harness import (C4, assert_same_state, cached_ref, check_engine_state, check_mt_state, check_step,
                     engine as _engine, engine_state, pack_cols, raw_state)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, N_W, AGE = 8, 3, 12
SEED0 = {"10x20": 7600, "11x12": 7600, "6x9": 7500}  # chosen on the CPU: the aged oracles meet the conditions below
DEAD = -1.0e6


def _bits(x):
    x = x if isinstance(x, np.ndarray) else x.cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def weights3(features):
    """Three finite weight rows of the set: the published players (or the
    greedy score and a height lover), and a random row of mixed magnitudes."""
    G = _engine()
    rng = np.random.default_rng(41)
    if features == "bcts":
        rows = [G.engine.weight_rows(G.BCTS_WEIGHTS, "bcts")[0], G.engine.weight_rows(G.DELLACHERIE_WEIGHTS, "bcts")[0]]
    else:
        rows = [PR.GREEDY, PR.AGG_UP]
    nf = len(rows[0])
    rows.append((rng.uniform(-1, 1, nf) * 10.0 ** rng.integers(-2, 3, nf)).astype(np.float32))
    return np.stack(rows).astype(np.float32)


def aged_oracle(board, config):
    """8 oracle envs after 12 placement steps, envs 0..3 on the greedy weights
    and 4..7 on AGG_UP (which piles up), with the slots they took."""
    def make():
        kw = PR.case_kw(board, config)
        ob = O.OracleBatch(N, [SEED0[board] + e for e in range(N)], **kw)
        ob.reset()
        h = LR.helper_for(ob)
        slots = np.empty((AGE, N), np.int32)
        for t in range(AGE):
            for i in range(N):
                env = ob.envs[i]
                feat = PR.slot_features(h, ob.board(i).astype(bool), env.shape_id, env.holes, env.piece_height)
                slots[t, i] = PR.choose(PR.GREEDY if i < N // 2 else PR.AGG_UP, feat)
                PR.ref_place_step(ob, i, slots[t, i], "same_step")
        return dict(slots=slots, state=ob.packed_state(), ob=ob)
    return cached_ref(("lookahead_aged", board, config), make)


def ref_plies(board, config, features):
    return cached_ref(("lookahead_plies", board, config, features),
                      lambda: LR.plies_batch(aged_oracle(board, config)["ob"], features))


def aged_batch(board, config):
    ref = aged_oracle(board, config)
    b = _engine().TetrisBatch(N, autoreset="same_step", seeds=[SEED0[board] + e for e in range(N)],
                              **PR.case_kw(board, config))
    b.reset()
    for t in range(AGE):
        b.step_placements(ref["slots"][t], obs="none")
    check_engine_state(b, ref["state"], "aged")
    return b


def check_choice(c, want, what, table=True):
    for name in ("slots", "slots2", "actions"):
        assert np.array_equal(getattr(c, name).cpu().numpy(), want[name]), (what, name)
    assert np.array_equal(_bits(c.scores), _bits(want["scores"])), (what, "scores")
    if table:
        assert np.array_equal(c.slots2_all.cpu().numpy(), want["slots2_all"]), (what, "slots2_all")
        assert np.array_equal(_bits(c.scores_all), _bits(want["scores_all"])), (what, "scores_all")
    else:
        assert c.scores_all is None and c.slots2_all is None


# ------------------------------------------------------------------ 1. against the cell-by-cell reference
@pytest.mark.parametrize("features", ["base", "bcts"])
@pytest.mark.parametrize("config", sorted(PR.CONFIGS))
@pytest.mark.parametrize("board", sorted(PR.BOARDS))
def test_against_the_reference(board, config, features):
    """Every output, float32 bit for bit, for every slot of 8 aged envs with
    three weight rows: without and with first-ply weights, under a mask from
    reachable().steps, and under a mask of zeros.  11x12 has S = 68: both plies
    run their second pass."""
    pb = ref_plies(board, config, features)
    w = weights3(features)
    W = PR.BOARDS[board][0]
    S = 4 * (W + 6)
    b = aged_batch(board, config)
    try:
        before = engine_state(b)
        wd = torch.as_tensor(w, device=b.device)
        # no first-ply weights
        want = LR.score_batch(pb, None, w, DEAD)
        assert want["dead"].any(), "no dead candidate in the sample"
        c = b.policy_lookahead(wd, features=features, table=True)
        assert tuple(c.scores_all.shape) == (N, S) and c.scores_all.dtype == torch.float32
        check_choice(c, want, "w1 none")
        one_ply = b.policy_linear(wd, features=features).slots.cpu().numpy()
        assert np.array_equal(one_ply, [FR.choose(w[e % N_W], pb["plies"][e]["f1"])[0] for e in range(N)])
        differ = int((one_ply != want["slots"]).sum())
        live = sum(len(p["f2"]) for p in pb["plies"])
        print("lookahead", board, config, features, "live s1", live, "dead candidates", int(want["dead"].sum()),
              "choices that differ from one ply", differ)
        assert differ >= 1
        check_choice(b.policy_lookahead(wd, features=features), want, "no table", table=False)
        # first-ply weights, a dead_value within the scores' range, host weights
        want = LR.score_batch(pb, w, w, -300.0)
        check_choice(b.policy_lookahead(w, first_weights=w, dead_value=-300.0, features=features, table=True), want,
                     "w1 = w2")
        # confined to the slots the live piece can reach
        reach = b.reachable(first=False)
        allowed = reach.steps.cpu().numpy()
        assert 0 < (allowed != 0).sum() <= want["cand"].sum()
        want = LR.score_batch(pb, w, w, DEAD, allowed)
        check_choice(b.policy_lookahead(wd, first_weights=wd, features=features, allowed=reach, table=True), want,
                     "reachable")
        # nothing allowed
        zeros = torch.zeros((N, S), dtype=torch.int32, device=b.device)
        want = LR.score_batch(pb, None, w, DEAD, np.zeros((N, S), np.int32))
        assert (want["slots"] == -1).all() and (want["actions"] == 2).all() and not want["scores"].any()
        check_choice(b.policy_lookahead(wd, features=features, allowed=zeros, table=True), want, "mask of zeros")
        assert_same_state(before, b, "policy_lookahead changed the state")
    finally:
        b.close()


# ------------------------------------------------------------------ 2. against the pinned one-ply pieces
@pytest.mark.parametrize("features", ["base", "bcts"])
@pytest.mark.parametrize("board,n", [((10, 20), 256), ((32, 28), 64)], ids=["10x20", "32x28"])
def test_against_the_one_ply_calls_at_a_wider_batch(board, n, features):
    """10x20 with 256 envs, and the largest board, 32x28 with 64 (S = 152: three
    first-ply waves, three second-ply passes, the widest LDS rows), autoreset
    'none', aged 30 greedy placement steps: for every s1 a scratch batch loads
    the snapshot, plays s1 in every env (step_placements) and asks
    policy_linear; where s1 is a live candidate of env e, the table holds
    float32(S1 + that score) and that slot.  Dead candidates hold S1 +
    dead_value and -1, every other slot 0 and -1."""
    G = _engine()
    kw = dict(width=board[0], height=board[1], **C4)
    seeds = [7900 + e for e in range(n)]
    b, scratch = (G.TetrisBatch(n, autoreset="none", seeds=seeds, **kw) for _ in range(2))
    try:
        b.reset()
        scratch.reset()
        b.play_linear(G.GREEDY_WEIGHTS, 30, placements=True)
        w = weights3(features)
        wd = torch.as_tensor(w, device=b.device)
        snap = b.save()
        S = b.n_slots
        feat = b.afterstates(boards=False, features=features).feat.cpu().numpy()  # [n, R, S]
        rows = np.arange(n) % N_W
        s1_scores = np.stack([FR.scores_f32(w[rows[e]], feat[e]) for e in range(n)])
        valid, dead = feat[:, PR.VALID] != 0, feat[:, PR.DEAD] != 0
        c = b.policy_lookahead(wd, first_weights=wd, dead_value=-250.0, features=features, table=True)
        got, got2 = c.scores_all.cpu().numpy(), c.slots2_all.cpu().numpy()
        want = np.zeros((n, S), np.float32)
        want2 = np.full((n, S), -1, np.int32)
        for s1 in range(S):
            live = valid[:, s1] & ~dead[:, s1]
            if live.any():
                scratch.load(snap)
                _, _, done = scratch.step_placements(np.full(n, s1), obs="none")
                assert not done.cpu().numpy()[live].any()
                one = scratch.policy_linear(wd, features=features)
                sc, sl = one.scores.cpu().numpy(), one.slots.cpu().numpy()
                assert (sl[live] >= 0).all()
                want[live, s1] = (s1_scores[live, s1] + sc[live]).astype(np.float32)
                want2[live, s1] = sl[live]
            d = valid[:, s1] & dead[:, s1]
            want[d, s1] = s1_scores[d, s1] + np.float32(-250.0)
        print("one-ply composition", board, features, "live", int((valid & ~dead).sum()), "dead", int((valid & dead).sum()))
        assert (valid & dead).any() and (valid & ~dead).sum() > 10 * n
        assert np.array_equal(got2, want2)
        assert np.array_equal(_bits(got), _bits(want))
        # the choice is the first maximum of the table over the valid slots
        masked = np.where(valid, got, -np.inf)
        assert np.array_equal(c.slots.cpu().numpy(), masked.argmax(axis=1))
        env = np.arange(n)
        assert np.array_equal(_bits(c.scores), _bits(got[env, masked.argmax(axis=1)]))
        assert np.array_equal(c.slots2.cpu().numpy(), got2[env, masked.argmax(axis=1)])
    finally:
        b.close()
        scratch.close()


# ------------------------------------------------------------------ 3. the state
def drop_heavy(T, n, seed=5):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((T, n)) < 0.5, 2, rng.integers(0, 7, (T, n))).astype(np.uint8)


@pytest.mark.parametrize("features", ["base", "bcts"])
def test_the_call_changes_nothing_the_reference_can_see(features):
    """Board, piece and counters in device memory, the state as get_state gives
    it, the snapshot, and 20 further steps against an untouched twin."""
    G = _engine()
    n, kw = 70, dict(width=10, height=20, **C4)
    seeds = [8100 + e for e in range(n)]
    b, twin = (G.TetrisBatch(n, autoreset="same_step", seeds=seeds, **kw) for _ in range(2))
    try:
        acts = drop_heavy(50, n, 21)
        for x in (b, twin):
            x.reset()
            for t in range(30):
                x.step(acts[t], obs="none")
        raw0 = raw_state(b)
        assert ((raw0["stats"][13, :n].view(np.uint32) >> 24) & 1 == 0).any()  # envs without a preview
        c = b.policy_lookahead(G.GREEDY_WEIGHTS if features == "base" else G.BCTS_WEIGHTS, features=features, table=True)
        assert (c.slots.cpu().numpy() >= 0).all()
        raw1 = raw_state(b)
        assert np.array_equal(raw0["board"], raw1["board"])
        rows = [r for r in range(raw0["stats"].shape[0]) if r != 13]
        assert np.array_equal(raw0["stats"][rows], raw1["stats"][rows])
        assert_same_state(b, twin, "around policy_lookahead", fields=("board", "piece", "stats", "mt"))
        snap = twin.save()
        b.policy_lookahead(G.GREEDY_WEIGHTS)
        assert b.save() == snap
        for t in range(30, 50):
            got, want = b.step(acts[t]), twin.step(acts[t])
            for g, x in zip(got, want):
                assert torch.equal(g, x), t
        assert_same_state(b, twin, "20 steps later")
    finally:
        b.close()
        twin.close()


# ------------------------------------------------------------------ 4. play
TINY_T = 30


def tiny_lookahead_player():
    """placement_ref.cpu_player with the two-ply choice: per env and step
    lookahead_ref on the oracle's state (weights and first-ply weights
    THREE_ROWS, row e % 3), then ref_place_step; env 0 starts on
    tiny_blocked_board().  No engine call."""
    def make():
        n, kw, T = PR.TINY["n"], PR.TINY["kw"], TINY_T
        ob = O.OracleBatch(n, [PR.TINY["seed0"] + e for e in range(n)], **kw)
        ob.reset()
        ob.set_state(0, board=PR.tiny_blocked_board(), ay=PR.TINY_AY)
        h = LR.helper_for(ob)
        out = dict(slots=np.empty((T, n), np.int32), obs=np.empty((T, n, kw["width"]), np.uint32),
                   reward=np.empty((T, n), np.int32), done=np.empty((T, n), np.uint8), placed=np.empty((T, n), np.uint8))
        for t in range(T):
            for e in range(n):
                w = PR.THREE_ROWS[e % 3]
                out["slots"][t, e] = LR.lookahead_env(h, ob, e, w, w, DEAD)["slot"]
                out["obs"][t, e], out["reward"][t, e], out["done"][t, e], out["placed"][t, e] = \
                    PR.ref_place_step(ob, e, out["slots"][t, e], "same_step")
        out["final"], out["ob"] = ob.packed_state(), ob
        return out
    return cached_ref("lookahead_tiny_player", make)


def _tiny_batch():
    n, kw = PR.TINY["n"], PR.TINY["kw"]
    b = _engine().TetrisBatch(n, autoreset="same_step", seeds=[PR.TINY["seed0"] + e for e in range(n)], **kw)
    b.reset()
    st = b.get_state(("board", "piece"))
    st["board"][:, 0] = pack_cols(PR.tiny_blocked_board())
    st["piece"][0] |= np.uint32(PR.TINY_AY << 11)
    b.set_state(**st)
    return b


def test_play_equals_the_cpu_player():
    """play_lookahead(k = 30) in one call: returns, episodes, the last step's
    outputs, the final state and the MT state; and one piece at a time: every
    step's reward and done as the increments of returns / episodes."""
    ref = tiny_lookahead_player()
    assert ref["slots"][0, 0] == -1 and ref["placed"][0, 0] == 0 and ref["done"].sum() >= 3
    T = TINY_T
    b, single = _tiny_batch(), _tiny_batch()
    try:
        w = torch.as_tensor(PR.THREE_ROWS, device=b.device)
        ret, eps = b.play_lookahead(w, T, first_weights=w)
        assert np.array_equal(ret.cpu().numpy(), ref["reward"].astype(np.int64).sum(axis=0))
        assert np.array_equal(eps.cpu().numpy(), ref["done"].astype(np.int32).sum(axis=0))
        check_step(ref, T - 1, b.obs, b.reward, b.done)
        check_engine_state(b, ref["final"])
        check_mt_state(b, ref["ob"])
        r1 = torch.zeros(b.n, dtype=torch.int64, device=b.device)
        e1 = torch.zeros(b.n, dtype=torch.int32, device=b.device)
        for t in range(T):
            r0, e0 = r1.clone(), e1.clone()
            single.play_lookahead(w, 1, first_weights=w, returns=r1, episodes=e1)
            assert np.array_equal((r1 - r0).cpu().numpy(), ref["reward"][t]), ("reward", t)
            assert np.array_equal((e1 - e0).cpu().numpy(), ref["done"][t]), ("done", t)
            check_step(ref, t, single.obs, single.reward, single.done)
        check_engine_state(single, ref["final"], "one piece at a time")
    finally:
        b.close()
        single.close()


@pytest.mark.parametrize("features", ["base", "bcts"])
@pytest.mark.parametrize("autoreset", PR.AUTORESETS)
def test_play_equals_the_rounds_by_hand(autoreset, features):
    """10x20, n = 200: play_lookahead(k = 25) against 25 rounds of
    policy_lookahead -> step_placements(its slots): sums, last outputs and the
    state; 10 + 15 chained; k = 0; the caller's `out`."""
    G = _engine()
    n, K = 200, 25
    kw = dict(width=10, height=20, **C4)
    seeds = [8300 + e for e in range(n)]
    one, two, twin = (G.TetrisBatch(n, autoreset=autoreset, seeds=seeds, **kw) for _ in range(3))
    try:
        w = torch.as_tensor(weights3(features), device=one.device)
        w1 = torch.as_tensor(weights3(features)[::-1].copy(), device=one.device)
        for x in (one, two, twin):
            x.reset()
            x.play_linear(G.GREEDY_WEIGHTS, 12, placements=True)  # some height before the comparison
        rsum, dsum = np.zeros(n, np.int64), np.zeros(n, np.int32)
        for _ in range(K):
            c = twin.policy_lookahead(w, first_weights=w1, dead_value=-500.0, features=features)
            last = tuple(x.clone() for x in twin.step_placements(c.slots))
            assert torch.equal(twin.placed != 0, c.slots >= 0)
            rsum += last[1].cpu().numpy()
            dsum += last[2].cpu().numpy()

        def same(b, ret, eps, what, outs=None):
            o, r, d = outs or (b.obs, b.reward, b.done)
            assert_same_state(b, twin, what)
            assert np.array_equal(ret.cpu().numpy(), rsum) and np.array_equal(eps.cpu().numpy(), dsum), what
            assert torch.equal(o, last[0]) and torch.equal(r, last[1]) and torch.equal(d, last[2]), what

        ret, eps = one.play_lookahead(w, K, first_weights=w1, dead_value=-500.0, features=features)
        assert ret.dtype == torch.int64 and eps.dtype == torch.int32
        same(one, ret, eps, "k = 25")
        print("lookahead play", autoreset, features, "episode ends", int(dsum.sum()), "return", int(rsum.sum()))
        out = (torch.empty_like(two.obs), torch.empty_like(two.reward), torch.empty_like(two.done))
        r2, e2 = two.play_lookahead(w, 10, first_weights=w1, dead_value=-500.0, features=features, obs="none")
        r2b, e2b = two.play_lookahead(w, 15, first_weights=w1, dead_value=-500.0, features=features, returns=r2,
                                      episodes=e2, out=out)
        assert r2b is r2 and e2b is e2
        same(two, r2, e2, "k = 10 + 15", out)
        before = (ret.clone(), eps.clone(), one.reward.clone(), one.obs.clone())
        one.play_lookahead(w, 0, first_weights=w1, features=features, returns=ret, episodes=eps)  # k = 0: nothing
        assert_same_state(one, twin, "k = 0")
        assert torch.equal(ret, before[0]) and torch.equal(eps, before[1])
        assert torch.equal(one.reward, before[2]) and torch.equal(one.obs, before[3])
    finally:
        for x in (one, two, twin):
            x.close()


# ------------------------------------------------------------------ 5. errors
def test_abi_errors():
    from gym_simpletetris_amd import _lib as C
    L = C.load()
    ctx = ctypes.c_void_p()
    n, S = 8, 64
    assert L.st_create(ctypes.byref(ctx), ctypes.byref(C.Config(10, 20, 0, 0, 0)), 0, n) == C.ST_OK
    try:
        w = torch.zeros((1, 18), dtype=torch.float32, device="cuda")
        sl = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        tab = torch.full((n, S), 7.0, dtype=torch.float32, device="cuda")
        ret = torch.zeros(n, dtype=torch.int64, device="cuda")
        pw, ps, ptab, pt = (ctypes.c_void_p(x.data_ptr()) for x in (w, sl, tab, ret))
        inf = float("inf")

        def policy(ctx_, fset=0, w2=pw, n_w=1, dead=-1.0, out=ps):
            return L.st_policy_lookahead(ctx_, fset, None, w2, n_w, dead, None, out, None, None, None, None, None, None)

        def play(ctx_, fset=0, w2=pw, n_w=1, dead=-1.0, k=1):
            return L.st_play_lookahead(ctx_, fset, None, w2, n_w, dead, k, pt, None, None, None, None, None)

        def all_estate():
            for fn, name in ((policy, b"st_policy_lookahead"), (play, b"st_play_lookahead")):
                assert fn(ctx) == C.ST_ESTATE
                assert name in L.st_last_error()
        all_estate()  # before seed
        seeds = np.arange(n, dtype=np.uint64)
        assert L.st_seed(ctx, ctypes.c_void_p(seeds.ctypes.data), None) == C.ST_OK
        all_estate()  # before reset
        assert L.st_reset(ctx, None, None) == C.ST_OK
        for fn in (policy, play):
            assert fn(None) == C.ST_EINVAL
            assert fn(ctx, w2=None) == C.ST_EINVAL
            assert fn(ctx, n_w=0) == C.ST_EINVAL
            for bad in (-1, 2):
                assert fn(ctx, fset=bad) == C.ST_EINVAL
            for bad in (inf, -inf, float("nan")):
                assert fn(ctx, dead=bad) == C.ST_EINVAL
        assert policy(ctx, out=None) == C.ST_EINVAL
        torch.cuda.synchronize()
        assert (sl == 77).all() and (ret == 0).all()
        # k <= 0 does nothing; every single output alone is enough
        assert play(ctx, k=0) == C.ST_OK and play(ctx, k=-3) == C.ST_OK
        assert L.st_policy_lookahead(ctx, 1, pw, pw, 1, -1.0, None, None, None, None, None, ptab, None, None) == C.ST_OK
        torch.cuda.synchronize()
        assert (ret == 0).all() and (sl == 77).all()
        # zero weights: a live candidate scores 0.0 + 0.0, a dead one (a piece that an off-board cell above row 0
        # keeps from falling) 0.0 + dead_value, and every other slot is written 0.0
        assert ((tab == 0) | (tab == -1.0)).all() and (tab == 0).sum() > n * S // 2
    finally:
        L.st_destroy(ctx)
