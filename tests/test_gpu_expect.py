"""st_next_weights / st_policy_expect / st_play_expect (TetrisBatch.next_weights,
.policy_expect, .play_expect) on the device.

The expectation is never the new kernel: it is expect_ref (the oracle plays
every first-ply slot, then every second-ply slot of each of the seven pieces on
the board and with the counters it holds after the first; the chain in numpy
float32), or policy_lookahead / next_piece, which test_gpu_lookahead.py and
test_gpu_next_piece.py pin, or, for the fused loop, the rounds by hand over
policy_expect itself, which the tests above it pin.

The reference boards are PR.BOARDS (S up to 68: two passes in both plies); the
largest board, 32x28 (S = 152: the LDS maximum, three first-ply waves, three
second-ply passes), is held against policy_lookahead in test 3, where the
cell-by-cell reference of 7 x 152 x 152 placements per env would take minutes."""
import ctypes

import numpy as np
import pytest
import torch

import expect_ref as EX
import lookahead_ref as LR
import placement_ref as PR
from harness import C4, assert_same_state, cached_ref, check_engine_state, engine as _engine, pack_cols, raw_state
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, N_W, AGE = 8, 3, 12
SEED0 = {"10x20": 7600, "11x12": 7600, "6x9": 7500}  # test_gpu_lookahead's: the aged oracles hold dead candidates
DEAD = -1.0e6
COUNT0 = 6  # ST_STAT_COUNT0


def _bits(x):
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def weights3(features):
    """Three finite weight rows of the set: the published players (or the
    greedy score and a height lover), and a random row of mixed magnitudes."""
    G = _engine()
    rng = np.random.default_rng(43)
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
    return cached_ref(("expect_aged", board, config), make)


def ref_plies(board, config, features):
    return cached_ref(("expect_plies", board, config, features),
                      lambda: EX.plies_batch(aged_oracle(board, config)["ob"], features))


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
    for name in ("slots", "actions"):
        assert np.array_equal(getattr(c, name).cpu().numpy(), want[name]), (what, name)
    assert np.array_equal(_bits(c.scores), _bits(want["scores"])), (what, "scores")
    if table:
        assert np.array_equal(c.slots2_all.cpu().numpy(), want["slots2_all"]), (what, "slots2_all")
        assert np.array_equal(_bits(c.tails), _bits(want["tails"])), (what, "tails")
        assert np.array_equal(_bits(c.scores_all), _bits(want["scores_all"])), (what, "scores_all")
    else:
        assert c.scores_all is None and c.tails is None and c.slots2_all is None


def set_counts(b, counts):
    """Host-written shape counts [n, 7] through set_state."""
    st = b.get_state(("stats",))
    st["stats"][COUNT0:COUNT0 + 7] = np.asarray(counts).T
    b.set_state(**st)


# ------------------------------------------------------------------ 1. against the cell-by-cell reference
VARIANTS = ("no_first_weights", "first_weights", "reachable", "counts_unequal", "counts_equal")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("features", ["base", "bcts"])
@pytest.mark.parametrize("config", sorted(PR.CONFIGS))
@pytest.mark.parametrize("board", sorted(PR.BOARDS))
def test_against_the_reference(board, config, features, variant):
    """Every output, float32 bit for bit, for every slot and every piece of 8
    aged envs with three weight rows.  11x12 has S = 68: both plies run their
    second pass."""
    pb = ref_plies(board, config, features)
    w = weights3(features)
    W = PR.BOARDS[board][0]
    S = 4 * (W + 6)
    b = aged_batch(board, config)
    try:
        wd = torch.as_tensor(w, device=b.device)
        assert np.array_equal(b.next_weights().cpu().numpy(), pb["m"].T)
        if variant == "no_first_weights":
            before = raw_state(b)
            want = EX.score_batch(pb, None, w, DEAD)
            assert want["dead"].any(), "no dead candidate in the sample"
            c = b.policy_expect(wd, features=features, table=True)
            assert tuple(c.tails.shape) == (N, 7, S) and c.tails.dtype == torch.float32
            assert tuple(c.slots2_all.shape) == (N, 7, S) and c.slots2_all.dtype == torch.int32
            check_choice(c, want, variant)
            check_choice(b.policy_expect(wd, features=features), want, "no table", table=False)
            one_ply = b.policy_linear(wd, features=features).slots.cpu().numpy()
            print("expect", board, config, features, "live s1", sum(len(p["f2"][0]) for p in pb["plies"]),
                  "dead candidates", int(want["dead"].sum()), "choices that differ from one ply",
                  int((one_ply != want["slots"]).sum()))
            # nothing allowed
            zeros = torch.zeros((N, S), dtype=torch.int32, device=b.device)
            want = EX.score_batch(pb, None, w, DEAD, np.zeros((N, S), np.int32))
            assert (want["slots"] == -1).all() and (want["actions"] == 2).all() and not want["tails"].any()
            check_choice(b.policy_expect(wd, features=features, allowed=zeros, table=True), want, "mask of zeros")
            after = raw_state(b)
            for k in before:
                assert np.array_equal(before[k], after[k]), k
        elif variant == "first_weights":  # a dead_value within the scores' range, host weights
            want = EX.score_batch(pb, w, w, -300.0)
            check_choice(b.policy_expect(w, first_weights=w, dead_value=-300.0, features=features, table=True), want,
                         variant)
        elif variant == "reachable":  # confined to the slots the live piece can reach
            reach = b.reachable(first=False)
            allowed = reach.steps.cpu().numpy()
            valid = np.stack([p["f1"][PR.VALID] != 0 for p in pb["plies"]])
            assert 0 < (allowed != 0).sum() <= valid.sum()
            want = EX.score_batch(pb, w, w, DEAD, allowed)
            assert np.array_equal(want["cand"], valid & (allowed != 0))
            check_choice(b.policy_expect(wd, first_weights=wd, features=features, allowed=reach, table=True), want,
                         variant)
        else:
            if variant == "counts_unequal":  # one shape at 40, the rest 0: odds 5 against 45
                counts = np.zeros((N, 7), np.int64)
                counts[np.arange(N), np.arange(N) % 7] = 40
            else:
                counts = np.full((N, 7), 11, np.int64)
            m = np.array([EX.weights_of(c) for c in counts])
            assert (m.min(axis=1) == 5).all() and ((m == 5).all() == (variant == "counts_equal"))
            set_counts(b, counts)
            assert np.array_equal(b.next_weights().cpu().numpy(), m.T)
            want = EX.score_batch(pb, w, w, -300.0, m=m)
            check_choice(b.policy_expect(wd, first_weights=wd, dead_value=-300.0, features=features, table=True), want,
                         variant)
    finally:
        b.close()


# ------------------------------------------------------------------ 2. hand-made boards (test_cpu_expect's)
def _crafted(boards, sids, counts):
    """A 6x9 batch whose env e holds bool board boards[e], a fresh piece sids[e]
    and the shape counts counts[e]; holes / piece_height counters 0."""
    n = len(boards)
    b = _engine().TetrisBatch(n, autoreset="none", seeds=list(range(n)), width=6, height=9)
    b.reset()
    st = b.get_state(("board", "piece", "stats"))
    for e in range(n):
        st["board"][:, e] = pack_cols(boards[e])
        st["piece"][e] = (int(st["piece"][e]) & ~7) | int(sids[e])
    st["stats"][3:5] = 0
    st["stats"][COUNT0:COUNT0 + 7] = np.asarray(counts).T
    b.set_state(**st)
    return b


def test_the_crafted_boards():
    """The inputs whose disagreements test_cpu_expect.py asserts in the
    reference: the well board with the O in play (the expectimax choice is
    neither the one-ply nor the O-known choice), and the tall board on which
    every first-ply slot dies, all seven pieces, under odds and a dead_value
    whose chain is not dead_value."""
    W, H = 6, 9
    well = np.zeros((W, H), bool)
    well[1:, H - 4:] = True
    tall = np.ones((W, H), bool)
    tall[:, 0] = False
    for y in range(1, H):
        tall[(y % 2) * 1, y] = False
        tall[3 + (y % 2), y] = False
    kw = dict(width=W, height=H)
    h = PR.helper_oracle(kw)
    lines = np.zeros(PR.NF, np.float32)
    lines[PR.LINES] = 1.0
    b = _crafted([well], [6], [(9, 9, 9, 9, 9, 0, 9)])
    try:
        want = EX.expect(h, well, 6, (9, 9, 9, 9, 9, 0, 9), 0, 0, None, lines, DEAD)
        c = b.policy_expect(lines, table=True)
        one_ply = int(b.policy_linear(lines).slots[0])
        known_o = LR.score(EX.as_lookahead(EX.plies(h, well, 6, 0, 0), 6), None, lines, DEAD)["slot"]
        assert int(c.slots[0]) == want["slot"] and want["slot"] not in (one_ply, known_o)
        assert _bits(c.scores)[0] == _bits(want["score"])
        for name in ("scores_all", "tails"):
            assert np.array_equal(_bits(getattr(c, name))[0], _bits(want[name])), name
        assert np.array_equal(c.slots2_all.cpu().numpy()[0], want["slots2_all"])
    finally:
        b.close()
    counts, dead = (2, 0, 1, 5, 3, 4, 5), -123.456
    b = _crafted([tall] * 7, list(range(7)), [counts] * 7)
    try:
        c = b.policy_expect(PR.GREEDY, first_weights=PR.GREEDY, dead_value=dead, table=True)
        c0 = b.policy_expect(PR.GREEDY, dead_value=dead)
        for sid in range(7):
            want = EX.expect(h, tall, sid, counts, 0, 0, PR.GREEDY, PR.GREEDY, dead)
            assert want["cand"].any() and np.array_equal(want["dead"], want["cand"])
            assert int(c.slots[sid]) == want["slot"] and _bits(c.scores)[sid] == _bits(want["score"])
            for name in ("scores_all", "tails"):
                assert np.array_equal(_bits(getattr(c, name))[sid], _bits(want[name])), (name, sid)
            assert (c.slots2_all[sid] == -1).all()
            assert _bits(c0.scores)[sid] == 0xC2F6E978 != _bits(np.float32(dead))  # the chain's value, not dead_value
    finally:
        b.close()


# ------------------------------------------------------------------ 3. against the lookahead, at a wider batch
@pytest.mark.parametrize("features", ["base", "bcts"])
@pytest.mark.parametrize("board,n", [((10, 20), 256), ((32, 28), 64)], ids=["10x20", "32x28"])
def test_against_the_lookahead_at_a_wider_batch(board, n, features):
    """10x20 with 256 envs, and the largest board, 32x28 with 64 (S = 152: three
    first-ply waves, three second-ply passes, the widest LDS rows), aged 30
    greedy placement steps.  The tail of the piece next_piece() names is
    policy_lookahead's table without first-ply weights (float32 values: its
    0.0f + T reads a -0.0 tail as +0.0), and so is that piece's second-ply slot;
    next_weights() is the rule on the counter rows; the scores are the numpy
    float32 chain over the device's own tails."""
    G = _engine()
    kw = dict(width=board[0], height=board[1], **C4)
    b = G.TetrisBatch(n, autoreset="same_step", seeds=[9300 + e for e in range(n)], **kw)
    try:
        b.reset()
        b.play_linear(G.GREEDY_WEIGHTS, 30, placements=True)
        w = weights3(features)
        wd = torch.as_tensor(w, device=b.device)
        S = b.n_slots
        c = b.policy_expect(wd, dead_value=-250.0, features=features, table=True)
        m = b.next_weights().cpu().numpy().astype(np.int64)  # [7, n]
        counts = b.get_state(("stats",))["stats"][COUNT0:COUNT0 + 7].astype(np.int64)
        assert np.array_equal(m, 5 + counts.max(axis=0) - counts) and m.min() == 5 and m.max() > 5
        nxt = b.next_piece().cpu().numpy().astype(np.int64)
        la = b.policy_lookahead(wd, dead_value=-250.0, features=features, table=True)
        env = np.arange(n)
        tails, sl2 = c.tails.cpu().numpy(), c.slots2_all.cpu().numpy()
        assert np.array_equal(tails[env, nxt], la.scores_all.cpu().numpy())
        assert np.array_equal(sl2[env, nxt], la.slots2_all.cpu().numpy())
        valid = b.afterstates(boards=False, features=features).feat.cpu().numpy()[:, PR.VALID] != 0
        cand = np.broadcast_to(valid[:, None], sl2.shape)
        assert len(set(nxt)) >= 5 and (sl2[cand] >= 0).sum() > 50 * n
        assert (sl2[~cand] == -1).all() and not tails[~cand].any()
        # the chain over the device's tails, elementwise numpy float32
        acc = np.zeros((n, S), np.float32)
        for q in range(7):
            acc = acc + m[q].astype(np.float32)[:, None] * tails[:, q]
        tot = np.float32(0.0) + acc / m.sum(axis=0).astype(np.float32)[:, None]
        assert tot.dtype == np.float32
        want = np.where(valid, tot, np.float32(0.0))
        assert np.array_equal(_bits(c.scores_all), _bits(want))
        masked = np.where(valid, want, -np.inf)
        assert np.array_equal(c.slots.cpu().numpy(), masked.argmax(axis=1))
        assert np.array_equal(_bits(c.scores), _bits(want[env, masked.argmax(axis=1)]))
        print("expect against lookahead", board, features, "candidates", int(valid.sum()), "choices that differ",
              int((c.slots != la.slots).sum().item()))
    finally:
        b.close()


# ------------------------------------------------------------------ 4. the state
def drop_heavy(T, n, seed=5):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((T, n)) < 0.5, 2, rng.integers(0, 7, (T, n))).astype(np.uint8)


@pytest.mark.parametrize("features", ["base", "bcts"])
def test_the_call_changes_nothing(features):
    """Device memory word for word -- board, piece, every counter row with the
    engine's private bits of the MT index row, both MT generation buffers --
    read without st_mt_sync around the call; then the state as get_state gives
    it against an untouched twin, and 50 further steps."""
    G = _engine()
    n, kw = 70, dict(width=10, height=20, **C4)
    seeds = [9500 + e for e in range(n)]
    b, twin = (G.TetrisBatch(n, autoreset="same_step", seeds=seeds, **kw) for _ in range(2))
    try:
        acts = drop_heavy(80, n, 23)
        for x in (b, twin):
            x.reset()
            for t in range(30):
                x.step(acts[t], obs="none")
        raw0 = raw_state(b)
        assert ((raw0["stats"][13, :n].view(np.uint32) >> 24) & 1 == 0).any()  # envs without a preview: none is drawn
        c = b.policy_expect(G.GREEDY_WEIGHTS if features == "base" else G.BCTS_WEIGHTS, features=features, table=True)
        m = b.next_weights()
        assert (c.slots.cpu().numpy() >= 0).all() and (m.cpu().numpy() >= 5).all()
        raw1 = raw_state(b)
        for k in raw0:
            assert np.array_equal(raw0[k], raw1[k]), k
        assert_same_state(b, twin, "around policy_expect")
        for t in range(30, 80):
            got, want = b.step(acts[t]), twin.step(acts[t])
            for g, x in zip(got, want):
                assert torch.equal(g, x), t
        assert_same_state(b, twin, "50 steps later")
    finally:
        b.close()
        twin.close()


# ------------------------------------------------------------------ 5. honesty
@pytest.mark.parametrize("features", ["base", "bcts"])
def test_the_choice_does_not_depend_on_the_random_state(features):
    """Two batches seeded differently hold the same boards, pieces and counters
    (set_state; the MT rows stay their own): policy_expect's outputs are
    bit-equal, while next_piece -- and so policy_lookahead -- tells them apart."""
    G = _engine()
    n, kw = 96, dict(width=10, height=20, **C4)
    src, one, two = (G.TetrisBatch(n, autoreset="same_step", seeds=[s0 + e for e in range(n)], **kw)
                     for s0 in (9700, 19700, 29700))
    try:
        for x in (src, one, two):
            x.reset()
        src.play_linear(G.GREEDY_WEIGHTS, 14, placements=True)
        st = src.get_state(("board", "piece", "stats"))
        for x in (one, two):
            own = x.get_state(("stats",))["stats"]
            stats = st["stats"].copy()
            stats[13] = own[13]  # the MT index stays the batch's own
            x.set_state(board=st["board"], stats=stats, piece=st["piece"])
        assert not np.array_equal(one.get_state(("mt",))["mt"], two.get_state(("mt",))["mt"])
        w = torch.as_tensor(weights3(features), device=one.device)
        a = one.policy_expect(w, first_weights=w, features=features, table=True)
        z = two.policy_expect(w, first_weights=w, features=features, table=True)
        for name in ("slots", "actions", "slots2_all"):
            assert torch.equal(getattr(a, name), getattr(z, name)), name
        for name in ("scores", "scores_all", "tails"):
            assert np.array_equal(_bits(getattr(a, name)), _bits(getattr(z, name))), name
        assert (a.slots >= 0).all()
        assert torch.equal(one.next_weights(), two.next_weights())
        assert not torch.equal(one.next_piece(), two.next_piece())
    finally:
        for x in (src, one, two):
            x.close()


# ------------------------------------------------------------------ 6. play
@pytest.mark.parametrize("features", ["base", "bcts"])
@pytest.mark.parametrize("autoreset", PR.AUTORESETS)
def test_play_equals_the_rounds_by_hand(autoreset, features):
    """10x20, n = 64: play_expect(k = 6) against 6 rounds of policy_expect ->
    step_placements(its slots): sums, last outputs and the state; 2 + 4
    chained; k = 0; the caller's `out`."""
    G = _engine()
    n, K = 64, 6
    kw = dict(width=10, height=20, **C4)
    seeds = [9900 + e for e in range(n)]
    one, two, twin = (G.TetrisBatch(n, autoreset=autoreset, seeds=seeds, **kw) for _ in range(3))
    try:
        w = torch.as_tensor(weights3(features), device=one.device)
        w1 = torch.as_tensor(weights3(features)[::-1].copy(), device=one.device)
        for x in (one, two, twin):
            x.reset()
            x.play_linear(PR.AGG_UP, 22, placements=True)  # piled up: episodes end inside the comparison
        rsum, dsum = np.zeros(n, np.int64), np.zeros(n, np.int32)
        for _ in range(K):
            c = twin.policy_expect(w, first_weights=w1, dead_value=-500.0, features=features)
            last = tuple(x.clone() for x in twin.step_placements(c.slots))
            assert torch.equal(twin.placed != 0, c.slots >= 0)
            rsum += last[1].cpu().numpy()
            dsum += last[2].cpu().numpy()

        def same(b, ret, eps, what, outs=None):
            o, r, d = outs or (b.obs, b.reward, b.done)
            assert_same_state(b, twin, what)
            assert np.array_equal(ret.cpu().numpy(), rsum) and np.array_equal(eps.cpu().numpy(), dsum), what
            assert torch.equal(o, last[0]) and torch.equal(r, last[1]) and torch.equal(d, last[2]), what

        ret, eps = one.play_expect(w, K, first_weights=w1, dead_value=-500.0, features=features)
        assert ret.dtype == torch.int64 and eps.dtype == torch.int32
        same(one, ret, eps, "k = 6")
        print("expect play", autoreset, features, "episode ends", int(dsum.sum()), "return", int(rsum.sum()))
        out = (torch.empty_like(two.obs), torch.empty_like(two.reward), torch.empty_like(two.done))
        r2, e2 = two.play_expect(w, 2, first_weights=w1, dead_value=-500.0, features=features, obs="none")
        r2b, e2b = two.play_expect(w, 4, first_weights=w1, dead_value=-500.0, features=features, returns=r2,
                                   episodes=e2, out=out)
        assert r2b is r2 and e2b is e2
        same(two, r2, e2, "k = 2 + 4", out)
        before = (ret.clone(), eps.clone(), one.reward.clone(), one.obs.clone())
        one.play_expect(w, 0, first_weights=w1, features=features, returns=ret, episodes=eps)  # k = 0: nothing
        assert_same_state(one, twin, "k = 0")
        assert torch.equal(ret, before[0]) and torch.equal(eps, before[1])
        assert torch.equal(one.reward, before[2]) and torch.equal(one.obs, before[3])
    finally:
        for x in (one, two, twin):
            x.close()


# ------------------------------------------------------------------ 7. errors
def test_abi_errors():
    from gym_simpletetris_amd import _lib as C
    L = C.load()
    ctx = ctypes.c_void_p()
    n, S = 8, 64
    assert L.st_create(ctypes.byref(ctx), ctypes.byref(C.Config(10, 20, 0, 0, 0)), 0, n) == C.ST_OK
    try:
        w = torch.zeros((1, 18), dtype=torch.float32, device="cuda")
        sl = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        mm = torch.full((7, n), 77, dtype=torch.int32, device="cuda")
        tab = torch.full((n, 7, S), 7.0, dtype=torch.float32, device="cuda")
        ret = torch.zeros(n, dtype=torch.int64, device="cuda")
        pw, ps, pm, ptab, pt = (ctypes.c_void_p(x.data_ptr()) for x in (w, sl, mm, tab, ret))
        inf = float("inf")

        def policy(ctx_, fset=0, w2=pw, n_w=1, dead=-1.0, out=ps):
            return L.st_policy_expect(ctx_, fset, None, w2, n_w, dead, None, out, None, None, None, None, None, None)

        def play(ctx_, fset=0, w2=pw, n_w=1, dead=-1.0, k=1):
            return L.st_play_expect(ctx_, fset, None, w2, n_w, dead, k, pt, None, None, None, None, None)

        def odds(ctx_, out=pm):
            return L.st_next_weights(ctx_, out, None)

        def all_estate():
            for fn, name in ((policy, b"st_policy_expect"), (play, b"st_play_expect"), (odds, b"st_next_weights")):
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
        assert odds(None) == C.ST_EINVAL and odds(ctx, out=None) == C.ST_EINVAL
        torch.cuda.synchronize()
        assert (sl == 77).all() and (ret == 0).all() and (mm == 77).all()
        # k <= 0 does nothing; every single output alone is enough
        assert play(ctx, k=0) == C.ST_OK and play(ctx, k=-3) == C.ST_OK
        assert L.st_policy_expect(ctx, 1, pw, pw, 1, -1.0, None, None, None, None, None, ptab, None, None) == C.ST_OK
        assert odds(ctx) == C.ST_OK
        torch.cuda.synchronize()
        assert (ret == 0).all() and (sl == 77).all()
        # one piece spawned since the reset: its count is 1, so it has odds 5 and the others 6
        assert ((mm == 5).sum(dim=0) == 1).all() and ((mm == 6).sum(dim=0) == 6).all()
        # zero weights: every tail is 0.0 (a live candidate) or dead_value, and every other slot is written 0.0
        assert ((tab == 0) | (tab == -1.0)).all() and (tab == 0).sum() > n * 7 * S // 2
    finally:
        L.st_destroy(ctx)


def test_abi_errors_leave_a_live_context_untouched():
    """Bad set, n_w = 0, all outputs NULL and a NaN dead_value on a batch in
    mid-game: ST_EINVAL, and device memory word for word as before."""
    from gym_simpletetris_amd import _lib as C
    G = _engine()
    b = G.TetrisBatch(70, autoreset="same_step", seeds=[9990 + e for e in range(70)], width=10, height=20)
    try:
        b.reset()
        b.play_linear(G.GREEDY_WEIGHTS, 9)
        torch.cuda.synchronize()
        before = raw_state(b)
        w = torch.zeros((1, 18), dtype=torch.float32, device=b.device)
        sl = torch.full((b.n,), 77, dtype=torch.int32, device=b.device)
        ret = torch.zeros(b.n, dtype=torch.int64, device=b.device)
        pw, ps, pt = (ctypes.c_void_p(x.data_ptr()) for x in (w, sl, ret))
        L, ctx = b._L, b._ctx
        for fset, n_w, dead, out in ((2, 1, -1.0, ps), (-1, 1, -1.0, ps), (0, 0, -1.0, ps), (0, 1, -1.0, None),
                                     (0, 1, float("nan"), ps)):
            assert L.st_policy_expect(ctx, fset, None, pw, n_w, dead, None, out, None, None, None, None, None,
                                      None) == C.ST_EINVAL
            assert b"st_policy_expect" in L.st_last_error()
            if out is not None:
                assert L.st_play_expect(ctx, fset, None, pw, n_w, dead, 3, pt, None, None, None, None,
                                        None) == C.ST_EINVAL
                assert b"st_play_expect" in L.st_last_error()
        assert L.st_next_weights(ctx, None, None) == C.ST_EINVAL
        torch.cuda.synchronize()
        assert (sl == 77).all() and (ret == 0).all()
        after = raw_state(b)
        for k in before:
            assert np.array_equal(before[k], after[k]), k
    finally:
        b.close()
