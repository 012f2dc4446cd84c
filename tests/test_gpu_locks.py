"""st_lock_set / st_afterstates_at / st_routes_at / st_policy_locks /
st_play_locks (TetrisBatch.lock_set, .afterstates_at, .routes_at,
.policy_locks, .play_locks) against lock_ref: every lock position of every env
of the reachability sample and of the crafted states -- the tucks under
overhangs that are no slot's landing included --, their rows and boards, the
routes into them played out on the oracle, the fused player against the numpy
chain, the play loop against the loop by hand and an oracle replay, and the
error paths."""
import ctypes

import numpy as np
import pytest

import feature_ref as FR
import lock_ref as LR
import placement_ref as PR
import reach_ref as R
import route_ref as RR
from harness import (assert_same_state, cached_ref, check_mt_state, check_step, engine, engine_state, pack_cols)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROUTE_ENVS = 20  # envs a case whose every lock position is routed and played out


def _torch():
    import torch
    return torch


def _np(t):
    return t.cpu().numpy()


def load_oracle(b, ob, idx=None):
    """Every env's state of an OracleBatch (envs idx of it) into the batch."""
    idx = np.arange(ob.n) if idx is None else np.asarray(idx)
    ps = ob.packed_state()
    st = b.get_state(("board", "piece", "stats", "mt"))
    st["board"][:] = ps["board"][:, idx]
    st["piece"][:] = ps["piece"][idx]
    st["stats"][:13] = ps["stats"][:, idx]
    rng = np.ctypeslib.as_array(ob.envs)["rng"]
    st["stats"][13] = rng["index"][idx]
    st["mt"][:] = rng["mt"][idx]
    b.set_state(**st)


def clone_oracle(ob, kw):
    c = O.OracleBatch(ob.n, [0] * ob.n, **kw)
    ctypes.memmove(ctypes.addressof(c.envs), ctypes.addressof(ob.envs), ctypes.sizeof(ob.envs))
    return c


def sample_batch(board, config, autoreset="same_step"):
    kw = R.case_kw(board, config)
    b = engine().TetrisBatch(R.N, autoreset=autoreset, seeds=R.case_seeds(board, config), **kw)
    b.reset()
    smp = R.sample(board, config)
    load_oracle(b, smp["ob"])
    return b, smp, kw


def graphs(board, config):
    """route_ref's graph of every env of the sample."""
    def make():
        smp, kw = R.sample(board, config), R.case_kw(board, config)
        h, hf = R.helpers(kw)
        return [RR.env_routes(h, hf, smp["ob"], e) for e in range(R.N)]
    return cached_ref(("route_graphs", board, config), make)


def route_words(routes):
    return np.array([RR.pack(r) for r in routes], np.uint64).reshape(len(routes), RR.ROUTE_WORDS)


def got_words(rt):
    return _np(rt.route).view(np.uint64).T


def pos_table(W, locks, cap, fill=-1):
    """int32 [n, cap]: every env's positions ascending, `fill` behind them, cut at cap."""
    out = np.full((len(locks), cap), fill, np.int32)
    for e, lk in enumerate(locks):
        p = LR.pos_list(W, lk)[:cap]
        out[e, :len(p)] = p
    return out


def crafted_groups():
    groups = {}
    for case in R.CRAFTED:
        groups.setdefault(tuple(sorted(case[1].items())), []).append(case)
    return list(groups.values())


def crafted_batch(cases):
    n, cfg = len(cases), cases[0][1]
    b = engine().TetrisBatch(n, seeds=list(range(40, 40 + n)), width=R.CW, height=R.CH, **cfg)
    b.reset()
    st = b.get_state(("board", "piece"))
    for i, (_, _, board, sid, rot, x, y, l, _) in enumerate(cases):
        st["board"][:, i] = pack_cols(board)
        st["piece"][i] = sid | rot << 3 | x << 5 | y << 11 | l << 17
    b.set_state(**st)
    return b


# ------------------------------------------------------------------ 1. lock_set
@pytest.mark.parametrize("board,config", R.CASES)
def test_lock_set_equals_the_oracle_search(board, config):
    b, smp, _ = sample_batch(board, config)
    ls = LR.sample(board, config)
    W, S = b.width, b.n_slots
    before = engine_state(b)
    top = int(ls["count"].max())
    for cap in (64, top, 3):
        got = b.lock_set(cap=cap)
        rows = _np(got.rows).view(np.uint32)
        assert rows.shape == (R.N, S) and np.array_equal(rows, ls["rows"]), np.argwhere(rows != ls["rows"])[:8]
        assert np.array_equal(_np(got.count), ls["count"])
        assert np.array_equal(_np(got.pos), pos_table(W, ls["locks"], cap)), cap
    only = b.lock_set(rows=False)
    assert only.rows is None and only.pos is None and np.array_equal(_np(only.count), ls["count"])
    # bit Y[s] of a valid slot is st_reachable's answer
    reach = _np(b.reachable(first=False).steps) > 0
    bit = ((ls["rows"] >> smp["Y"].astype(np.uint32)) & 1).astype(bool) & smp["valid"]
    assert np.array_equal(bit, reach)
    assert_same_state(before, b, "lock_set changed the state")
    check_mt_state(b, smp["ob"], "after lock_set")


@pytest.mark.parametrize("cases", crafted_groups(), ids=lambda cs: "lock%d" % cs[0][1].get("lock_delay", 0))
def test_lock_set_crafted_states(cases):
    b = crafted_batch(cases)
    got = b.lock_set(cap=32)
    rows, pos, count = _np(got.rows).view(np.uint32), _np(got.pos), _np(got.count)
    for i, case in enumerate(cases):
        lk = LR.crafted_locks(case)
        assert np.array_equal(rows[i], LR.rows_of(R.CW, b.n_slots, lk)), case[0]
        assert count[i] == len(lk) and np.array_equal(pos[i], pos_table(R.CW, [lk], 32)[0]), case[0]
    names = [c[0] for c in cases]
    if "spawn_in_stack" in names:  # the colliding start is no lock position
        assert count[names.index("spawn_in_stack")] == 0
    if "under_overhang" in names:  # the tuck under the block, no slot's landing
        assert LR.lock_pos(R.CW, 0, 0, 8) in pos[names.index("under_overhang")]


# ------------------------------------------------------------------ 2. afterstates_at
@pytest.mark.parametrize("features", ["base", "bcts"])
@pytest.mark.parametrize("board,config", R.CASES)
def test_afterstates_at_every_lock_position(board, config, features):
    b, smp, _ = sample_batch(board, config)
    ls, ref = LR.sample(board, config), LR.sample_feat(board, config, features)
    W, S = b.width, b.n_slots
    cap = max(int(ls["count"].max()), 70)  # above 64: a second pass
    pos = pos_table(W, ls["locks"], cap)
    before = engine_state(b)
    got = b.afterstates_at(pos, features=features)
    feat, brd = _np(got.feat), _np(got.boards).view(np.uint32)
    nrows = 18 if features == "bcts" else 11
    assert feat.shape == (R.N, nrows, cap) and brd.shape == (R.N, W, cap)
    for e, lk in enumerate(ls["locks"]):
        for i, p in enumerate(sorted(lk, key=lambda q: LR.lock_pos(W, *q))):
            f, bw = ref[e][p]
            assert np.array_equal(feat[e, :, i], f), (e, p, feat[e, :, i], f)
            assert np.array_equal(brd[e, :, i], bw), (e, p, "board")
        assert not feat[e, :, len(lk):].any() and not brd[e, :, len(lk):].any(), (e, "the -1 entries")
    nob = b.afterstates_at(pos, boards=False, features=features)
    assert nob.boards is None and np.array_equal(_np(nob.feat), feat)
    # at every slot's landing: st_afterstates_set's rows and board, bit for bit (S = 68 on 11x12: two passes)
    land = np.where(smp["valid"], np.arange(S)[None] * 32 + smp["Y"], -1).astype(np.int32)
    at, whole = b.afterstates_at(land, features=features), b.afterstates(features=features)
    assert np.array_equal(_np(at.feat), _np(whole.feat)) and np.array_equal(_np(at.boards), _np(whole.boards))
    assert_same_state(before, b, "afterstates_at changed the state")


@pytest.mark.parametrize("features", ["base", "bcts"])
def test_afterstates_at_non_evaluable_entries(features):
    board, config = "11x12", "default"
    b, smp, kw = sample_batch(board, config)
    W, H, S = b.width, b.height, b.n_slots
    ref = LR.sample_feat(board, config, features)
    ob = smp["ob"]
    pos = np.full((R.N, 6), -1, np.int32)
    good = []
    for e in range(R.N):
        s = int(np.flatnonzero(smp["steps"][e] > 0)[0]) if (smp["steps"][e] > 0).any() else -1
        y = int(smp["Y"][e, s]) if s >= 0 else 0
        good.append(s >= 0)
        pos[e] = (s * 32 + y - 1 if s >= 0 and y > 0 else -1,   # floating: the row above a landing
                  s * 32 + y + 1 if s >= 0 else -1,             # colliding: the row below it
                  s * 32 + y if s >= 0 else -1,                 # evaluable
                  (e % S) * 32 + H + e % (32 - H),              # a row y >= H
                  (S + e) * 32 + 3,                             # a slot >= S
                  -1)
        bool_board = ob.board(e).astype(bool)
        for i in (0, 1, 3, 4, 5):
            assert not LR.evaluable(bool_board, ob.envs[e].shape_id, W, int(pos[e, i])), (e, i)
        assert s < 0 or LR.evaluable(bool_board, ob.envs[e].shape_id, W, int(pos[e, 2]))
    assert sum(good) >= R.N // 2
    got = b.afterstates_at(pos, features=features)
    feat, brd = _np(got.feat), _np(got.boards).view(np.uint32)
    for i in (0, 1, 3, 4, 5):
        assert not feat[:, :, i].any() and not brd[:, :, i].any(), i
    per = W + 6
    for e in np.flatnonzero(good):
        s = int(pos[e, 2]) >> 5
        f, bw = ref[e][(s // per, s % per - 3, int(pos[e, 2]) & 31)]
        assert np.array_equal(feat[e, :, 2], f) and np.array_equal(brd[e, :, 2], bw), e


# ------------------------------------------------------------------ 3. routes_at
@pytest.mark.parametrize("board,config", R.CASES)
def test_routes_at_every_lock_position_and_play_out(board, config):
    b, smp, kw = sample_batch(board, config)
    ls, gr = LR.sample(board, config), graphs(board, config)
    W, S, n = b.width, b.n_slots, R.N
    ob = smp["ob"]
    envs = range(ROUTE_ENVS)
    lists = [sorted(ls["locks"][e], key=lambda q: LR.lock_pos(W, *q)) for e in envs]
    rounds = max(len(l) for l in lists)
    torch = _torch()
    need = np.zeros(n, np.uint8)
    need[:ROUTE_ENVS] = 1
    route = torch.full((RR.ROUTE_WORDS, n), -5, dtype=torch.int64, device=b.device)
    steps = torch.full((n,), -5, dtype=torch.int32, device=b.device)
    before = engine_state(b)
    h, hf = R.helpers(kw)
    one = O.OracleBatch(1, [0], **kw)
    size = ctypes.sizeof(O.Env)
    ref_feat = LR.sample_feat(board, config, "base")
    for j in range(rounds + 1):
        # round j: env e's j-th lock position; behind a list's end, and in the last round, targets that cannot be served
        tg = np.full(n, -1, np.int32)
        exp = [[] for _ in range(n)]
        for e in envs:
            if j < len(lists[e]):
                tg[e] = LR.lock_pos(W, *lists[e][j])
                exp[e] = LR.route_to(gr[e], lists[e][j])
                assert len(exp[e]) == ls["locks"][e][lists[e][j]], "route_ref and reach_ref disagree"
            else:
                r, x, y = lists[e][0] if lists[e] else (0, 0, 1)
                tg[e] = (-1, S * 32 + 5, LR.lock_pos(W, r, x, y - 1) if y > 0 else -1)[(e + j) % 3]  # (floating: no lock)
                if tg[e] >= 0 and (tg[e] >> 5) < S:
                    assert LR.lock_rot_x_y(W, int(tg[e])) not in ls["locks"][e]
        rt = b.routes_at(tg, need=need, out=(route, steps))
        assert np.array_equal(_np(rt.steps)[:ROUTE_ENVS], [len(exp[e]) for e in envs]), j
        assert np.array_equal(got_words(rt)[:ROUTE_ENVS], route_words(exp[:ROUTE_ENVS])), j
        assert (_np(steps)[ROUTE_ENVS:] == -5).all() and (_np(route)[:, ROUTE_ENVS:] == -5).all()  # not needed
        for e in envs:  # the route locks exactly there on its last action and not before
            if not exp[e]:
                continue
            p = lists[e][j]
            ctypes.memmove(ctypes.addressof(one.envs[0]), ctypes.addressof(ob.envs[e]), size)
            hf.load(ob.board(e), ob.envs[e].shape_id)
            env = one.envs[0]
            for i, a in enumerate(exp[e]):
                where = hf.step(env.rot, env.ax, env.ay, 0, a)[:3]
                spawned = sum(env.counts)
                _, rew, done, _ = one.step_one(0, a)
                locked = sum(env.counts) != spawned or done
                assert locked == (i == len(exp[e]) - 1), (e, p, i)
            assert where == p, (e, p, where)
            f, bw = ref_feat[e][p]
            assert rew == f[PR.REWARD], (e, p)
            if not done:
                assert np.array_equal(pack_cols(one.board(0)), bw), (e, p)
    assert_same_state(before, b, "routes_at changed the state")


@pytest.mark.parametrize("cases", crafted_groups(), ids=lambda cs: "lock%d" % cs[0][1].get("lock_delay", 0))
def test_routes_at_crafted_states(cases):
    b = crafted_batch(cases)
    kw = dict(width=R.CW, height=R.CH, **cases[0][1])
    h, hf = R.helpers(kw)
    ers = [RR.EnvRoutes(h, hf, c[2], c[3], c[4], c[5], c[6], c[7]) for c in cases]
    lists = [sorted(LR.crafted_locks(c), key=lambda q: LR.lock_pos(R.CW, *q)) for c in cases]
    for j in range(max(len(l) for l in lists) + 1):
        tg = np.array([LR.lock_pos(R.CW, *l[j]) if j < len(l) else -1 for l in lists], np.int32)
        exp = [LR.route_to(er, l[j]) if j < len(l) else [] for er, l in zip(ers, lists)]
        rt = b.routes_at(tg)
        assert np.array_equal(_np(rt.steps), [len(r) for r in exp]), j
        assert np.array_equal(got_words(rt), route_words(exp)), j
    # the colliding start of spawn_in_stack locks where it stands: no lock position, not served
    names = [c[0] for c in cases]
    if "spawn_in_stack" in names:
        i = names.index("spawn_in_stack")
        tg = np.full(len(cases), -1, np.int32)
        tg[i] = LR.lock_pos(R.CW, 0, 3, 0)
        rt = b.routes_at(tg)
        assert _np(rt.steps)[i] == 0 and (got_words(rt)[i] == np.uint64(RR.NONE_WORD)).all()


# ------------------------------------------------------------------ 4. policy_locks
def weights3(features):
    G = engine()
    rows = 18 if features == "bcts" else 11
    first = G.engine.weight_rows(G.BCTS_WEIGHTS, "bcts")[0] if features == "bcts" else PR.GREEDY
    rnd = np.random.default_rng(2100).normal(size=rows).astype(np.float32)
    return np.stack([np.asarray(first, np.float32), LR.deep_row(rows), rnd])


def policy_ref(board, config, features, w):
    """pos, score, feat column, count, route of every env under weight rows w [n_w, rows]."""
    ls, ref, gr = LR.sample(board, config), LR.sample_feat(board, config, features), graphs(board, config)
    W = R.BOARDS[board][0]
    out = []
    for e, lk in enumerate(ls["locks"]):
        order = sorted(lk, key=lambda q: LR.lock_pos(W, *q))
        feats = np.stack([ref[e][p][0] for p in order], axis=1) if order else np.zeros((w.shape[1], 0), np.int32)
        i, sc = LR.choose(w[e % len(w)], feats)
        if i < 0:
            out.append((-1, np.float32(0), np.zeros(w.shape[1], np.int32), 0, []))
        else:
            out.append((LR.lock_pos(W, *order[i]), sc, feats[:, i], len(order), LR.route_to(gr[e], order[i])))
    return out


@pytest.mark.parametrize("board,config,features", [(b_, c_, "bcts") for b_, c_ in R.CASES] +
                         [("10x20", "default", "base"), ("6x9", "c4_lock3", "base")])
def test_policy_locks_is_the_numpy_chain(board, config, features):
    torch = _torch()
    b, smp, kw = sample_batch(board, config)
    n = R.N
    w = weights3(features)
    want = policy_ref(board, config, features, w)
    wt = torch.as_tensor(w, device=b.device)
    before = engine_state(b)
    ch = b.policy_locks(wt, features=features)
    assert np.array_equal(_np(ch.pos), [x[0] for x in want]), np.flatnonzero(_np(ch.pos) != [x[0] for x in want])[:8]
    assert np.array_equal(_np(ch.scores).view(np.uint32), np.array([x[1] for x in want], np.float32).view(np.uint32))
    assert np.array_equal(_np(ch.feat), np.stack([x[2] for x in want], axis=1))
    assert np.array_equal(_np(ch.count), [x[3] for x in want])
    assert np.array_equal(_np(ch.routes.steps), [len(x[4]) for x in want])
    assert np.array_equal(got_words(ch.routes), route_words([x[4] for x in want]))
    assert np.array_equal(_np(ch.y), _np(ch.feat)[PR.Y])  # rows by name
    # the need mask leaves the other envs' words alone
    need = (np.arange(n) % 3 != 1)
    outs = (torch.full((n,), -9, dtype=torch.int32, device=b.device),
            torch.full((RR.ROUTE_WORDS, n), -9, dtype=torch.int64, device=b.device),
            torch.full((n,), -9, dtype=torch.int32, device=b.device),
            torch.full((n,), -9.0, dtype=torch.float32, device=b.device),
            torch.full((w.shape[1], n), -9, dtype=torch.int32, device=b.device),
            torch.full((n,), -9, dtype=torch.int32, device=b.device))
    b.policy_locks(wt, features=features, need=need, out=outs)
    for t, full in zip(outs, (ch.pos, ch.routes.route, ch.routes.steps, ch.scores, ch.feat, ch.count)):
        g, f = _np(t), _np(full)
        assert np.array_equal(g[..., need], f[..., need]) and (g[..., ~need] == -9).all()
    # without d_route: the same choice, no search
    from gym_simpletetris_amd import _lib as C
    pos2 = torch.full((n,), -9, dtype=torch.int32, device=b.device)
    C.check(C.load().st_policy_locks(b._ctx, C.FEATURE_SETS[features], ctypes.c_void_p(wt.data_ptr()), 3, None,
                                     ctypes.c_void_p(pos2.data_ptr()), None, None, None, None, None, b._stream()))
    assert np.array_equal(_np(pos2), _np(ch.pos))
    # the deep row alone: some env's best lock position is no slot's landing, so policy_routed chooses otherwise
    if board != "6x9":
        deep = torch.as_tensor(w[1:2], device=b.device)
        lk, rt = b.policy_locks(deep, features=features), b.policy_routed(deep, features=features)
        differ = (_np(lk.pos) >> 5 != _np(rt.slots)) | (_np(lk.y) != smp["Y"][np.arange(n), np.clip(_np(rt.slots), 0, None)])
        assert differ.sum() >= 1
        assert (_np(lk.scores) >= _np(rt.scores)).all()  # the slot landings are among the lock positions
    assert_same_state(before, b, "policy_locks changed the state")


# ------------------------------------------------------------------ 5. play_locks
def by_hand(b, wt, features, k, returns, episodes, pieces, log=None):
    """The header's loop: policy_locks for the envs whose plan ran out, the
    route's next action, step.  log: a list that receives each step's
    (actions, obs, reward, done, whether the env played a route's action)."""
    torch = _torch()
    n = b.n
    rows = 18 if features == "bcts" else 11
    rem = torch.zeros(n, dtype=torch.int32, device=b.device)
    outs = (torch.full((n,), -1, dtype=torch.int32, device=b.device),
            torch.full((RR.ROUTE_WORDS, n), RR.NONE_WORD, dtype=torch.int64, device=b.device),
            torch.zeros(n, dtype=torch.int32, device=b.device), torch.zeros(n, dtype=torch.float32, device=b.device),
            torch.zeros((rows, n), dtype=torch.int32, device=b.device), torch.zeros(n, dtype=torch.int32, device=b.device))
    route, steps = outs[1], outs[2]
    out = None
    for _ in range(k):
        need = rem == 0
        b.policy_locks(wt, features=features, need=need, out=outs)
        length = steps.clamp(max=RR.ROUTE_MAX)
        rem = torch.where(need, length, rem)
        i = (length - rem).clamp(min=0).to(torch.int64)
        word = torch.where(i >= 21, route[1], route[0])
        a = torch.where(rem > 0, (word >> (3 * (i % 21))) & 7, torch.full_like(word, 2)).to(torch.uint8)
        pieces += ((rem == 1) & (steps <= RR.ROUTE_MAX)).to(torch.int32)
        had = _np(rem > 0)
        rem = (rem - 1).clamp(min=0)
        out = b.step(a, obs="packed")
        returns += out[1].to(torch.int64)
        episodes += out[2].to(torch.int32)
        if log is not None:
            log.append((_np(a).copy(), out[0].clone(), _np(out[1]).copy(), _np(out[2]).copy(), had))
    return out


@pytest.mark.parametrize("autoreset", PR.AUTORESETS)
@pytest.mark.parametrize("board,config,features", [("10x20", "default", "bcts"), ("6x9", "c4_lock3", "base")])
def test_play_locks_equals_the_loop_by_hand_and_the_oracle(board, config, features, autoreset):
    torch = _torch()
    b, smp, kw = sample_batch(board, config, autoreset)
    twin, _, _ = sample_batch(board, config, autoreset)
    n, K = R.N, 3 * kw["height"]
    wt = torch.as_tensor(weights3(features), device=b.device)
    ret, eps, pcs = b.play_locks(wt, K, features=features)
    t_ret = torch.zeros(n, dtype=torch.int64, device=b.device)
    t_eps = torch.zeros(n, dtype=torch.int32, device=b.device)
    t_pcs = torch.zeros(n, dtype=torch.int32, device=b.device)
    log = []
    t_obs, t_rew, t_done = by_hand(twin, wt, features, K, t_ret, t_eps, t_pcs, log)
    assert np.array_equal(_np(b.obs), _np(t_obs)) and np.array_equal(_np(b.reward), _np(t_rew))
    assert np.array_equal(_np(b.done), _np(t_done))
    assert np.array_equal(_np(ret), _np(t_ret)) and np.array_equal(_np(eps), _np(t_eps))
    assert np.array_equal(_np(pcs), _np(t_pcs)), np.flatnonzero(_np(pcs) != _np(t_pcs))[:8]
    assert_same_state(engine_state(twin), b, "play_locks against the loop by hand")

    # the same plans replayed on the oracle, step by step; pieces counts the locks
    ob = clone_oracle(smp["ob"], kw)
    W = kw["width"]
    ref = dict(reward=np.zeros((K, n), np.int32), done=np.zeros((K, n), np.uint8), obs=np.zeros((K, n, W), np.uint32))
    locks = np.zeros(n, np.int32)
    for t, (acts, obs, rew, done, had) in enumerate(log):
        for e in range(n):
            spawned = ob.field("counts", (7,))[e].sum()
            o, ref["reward"][t, e], d, _ = ob.step_one(e, int(acts[e]))
            ref["obs"][t, e], ref["done"][t, e] = pack_cols(o), d
            locked = bool(ob.field("counts", (7,))[e].sum() != spawned or d)
            locks[e] += locked and bool(had[e])  # (an env without a lock position hard-drops without a plan)
            if d and autoreset == "same_step":
                ob.reset(e)
        check_step(ref, t, obs, rew, done)
    if autoreset == "same_step":  # (without it a dead env hard-drops on: locks that no route planned)
        assert np.array_equal(_np(pcs), locks), np.flatnonzero(_np(pcs) != locks)[:8]
    assert int(_np(pcs).sum()) >= n  # pieces were played

    # k = a then k = b equals k = a + b, with continued accumulators
    c, _, _ = sample_batch(board, config, autoreset)
    a_ = K // 3 + 1
    acc = c.play_locks(wt, a_, features=features)
    acc2 = c.play_locks(wt, K - a_, features=features, returns=acc[0], episodes=acc[1], pieces=acc[2])
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(acc, acc2))
    for got, want in zip(acc2, (ret, eps, pcs)):
        assert np.array_equal(_np(got), _np(want))
    assert np.array_equal(_np(c.obs), _np(b.obs)) and np.array_equal(_np(c.reward), _np(b.reward))
    assert_same_state(engine_state(b), c, "play_locks(a) + play_locks(b)")
    assert c.play_locks(wt, 0, features=features, returns=acc[0])[0] is acc[0]  # k = 0 does nothing
    assert_same_state(engine_state(b), c, "play_locks(0)")


# ------------------------------------------------------------------ 6. errors
def test_errors_change_nothing():
    from gym_simpletetris_amd import _lib as C
    torch = _torch()
    L = C.load()
    G = engine()
    n = 8
    b = G.TetrisBatch(n, seeds=list(range(n)), width=6, height=9, lock_delay=4)
    b.reset()
    before = engine_state(b)
    S = b.n_slots
    w = torch.zeros((1, 11), dtype=torch.float32, device=b.device)
    pos = np.zeros(n, np.int32)
    for call in (lambda: b.lock_set(cap=4), lambda: b.afterstates_at(pos[:, None]), lambda: b.routes_at(pos),
                 lambda: b.policy_locks(w), lambda: b.play_locks(w, 3)):
        with pytest.raises(C.StError) as ei:
            call()
        assert ei.value.code == C.ST_EINVAL and "lock_delay" in str(ei.value)
    assert_same_state(before, b, "a refused call changed the state")
    with pytest.raises(ValueError):
        b.lock_set(cap=0)
    with pytest.raises(ValueError):
        b.afterstates_at(pos)  # [n], not [n, cap]
    with pytest.raises(ValueError):
        b.routes_at(pos[:, None])

    b3 = G.TetrisBatch(n, seeds=list(range(n)), width=6, height=9, lock_delay=3)  # the largest lock_delay served
    b3.reset()
    assert int(b3.lock_set().count.sum()) > 0

    cfg = C.Config(6, 9, 0, 0, 0)
    ctx = ctypes.c_void_p()
    assert L.st_create(ctypes.byref(ctx), ctypes.byref(cfg), torch.device(b.device).index or 0, n) == C.ST_OK
    try:
        rows = torch.full((n, S), -9, dtype=torch.int32, device=b.device)
        lst = torch.full((n, 4), -9, dtype=torch.int32, device=b.device)
        cnt = torch.full((n,), -9, dtype=torch.int32, device=b.device)
        feat = torch.full((n, 11, 4), -9, dtype=torch.int32, device=b.device)
        route = torch.full((2, n), -9, dtype=torch.int64, device=b.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        calls = {
            "st_lock_set": lambda c: L.st_lock_set(c, p(rows), p(lst), 4, p(cnt), None),
            "st_afterstates_at": lambda c: L.st_afterstates_at(c, 0, p(lst), 4, p(feat), None, None),
            "st_routes_at": lambda c: L.st_routes_at(c, p(cnt), None, p(route), None, None),
            "st_policy_locks": lambda c: L.st_policy_locks(c, 0, p(w), 1, None, p(cnt), p(route), None, None, None,
                                                           None, None),
            "st_play_locks": lambda c: L.st_play_locks(c, 0, p(w), 1, 2, None, None, None, None, None, None, None),
        }
        for name, call in calls.items():  # before seed
            assert call(ctx) == C.ST_ESTATE and name.encode() in L.st_last_error(), name
        seeds = np.arange(n, dtype=np.uint64)
        assert L.st_seed(ctx, ctypes.c_void_p(seeds.ctypes.data), None) == C.ST_OK
        for name, call in calls.items():  # before reset
            assert call(ctx) == C.ST_ESTATE, name
        assert L.st_reset(ctx, None, None) == C.ST_OK
        for name, call in calls.items():
            assert call(None) == C.ST_EINVAL and name.encode() in L.st_last_error(), name
        assert L.st_lock_set(ctx, None, None, 4, None, None) == C.ST_EINVAL       # not all three may be NULL
        assert L.st_lock_set(ctx, p(rows), p(lst), 0, p(cnt), None) == C.ST_EINVAL  # cap >= 1 with a list
        assert L.st_afterstates_at(ctx, 0, None, 4, p(feat), None, None) == C.ST_EINVAL
        assert L.st_afterstates_at(ctx, 0, p(lst), 4, None, None, None) == C.ST_EINVAL
        assert L.st_afterstates_at(ctx, 0, p(lst), 0, p(feat), None, None) == C.ST_EINVAL
        assert L.st_afterstates_at(ctx, 7, p(lst), 4, p(feat), None, None) == C.ST_EINVAL
        assert L.st_routes_at(ctx, None, None, p(route), None, None) == C.ST_EINVAL
        assert L.st_routes_at(ctx, p(cnt), None, None, None, None) == C.ST_EINVAL
        assert L.st_policy_locks(ctx, 0, None, 1, None, p(cnt), p(route), None, None, None, None, None) == C.ST_EINVAL
        assert L.st_policy_locks(ctx, 0, p(w), 1, None, None, p(route), None, None, None, None, None) == C.ST_EINVAL
        assert L.st_policy_locks(ctx, 7, p(w), 1, None, p(cnt), p(route), None, None, None, None, None) == C.ST_EINVAL
        assert L.st_policy_locks(ctx, 0, p(w), 0, None, p(cnt), p(route), None, None, None, None, None) == C.ST_EINVAL
        assert L.st_play_locks(ctx, 0, None, 1, 2, None, None, None, None, None, None, None) == C.ST_EINVAL
        assert L.st_play_locks(ctx, 7, p(w), 1, 2, None, None, None, None, None, None, None) == C.ST_EINVAL
        assert L.st_play_locks(ctx, 0, p(w), 0, 2, None, None, None, None, None, None, None) == C.ST_EINVAL
        assert L.st_play_locks(ctx, 0, p(w), 1, 0, None, None, None, None, None, None, None) == C.ST_OK  # k <= 0
        torch.cuda.synchronize()
        for t in (rows, lst, cnt, feat, route):
            assert (_np(t) == -9).all()
    finally:
        assert L.st_destroy(ctx) == C.ST_OK
