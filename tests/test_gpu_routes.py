"""st_routes / st_policy_routed / st_play_routed (TetrisBatch.routes,
.policy_routed, .play_routed) against route_ref: whole routes of every env of
three samples, played out step by step beside the oracle; the need mask;
crafted states; the fused choice against the three calls it replaces; the
player against a twin driven by hand with the older calls and against the
oracle loop; the grid's tail with guard regions; the error paths."""
import ctypes

import numpy as np
import pytest

import feature_ref as FR
import placement_ref as PR
import reach_ref as R
import route_ref as RR
from harness import (assert_same_state, cached_ref, check_mt_state, engine, engine_state, pack_cols, words)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CASES = [("10x20", "default"), ("6x9", "lock2"), ("11x12", "c4_lock3")]
K = 40


def _torch():
    import torch
    return torch


def _np(t):
    return t.cpu().numpy()


def load_oracle(b, ob, idx=None, mt=True):
    """Every env's state of an OracleBatch (envs idx of it) into the batch."""
    idx = np.arange(ob.n) if idx is None else np.asarray(idx)
    ps = ob.packed_state()
    st = b.get_state(("board", "piece", "stats", "mt") if mt else ("board", "piece", "stats"))
    st["board"][:] = ps["board"][:, idx]
    st["piece"][:] = ps["piece"][idx]
    st["stats"][:13] = ps["stats"][:, idx]
    if mt:
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
    """[n, ROUTE_WORDS] uint64 of a list of action lists."""
    return np.array([RR.pack(r) for r in routes], np.uint64).reshape(len(routes), RR.ROUTE_WORDS)


def got_words(rt):
    return _np(rt.route).view(np.uint64).T


def mixed_targets(smp, S, seed=77):
    """test_routes_lock_the_piece_in_the_slot's mix: reachable, valid but
    unreachable, invalid, -1, S."""
    rng = np.random.default_rng(seed)
    steps0, valid = smp["steps"], smp["valid"]
    tg = np.empty(R.N, np.int32)
    for e in range(R.N):
        pools = [np.flatnonzero(steps0[e] > 0), np.flatnonzero(valid[e] & (steps0[e] == 0)), np.flatnonzero(~valid[e])]
        kind = e % 5
        tg[e] = -1 if kind == 3 else S if kind == 4 else (rng.choice(pools[kind]) if len(pools[kind]) else -1)
    return tg


def check_routes(rt, exp, what=""):
    """A Routes against a list of action lists: words, steps, action(i), length."""
    n = len(exp)
    ew = route_words(exp)
    gw = got_words(rt)
    lens = np.array([len(r) for r in exp], np.int32)
    assert np.array_equal(_np(rt.steps), lens), (what, "steps", np.flatnonzero(_np(rt.steps) != lens)[:8])
    assert np.array_equal(gw, ew), (what, "route", np.flatnonzero((gw != ew).any(axis=1))[:8])
    assert np.array_equal(_np(rt.length), np.minimum(lens, RR.ROUTE_MAX))
    for i in (0, 1, 20, 21, RR.ROUTE_MAX - 1):
        f = np.array([r[i] if i < len(r) else 7 for r in exp], np.uint8)
        a = rt.action(i)
        assert a.dtype == _torch().uint8 and np.array_equal(_np(a), f), (what, "action", i)
    assert n == gw.shape[0]


# ------------------------------------------------------------------ 1. routes
@pytest.mark.parametrize("board,config", CASES)
def test_routes_equal_route_ref_and_play_out(board, config):
    torch = _torch()
    b, smp, kw = sample_batch(board, config)
    ob = clone_oracle(smp["ob"], kw)
    n, S, W = R.N, b.n_slots, b.width
    tg = mixed_targets(smp, S)
    live = np.array([0 <= tg[e] < S and smp["steps"][e, tg[e]] > 0 for e in range(n)])
    assert live.sum() >= 10 and (~live).sum() >= 40
    exp = [graphs(board, config)[e].route(int(tg[e])) for e in range(n)]
    assert all((len(exp[e]) > 0) == live[e] for e in range(n))
    before = engine_state(b)
    rt = b.routes(tg)
    check_routes(rt, exp, "routes")
    assert_same_state(before, b, "routes changed the state")
    check_mt_state(b, smp["ob"], "after routes")

    # the route played through step(), beside the oracle
    after = b.afterstates(boards=True)
    a_rew, a_brd = _np(after.reward), _np(after.boards).view(np.uint32)
    lens = _np(rt.steps).copy()
    for k in range(int(lens.max())):
        fld = _np(rt.action(k))
        assert np.array_equal(fld == 7, k >= lens), ("fields past a route's end hold 7", k)
        acts = np.where(fld == 7, 6, fld).astype(np.uint8)  # a finished or unserved env idles
        spawned = ob.field("counts", (7,)).sum(axis=1).copy()
        obs, rew, done = b.step(torch.as_tensor(acts, device=b.device), obs="packed")
        exp_obs, exp_rew, exp_done = np.empty((n, W), np.uint32), np.empty(n, np.int32), np.empty(n, np.uint8)
        for e in range(n):
            o, exp_rew[e], d, _ = ob.step_one(e, int(acts[e]))
            exp_obs[e], exp_done[e] = pack_cols(o), d
        locked = (ob.field("counts", (7,)).sum(axis=1) != spawned) | (exp_done != 0)
        assert np.array_equal(_np(rew), exp_rew), ("reward", k)
        assert np.array_equal(_np(done).astype(np.uint8), exp_done), ("done", k)
        assert np.array_equal(words(obs), exp_obs), ("obs", k)
        now = lens == k + 1
        assert locked[now].all() and not locked[lens > k + 1].any(), ("a route locks on exactly step n", k)
        board_now = b.get_state(("board",))["board"]
        for e in np.flatnonzero(now):
            assert exp_rew[e] == a_rew[e, tg[e]], ("the slot's REWARD", e, k)
            if not exp_done[e]:
                assert np.array_equal(board_now[:, e], a_brd[e, :, tg[e]]), ("the slot's afterstate board", e, k)
        for e in np.flatnonzero(exp_done):
            ob.reset(e)  # same_step: the engine reset it inside the step


# ------------------------------------------------------------------ 2. the need mask
def test_need_mask_leaves_other_envs_untouched():
    torch = _torch()
    board, config = "11x12", "c4_lock3"
    b, smp, _ = sample_batch(board, config)
    n, S = R.N, b.n_slots
    tg = np.array([int(np.argmax(smp["steps"][e])) for e in range(n)], np.int32)  # the farthest slot
    exp = [graphs(board, config)[e].route(int(tg[e])) for e in range(n)]
    need = (np.arange(n) % 3 != 1)
    GUARD = -0x0123456789ABCDEF
    route = torch.full((RR.ROUTE_WORDS, n), GUARD, dtype=torch.int64, device=b.device)
    steps = torch.full((n,), -9, dtype=torch.int32, device=b.device)
    for mask in (torch.as_tensor(need, device=b.device), need.astype(np.uint8)):
        route.fill_(GUARD)
        steps.fill_(-9)
        rt = b.routes(tg, need=mask, out=(route, steps))
        assert rt.route.data_ptr() == route.data_ptr() and rt.steps.data_ptr() == steps.data_ptr()
        gw, gs = got_words(rt), _np(steps)
        assert (gw[~need] == np.uint64(GUARD & (2 ** 64 - 1))).all() and (gs[~need] == -9).all(), "not needed: untouched"
        assert np.array_equal(gw[need], route_words(exp)[need]) and np.array_equal(gs[need], [len(exp[e]) for e in np.flatnonzero(need)])
    # policy_routed honours it too
    w = PR.GREEDY
    sl = torch.full((n,), -9, dtype=torch.int32, device=b.device)
    sc = torch.full((n,), -9.0, dtype=torch.float32, device=b.device)
    route.fill_(GUARD)
    steps.fill_(-9)
    full = b.policy_routed(w)
    ch = b.policy_routed(w, need=need, out=(sl, route, steps, sc))
    assert (_np(sl)[~need] == -9).all() and (_np(sc)[~need] == -9.0).all() and (_np(steps)[~need] == -9).all()
    assert (got_words(ch.routes)[~need] == np.uint64(GUARD & (2 ** 64 - 1))).all()
    for got, ref in ((sl, full.slots), (sc, full.scores), (steps, full.routes.steps)):
        assert np.array_equal(_np(got)[need], _np(ref)[need])
    assert np.array_equal(got_words(ch.routes)[need], got_words(full.routes)[need])


# ------------------------------------------------------------------ 3. crafted states
def _crafted_groups():
    groups = {}
    for case in R.CRAFTED:
        groups.setdefault(tuple(sorted(case[1].items())), []).append(case)
    return list(groups.values())


@pytest.mark.parametrize("cases", _crafted_groups(), ids=lambda cs: "lock%d" % cs[0][1].get("lock_delay", 0))
def test_crafted_states(cases):
    """Starts in mid-air, on (and inside) the stack, with a host-written lock
    counter at L, a piece id 7: the route to every slot, and to -1 and S."""
    n, cfg = len(cases), cases[0][1]
    kw = dict(width=R.CW, height=R.CH, **cfg)
    b = engine().TetrisBatch(n, seeds=list(range(40, 40 + n)), **kw)
    b.reset()
    st = b.get_state(("board", "piece"))
    for i, (_, _, board, sid, rot, x, y, l, _) in enumerate(cases):
        st["board"][:, i] = pack_cols(board)
        st["piece"][i] = sid | rot << 3 | x << 5 | y << 11 | l << 17
    b.set_state(**st)
    h, hf = R.helpers(kw)
    ers = [RR.EnvRoutes(h, hf, c[2], c[3], c[4], c[5], c[6], c[7]) for c in cases]
    served = 0
    for s in range(-1, b.n_slots + 1):
        exp = [er.route(s) for er in ers]
        check_routes(b.routes(np.full(n, s, np.int32)), exp, ("slot", s))
        served += sum(len(r) > 0 for r in exp)
    assert served >= 4 * n
    for i, case in enumerate(cases):
        if case[8] is not None:  # the answer worked out by hand: lengths and first actions
            for s, (steps, first) in case[8].items():
                r = ers[i].route(s)
                assert len(r) == steps and r[0] == first, (case[0], s)


# ------------------------------------------------------------------ 4. policy_routed
def covered_state():
    """6x9, lock_delay 3: the O piece rests on the floor under a full cover in
    row 5 with the lock counter at L.  It locks in one step, below the cover;
    every valid slot lands on the cover: no reachable candidate."""
    board = np.zeros((R.CW, R.CH), np.uint8)
    board[:, 5] = 1
    return board, R.O_ | 0 << 3 | 3 << 5 | 8 << 11 | 3 << 17


@pytest.mark.parametrize("features,rows", [("base", 1), ("base", 3), ("bcts", 1), ("bcts", 3)])
@pytest.mark.parametrize("board,config", [("10x20", "default"), ("6x9", "c4_lock3")])
def test_policy_routed_is_the_three_calls(board, config, features, rows):
    torch = _torch()
    G = engine()
    b, smp, kw = sample_batch(board, config)
    n = R.N
    if board == "6x9":
        st = b.get_state(("board", "piece"))
        cb, cp = covered_state()
        st["board"][:, 0], st["piece"][0] = pack_cols(cb), cp
        b.set_state(**st)
    rng = np.random.default_rng(31)
    if features == "base":
        w = np.stack([PR.GREEDY, PR.AGG_UP, rng.integers(-9, 10, PR.NF).astype(np.float32)])[:rows]
    else:
        w = np.stack([G.engine.weight_rows(G.BCTS_WEIGHTS, "bcts")[0], G.engine.weight_rows(G.DELLACHERIE_WEIGHTS, "bcts")[0],
                      rng.integers(-9, 10, FR.NF).astype(np.float32)])[:rows]
    wt = torch.as_tensor(w, device=b.device)
    before = engine_state(b)
    reach = b.reachable(first=False)
    lin = b.policy_linear(wt, features=features, allowed=reach.steps)
    ch = b.policy_routed(wt, features=features)
    slots, routes, scores = ch
    assert np.array_equal(_np(slots), _np(lin.slots)), np.flatnonzero(_np(slots) != _np(lin.slots))[:8]
    assert np.array_equal(_np(scores), _np(lin.scores))
    rt = b.routes(lin.slots)
    assert np.array_equal(got_words(routes), got_words(rt)) and np.array_equal(_np(routes.steps), _np(rt.steps))
    sl = _np(slots)
    assert np.array_equal(_np(routes.steps), np.where(sl >= 0, _np(reach.steps)[np.arange(n), np.clip(sl, 0, None)], 0))
    assert (sl >= 0).sum() >= n // 2
    if board == "6x9":
        assert _np(reach.steps)[0].max() == 0 and _np(b.afterstates(boards=False).valid)[0].any()
        assert sl[0] == -1 and _np(routes.steps)[0] == 0 and _np(scores)[0] == 0.0
        assert (got_words(routes)[0] == np.uint64(RR.NONE_WORD)).all()
    assert_same_state(before, b, "policy_routed changed the state")


# ------------------------------------------------------------------ 5. play_routed
def by_hand(b, wt, features, k, returns, episodes, pieces):
    """The header's loop with the older calls only: reachable, policy_linear,
    route_actions, step."""
    torch = _torch()
    n = b.n
    rem = torch.zeros(n, dtype=torch.int32, device=b.device)
    slot = torch.full((n,), -1, dtype=torch.int32, device=b.device)
    rs = torch.zeros(n, dtype=torch.int32, device=b.device)
    out = None
    for _ in range(k):
        need = rem == 0
        lin = b.policy_linear(wt, features=features, allowed=b.reachable(first=False).steps)
        slot = torch.where(need, lin.slots, slot)
        a = b.route_actions(slot, steps=rs).clone()
        rem = torch.where(need, rs.clamp(max=RR.ROUTE_MAX), rem)
        pieces += ((rem == 1) & (rs == 1)).to(torch.int32)  # the route's last action: the target is one step away
        rem = (rem - 1).clamp(min=0)
        out = b.step(a, obs="packed")
        returns += out[1].to(torch.int64)
        episodes += out[2].to(torch.int32)
    return out


def play_weights(G, features, device):
    torch = _torch()
    if features == "base":
        return torch.as_tensor(PR.THREE_ROWS, device=device)
    return torch.as_tensor(G.engine.weight_rows(G.BCTS_WEIGHTS, "bcts"), device=device)


@pytest.mark.parametrize("autoreset", PR.AUTORESETS)
@pytest.mark.parametrize("board,config,features", [("10x20", "default", "bcts"), ("6x9", "c4_lock3", "base")])
def test_play_routed_equals_the_loop_by_hand(board, config, features, autoreset):
    torch = _torch()
    b, _, _ = sample_batch(board, config, autoreset)
    twin, _, _ = sample_batch(board, config, autoreset)
    wt = play_weights(engine(), features, b.device)
    n = R.N
    ret, eps, pcs = b.play_routed(wt, K, features=features)
    t_ret = torch.zeros(n, dtype=torch.int64, device=b.device)
    t_eps = torch.zeros(n, dtype=torch.int32, device=b.device)
    t_pcs = torch.zeros(n, dtype=torch.int32, device=b.device)
    t_obs, t_rew, t_done = by_hand(twin, wt, features, K, t_ret, t_eps, t_pcs)
    assert np.array_equal(_np(b.obs), _np(t_obs)) and np.array_equal(_np(b.reward), _np(t_rew))
    assert np.array_equal(_np(b.done), _np(t_done))
    assert np.array_equal(_np(ret), _np(t_ret)) and np.array_equal(_np(eps), _np(t_eps))
    assert np.array_equal(_np(pcs), _np(t_pcs)), np.flatnonzero(_np(pcs) != _np(t_pcs))[:8]
    assert int(_np(pcs).sum()) >= n  # pieces were played
    assert_same_state(engine_state(twin), b, "play_routed against the loop by hand")

    # k = 15 then k = 25 equals k = 40, with continued accumulators
    c, _, _ = sample_batch(board, config, autoreset)
    acc = c.play_routed(wt, 15, features=features)
    acc2 = c.play_routed(wt, 25, features=features, returns=acc[0], episodes=acc[1], pieces=acc[2])
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(acc, acc2))
    for got, ref in zip(acc2, (ret, eps, pcs)):
        assert np.array_equal(_np(got), _np(ref))
    assert np.array_equal(_np(c.obs), _np(b.obs)) and np.array_equal(_np(c.reward), _np(b.reward))
    assert_same_state(engine_state(b), c, "play_routed(15) + play_routed(25)")
    assert c.play_routed(wt, 0, features=features, returns=acc[0])[0] is acc[0]  # k = 0 does nothing
    assert_same_state(engine_state(b), c, "play_routed(0)")


@pytest.mark.parametrize("autoreset", PR.AUTORESETS)
def test_play_routed_equals_the_oracle_loop(autoreset):
    board, config = "6x9", "lock2"
    b, smp, kw = sample_batch(board, config, autoreset)
    one, _, _ = sample_batch(board, config, autoreset)
    ref = RR.play_routed(clone_oracle(smp["ob"], kw), kw, PR.THREE_ROWS, K, "base", autoreset)
    wt = play_weights(engine(), "base", b.device)
    # one step a call: every step's reward / done (and k = 1 forty times is k = 40)
    acc = None
    for t in range(K):
        acc = one.play_routed(wt, 1, returns=acc and acc[0], episodes=acc and acc[1], pieces=acc and acc[2], obs="none")
        assert np.array_equal(_np(one.reward), ref["reward"][t]), ("reward", t)
        assert np.array_equal(_np(one.done).astype(np.uint8), ref["done"][t]), ("done", t)
    ret, eps, pcs = b.play_routed(wt, K)
    assert np.array_equal(_np(ret), ref["reward"].sum(axis=0)) and np.array_equal(_np(eps), ref["done"].sum(axis=0))
    assert np.array_equal(_np(pcs), ref["pieces"]) and (ref["pieces"] > 0).sum() >= R.N // 2
    for got, want in zip(acc, (ret, eps, pcs)):
        assert np.array_equal(_np(got), _np(want))
    assert_same_state(engine_state(one), b, "forty calls of one step")
    for e, t, slot, where, landing in ref["planned"]:  # every piece locked in the slot that was planned
        assert where == landing, (e, t, slot)


# ------------------------------------------------------------------ 6. grid and tails
def test_large_grid_and_out_buffers():
    torch = _torch()
    board, config, n, G = "10x20", "c4_lock3", 4099, 64
    kw = R.case_kw(board, config)
    smp = R.sample(board, config)
    b = engine().TetrisBatch(n, seeds=list(range(n)), **kw)
    b.reset()
    idx = np.arange(n) % R.N
    load_oracle(b, smp["ob"], idx, mt=False)
    S = b.n_slots
    before = engine_state(b)
    gr = graphs(board, config)
    tg = ((7 * np.arange(n)) % (S + 2) - 1).astype(np.int32)  # -1 and S occur
    memo = {}

    def route_of(i, s):
        if (i, s) not in memo:
            memo[(i, s)] = gr[i].route(s)
        return memo[(i, s)]

    exp = [route_of(int(idx[e]), int(tg[e])) for e in range(n)]
    GUARD = 0x5A5A5A5A5A5A5A5A
    rbuf = torch.full((RR.ROUTE_WORDS * n + G,), GUARD, dtype=torch.int64, device=b.device)
    sbuf = torch.full((n + G,), -9, dtype=torch.int32, device=b.device)
    out = (rbuf[:RR.ROUTE_WORDS * n].view(RR.ROUTE_WORDS, n), sbuf[:n])
    rt = b.routes(tg, out=out)
    assert rt.route.data_ptr() == rbuf.data_ptr() and rt.steps.data_ptr() == sbuf.data_ptr()
    check_routes(rt, exp, "the large grid")
    assert (_np(rbuf[RR.ROUTE_WORDS * n:]) == GUARD).all() and (_np(sbuf[n:]) == -9).all()
    # policy_routed: every output with a guard region behind it
    lbuf = torch.full((n + G,), -9, dtype=torch.int32, device=b.device)
    cbuf = torch.full((n + G,), -9.0, dtype=torch.float32, device=b.device)
    rbuf.fill_(GUARD)
    sbuf.fill_(-9)
    w = torch.as_tensor(PR.THREE_ROWS, device=b.device)
    ch = b.policy_routed(w, out=(lbuf[:n], out[0], out[1], cbuf[:n]))
    lin = b.policy_linear(w, allowed=b.reachable(first=False).steps)
    assert np.array_equal(_np(ch.slots), _np(lin.slots)) and np.array_equal(_np(ch.scores), _np(lin.scores))
    sl = _np(lin.slots)
    check_routes(ch.routes, [route_of(int(idx[e]), int(sl[e])) for e in range(n)], "policy_routed on the large grid")
    for buf, g in ((rbuf[RR.ROUTE_WORDS * n:], GUARD), (sbuf[n:], -9), (lbuf[n:], -9), (cbuf[n:], -9.0)):
        assert (_np(buf) == g).all()
    assert_same_state(before, b, "the large grid changed the state")
    # play_routed: the accumulators' tails; the first 70 envs against a 70-env batch of the same seeds and state
    abuf = [torch.full((n + G,), 0, dtype=dt, device=b.device) for dt in (torch.int64, torch.int32, torch.int32)]
    for t in abuf:
        t[n:] = -9
    ret, eps, pcs = b.play_routed(w, 3, returns=abuf[0][:n], episodes=abuf[1][:n], pieces=abuf[2][:n])
    assert all((_np(t[n:]) == -9).all() for t in abuf)
    small = engine().TetrisBatch(R.N, seeds=list(range(R.N)), **kw)
    small.reset()
    load_oracle(small, smp["ob"], mt=False)
    r70 = small.play_routed(w, 3)
    for got, want in zip((ret, eps, pcs), r70):
        assert np.array_equal(_np(got)[:R.N], _np(want))
    assert int(_np(pcs)[R.N:].sum()) > 0 and np.array_equal(_np(b.reward)[:R.N], _np(small.reward))


# ------------------------------------------------------------------ 6b. the widest board, the most planes
def test_widest_board_and_lock_delay_3():
    """32x28 with lock_delay 3: 152 slots (three slots a lane), four planes, the
    largest LDS request; routes of about twenty steps."""
    from harness import ASEED
    torch = _torch()
    kw = dict(width=32, height=28, lock_delay=3, step_reset=True)
    n = 3
    seeds = [7700 + e for e in range(n)]
    ob = O.OracleBatch(n, seeds, **kw)
    ob.reset()
    acts = O.splitmix64_actions(ASEED, 0, 400, n)
    for e in range(n):
        for t in range(150 + 100 * e):
            if ob.step_one(e, int(acts[t, e]))[2]:
                ob.reset(e)
    b = engine().TetrisBatch(n, seeds=seeds, **kw)
    b.reset()
    load_oracle(b, ob)
    h, hf = R.helpers(kw)
    ers = [RR.env_routes(h, hf, ob, e) for e in range(n)]
    steps = np.stack([er.steps() for er in ers])
    assert np.array_equal(_np(b.reachable(first=False).steps), steps)
    assert steps.max() >= 15
    S = b.n_slots
    for tg in (steps.argmax(axis=1), np.array([np.flatnonzero(steps[e])[0] for e in range(n)]),
               np.array([np.flatnonzero(steps[e])[-1] for e in range(n)]), np.full(n, S - 1), np.full(n, S)):
        tg = tg.astype(np.int32)
        check_routes(b.routes(tg), [ers[e].route(int(tg[e])) for e in range(n)], ("32x28", tg.tolist()))
    w = torch.as_tensor(PR.THREE_ROWS, device=b.device)
    ch = b.policy_routed(w)
    lin = b.policy_linear(w, allowed=b.reachable(first=False).steps)
    assert np.array_equal(_np(ch.slots), _np(lin.slots)) and np.array_equal(_np(ch.scores), _np(lin.scores))
    check_routes(ch.routes, [ers[e].route(int(_np(lin.slots)[e])) for e in range(n)], "32x28 policy_routed")


# ------------------------------------------------------------------ 7. errors
def test_errors_change_nothing():
    from gym_simpletetris_amd import _lib as C
    torch = _torch()
    L = C.load()
    G = engine()
    n = 8
    b = G.TetrisBatch(n, seeds=list(range(n)), width=6, height=9, lock_delay=4)
    b.reset()
    before = engine_state(b)
    GUARD = 0x1111111111111111
    route = torch.full((RR.ROUTE_WORDS, n), GUARD, dtype=torch.int64, device=b.device)
    steps = torch.full((n,), -9, dtype=torch.int32, device=b.device)
    slots = torch.full((n,), -9, dtype=torch.int32, device=b.device)
    scores = torch.full((n,), -9.0, dtype=torch.float32, device=b.device)
    ret = torch.full((n,), -9, dtype=torch.int64, device=b.device)
    pcs = torch.full((n,), -9, dtype=torch.int32, device=b.device)

    def untouched():
        torch.cuda.synchronize()
        assert (_np(route) == GUARD).all() and (_np(steps) == -9).all() and (_np(slots) == -9).all()
        assert (_np(scores) == -9.0).all() and (_np(ret) == -9).all() and (_np(pcs) == -9).all()

    for call in (lambda: b.routes(np.zeros(n, np.int32), out=(route, steps)),
                 lambda: b.policy_routed(PR.GREEDY, out=(slots, route, steps, scores)),
                 lambda: b.play_routed(PR.GREEDY, 3, returns=ret, pieces=pcs)):
        with pytest.raises(C.StError) as ei:
            call()
        assert ei.value.code == C.ST_EINVAL and "lock_delay" in str(ei.value)
    untouched()
    assert_same_state(before, b, "a refused call changed the state")

    cfg = C.Config(6, 9, 0, 0, 0)
    ctx = ctypes.c_void_p()
    assert L.st_create(ctypes.byref(ctx), ctypes.byref(cfg), torch.device(b.device).index or 0, n) == C.ST_OK
    try:
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        tg = torch.zeros(n, dtype=torch.int32, device=b.device)
        w = torch.as_tensor(PR.GREEDY[None], device=b.device)
        wb = torch.zeros((1, FR.NF), dtype=torch.float32, device=b.device)

        def all_three(code):
            assert L.st_routes(ctx, p(tg), None, p(route), p(steps), None) == code
            assert b"st_routes" in L.st_last_error()
            assert L.st_policy_routed(ctx, 0, p(w), 1, None, p(slots), p(route), p(steps), p(scores), None) == code
            assert b"st_policy_routed" in L.st_last_error()
            assert L.st_play_routed(ctx, 1, p(wb), 1, 3, p(ret), None, p(pcs), None, None, None, None) == code
            assert b"st_play_routed" in L.st_last_error()

        all_three(C.ST_ESTATE)  # before seed
        seeds = np.arange(n, dtype=np.uint64)
        assert L.st_seed(ctx, ctypes.c_void_p(seeds.ctypes.data), None) == C.ST_OK
        all_three(C.ST_ESTATE)  # before reset
        assert L.st_reset(ctx, None, None) == C.ST_OK
        E = C.ST_EINVAL
        assert L.st_routes(None, p(tg), None, p(route), p(steps), None) == E
        assert L.st_routes(ctx, None, None, p(route), p(steps), None) == E
        assert L.st_routes(ctx, p(tg), None, None, p(steps), None) == E
        assert L.st_policy_routed(None, 0, p(w), 1, None, p(slots), p(route), p(steps), p(scores), None) == E
        assert L.st_policy_routed(ctx, 0, None, 1, None, p(slots), p(route), p(steps), p(scores), None) == E
        assert L.st_policy_routed(ctx, 0, p(w), 1, None, None, p(route), p(steps), p(scores), None) == E
        assert L.st_policy_routed(ctx, 0, p(w), 1, None, p(slots), None, p(steps), p(scores), None) == E
        assert L.st_policy_routed(ctx, 2, p(w), 1, None, p(slots), p(route), p(steps), p(scores), None) == E
        assert L.st_policy_routed(ctx, 0, p(w), 0, None, p(slots), p(route), p(steps), p(scores), None) == E
        assert L.st_play_routed(None, 0, p(w), 1, 3, p(ret), None, p(pcs), None, None, None, None) == E
        assert L.st_play_routed(ctx, 0, None, 1, 3, p(ret), None, p(pcs), None, None, None, None) == E
        assert L.st_play_routed(ctx, -1, p(w), 1, 3, p(ret), None, p(pcs), None, None, None, None) == E
        assert L.st_play_routed(ctx, 0, p(w), 0, 3, p(ret), None, p(pcs), None, None, None, None) == E
        untouched()
        # the optional outputs may be NULL, and k <= 0 does nothing
        assert L.st_routes(ctx, p(tg), None, p(route), None, None) == C.ST_OK
        assert L.st_policy_routed(ctx, 0, p(w), 1, None, p(slots), p(route), None, None, None) == C.ST_OK
        assert L.st_play_routed(ctx, 0, p(w), 1, -1, p(ret), None, p(pcs), None, None, None, None) == C.ST_OK
        torch.cuda.synchronize()
        assert (_np(steps) == -9).all() and (_np(scores) == -9.0).all() and (_np(ret) == -9).all() and (_np(pcs) == -9).all()
        assert (_np(route) != GUARD).all() and (_np(slots) != -9).all()
    finally:
        assert L.st_destroy(ctx) == C.ST_OK
