"""Resets of LIVE envs -- what a training loop's time limit does every few
hundred steps -- on every reset surface, bit-exact against the reference's
own outputs (tests/golden/truncated.npz) and the C oracle.

TetrisEngine.clear() (tetris_env.py:306-315) leaves _lock_delay alone, so a
piece resting on the stack hands its lock counter to the next episode's first
piece; after a death the counter is always 0 (the lock has just fired), so
only a reset of a live env shows whether k_reset keeps it.  k_reset takes the
preview the step kernels drew one spawn ahead, or (none valid: after
st_mt_sync or a host-written state) draws the piece itself: both paths, in one
wave under a partial mask, at a generation's end and behind long rejection
runs; masks of any non-zero byte; and what every step surface makes of the
state a reset leaves."""
import functools
import random

import numpy as np
import pytest
import torch

from harness import (C4, HipAdapter, assert_same_state, batch_and_oracle, cached_ref, check_engine_state,
                     check_mt_state, check_step, check_steps, drive_surface, engine as _engine, pack_cols, raw_state,
                     record, set_mt_state, unpack_f32, untemper)
from oracle import oracle as O
from replay import load_set, replay_truncated

pytestmark = pytest.mark.gpu

TRUNCATED = load_set("truncated.npz")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device")


# ---------------------------------------------------------------- the reference's fixture
@pytest.mark.parametrize("sync", [True, False], ids=["sync", "nosync"])
@pytest.mark.parametrize("name", sorted(TRUNCATED))
def test_hip_truncated(name, sync):
    """Every field of every step, the state behind every reset and the render
    straight after it.  Synced reads give every preview back, so k_reset
    draws the new piece (need1); unsynced ones keep it, so k_reset consumes
    it."""
    meta, arrs = TRUNCATED[name]
    resets = replay_truncated(functools.partial(HipAdapter, sync=sync), name, meta, arrs)
    assert resets == int(arrs["reset"].sum())


SINGLE = ("lock2_reset_c4", "lock40_7x12")
INFO = ("time", "score", "lines_cleared", "holes", "deaths")
RTYPES = {0: int, 1: np.int64, 2: float, 3: np.float64}


@pytest.mark.parametrize("name", SINGLE)
@pytest.mark.parametrize("rng", ["private", "global"])
def test_single_env_truncated(name, rng):
    """TetrisEnv along env 0 of the fixture: reset(return_info=True) where
    the reference reset, its info against the recorded one."""
    G = _engine()
    meta, arrs = TRUNCATED[name]
    kw, seed = dict(meta["cfg"]), meta["seed_base"]
    H = kw.get("height", 20)
    env = G.TetrisEnv(rng=rng, seed=seed if rng == "private" else None, **kw)
    if rng == "global":
        random.seed(seed)
    assert not env.reset().any()
    resets = 0
    for t in range(arrs["actions"].shape[0]):
        o, r, d, info = env.step(int(arrs["actions"][t, 0]))
        assert np.array_equal(o, unpack_f32(arrs["obs"][t, 0], H)), t
        assert r == arrs["reward"][t, 0] and type(r) is RTYPES[int(arrs["rtype"][t, 0])], (t, r, type(r))
        assert d == bool(arrs["done"][t, 0]), t
        got = [info[k] for k in INFO] + list(info["statistics"].values()) + [info["current_piece"]]
        want = [arrs[k][t, 0] for k in ("time", "score", "lines", "holes", "deaths")] + list(arrs["counts"][t, 0]) \
            + [G.SHAPE_NAMES[int(arrs["piece"][t, 0]) & 7]]
        assert got == want, (t, got, want)
        if arrs["reset"][t, 0]:
            o0, rinfo = env.reset(return_info=True)
            assert o0.dtype == np.float32 and not o0.any()
            got = [rinfo[k] for k in INFO] + list(rinfo["statistics"].values()) + [rinfo["current_piece"]]
            want = [arrs["reset_" + k][t, 0] for k in INFO] + list(arrs["reset_counts"][t, 0]) \
                + [G.SHAPE_NAMES[int(arrs["reset_piece"][t, 0])]]
            assert got == want, (t, got, want)
            resets += 1
    assert resets == int(arrs["reset"][:, 0].sum()) > int(arrs["done"][:, 0].sum())
    env.close()


@pytest.mark.parametrize("name", SINGLE)
def test_tetris_engine_truncated(name):
    """TetrisEngine along env 0 of the fixture: clear() where the reference
    reset; behind each the lock counter the next episode inherits, render()
    at the spawn anchor and the one live shape_counts dict."""
    G = _engine()
    meta, arrs = TRUNCATED[name]
    kw = dict(meta["cfg"])
    W, H = kw.pop("width", 10), kw.pop("height", 20)
    eng = G.TetrisEngine(W, H, rng="private", seed=meta["seed_base"], **kw)
    counts = eng.shape_counts
    assert not eng.clear().any()
    inherited = 0
    for t in range(arrs["actions"].shape[0]):
        state, r, d = eng.step(int(arrs["actions"][t, 0]))
        assert np.array_equal(state, unpack_f32(arrs["obs"][t, 0], H)), t
        assert r == arrs["reward"][t, 0] and d == bool(arrs["done"][t, 0]), t
        assert (eng.time, eng.score, eng._lock_delay) == (arrs["time"][t, 0], arrs["score"][t, 0],
                                                         int(arrs["piece"][t, 0]) >> 17), t
        if arrs["reset"][t, 0]:
            assert not eng.clear().any()
            assert eng._lock_delay == int(arrs["after_piece"][t, 0]) >> 17, t
            assert np.array_equal(pack_cols(eng.render()), arrs["after_render"][t, 0]), t
            assert eng.shape_counts is counts and list(counts.values()) == list(arrs["after_counts"][t, 0]), t
            assert eng.time == arrs["after_time"][t, 0] == 0
            inherited += int(eng._lock_delay != 0)
    assert inherited >= 3  # env 0 alone hands a live counter over several times
    eng.close()


# ---------------------------------------------------------------- oracle-driven: the reset kernel and what follows
SCORING = dict(C4, reward_step=True)
SEED0, ACT_SEED, MASK_SEED = 4400, 0x7A11, 0x3A5C
N, T = 300, 120            # four full waves and a ragged fifth
ZEROS_AT, ALL_AT, WAVE1_AT, LAST_AT, VALUES_AT = 20, 40, 60, 80, 100


def _mask_rows(n, steps, p, only=None, special=True):
    """One mask per step: uint8 [n], or None (every env).  Bernoulli(p) rows
    from a fixed seed (only: the steps that keep theirs); `special` overwrites
    five steps with an all-zero mask, None, exactly wave 1, env n - 1 alone,
    and a mask whose non-zero bytes are 2 and 255."""
    rng = np.random.default_rng(MASK_SEED)
    rows = list((rng.random((steps, n)) < p).astype(np.uint8))
    if only is not None:
        rows = [r if t in only else np.zeros(n, np.uint8) for t, r in enumerate(rows)]
    if special:
        e = np.arange(n)
        rows[ZEROS_AT] = np.zeros(n, np.uint8)
        rows[ALL_AT] = None
        rows[WAVE1_AT] = ((e >= 64) & (e < 128)).astype(np.uint8)
        rows[LAST_AT] = (e == n - 1).astype(np.uint8)
        rows[VALUES_AT] = np.where(rng.random(n) < 0.25, np.where(e % 2, 255, 2), 0).astype(np.uint8)
        assert set(np.unique(rows[VALUES_AT])) == {0, 2, 255}
    return rows


def _actions(steps, n):
    """Uniform actions, every other step a hard drop: locks, resting pieces
    and deaths on every board within the run."""
    acts = O.splitmix64_actions(ACT_SEED, 0, steps, n)
    acts[1::2] = 2
    return acts


def _truncated_ref(n, steps, kw, rows):
    """The oracle through `steps` steps, the envs of rows[t] reset behind
    step t (OracleBatch.rollout has already reset the dead ones: an env that
    died and is truncated in the same step is cleared twice).  Coverage is
    counted here, on the oracle alone."""
    ob = O.OracleBatch(n, [SEED0 + e for e in range(n)], **kw)
    ob.reset()
    sel = [np.arange(n) if r is None else np.nonzero(r)[0] for r in rows]

    def after(t, locked, pre):
        for i in sel[t]:
            ob.reset(int(i))

    ref = record(ob, _actions(steps, n), after=after)
    hit = np.zeros((steps, n), bool)
    for t, s in enumerate(sel):
        hit[t, s] = True
    done = ref["done"].astype(bool)
    trunc, lock = hit & ~done, ref["stats"][..., 7]  # the lock counter behind the step, where no lock fired
    waves = [bool(trunc[:, w:w + 64].any()) for w in range(0, n, 64)]
    ref.update(rows=rows, ob=ob, state=ob.packed_state(),
               cover=dict(truncations=int(trunc.sum()), lock1=int((trunc & (lock == 1)).sum()),
                          lock2=int((trunc & (lock == 2)).sum()), locked=int((trunc & (lock != 0)).sum()),
                          twice=int((hit & done).sum()), waves=waves))
    return ref


def _board_kw(board):
    return dict(width=board[0], height=board[1], lock_delay=2, step_reset=True, **SCORING)


def _matrix_ref(board, k=1):
    """k = 1: the surface x board matrix's masks.  k > 1: truncations behind
    the last step of each chunk of k steps only, denser in proportion."""
    def make():
        if k == 1:
            rows = _mask_rows(N, T, 1 / 16)
        else:
            ends = set(range(k - 1, T, k)) | {T - 1}
            rows = _mask_rows(N, T, min(0.5, k / 16), only=ends, special=False)
        ref = _truncated_ref(N, T, _board_kw(board), rows)
        c = ref["cover"]
        assert c["lock1"] > 0 and c["lock2"] > 0 and c["twice"] > 0 and all(c["waves"]), (board, k, c)
        return ref
    return cached_ref(("truncation matrix", board, k), make)


def _reset(b, row, t=None):
    """reset(row) on the engine; an all-zero mask must change nothing at all:
    not the state, not the previews, not the MT buffers."""
    if row is None:
        b.reset()
    elif not row.any():
        before = raw_state(b)
        b.reset(torch.as_tensor(row.copy(), device=b.device))
        assert_same_state(before, raw_state(b), ("all-zero mask", t))
    else:
        b.reset(torch.as_tensor(row.copy(), device=b.device))


def _check_final(target, ref):
    check_engine_state(target, ref["state"])
    check_mt_state(target, ref["ob"])


MATRIX = [((10, 20), s) for s in ("step", "gated", "f32", "wire", "vec")] + \
    [(bd, "step") for bd in ((6, 9), (4, 4), (5, 27), (32, 28))]


@pytest.mark.parametrize("board,surface", MATRIX, ids=[f"{w}x{h}-{s}" for (w, h), s in MATRIX])
def test_truncation_surface_matrix(board, surface):
    """Every step surface continues from the state a reset of live envs
    leaves, 120 steps with random 1/16 masks and the five special ones."""
    G = _engine()
    ref = _matrix_ref(board)
    kw = _board_kw(board)
    if surface == "vec":
        target = G.TetrisVecEnv(N, seed=SEED0, obs_format="packed", **kw)
        target.reset()
    else:
        target = G.TetrisBatch(N, autoreset="same_step", seeds=[SEED0 + e for e in range(N)], **kw)
        target.reset()
    b = getattr(target, "engine", target)
    host = surface in ("step", "f32")
    try:
        drive_surface(target, ref, surface, ref["acts"] if host else torch.as_tensor(ref["acts"].copy(), device=b.device),
                      on_step=lambda t: _reset(b, ref["rows"][t], t))
        _check_final(target, ref)
    finally:
        target.close()


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("board,mode", [((10, 20), "packed"), ((10, 20), "f32"), ((9, 15), "packed"), ((9, 15), "f32"),
                                        ((10, 20), "step_n")],
                         ids=["10x20-packed", "10x20-f32", "9x15-packed", "9x15-f32", "10x20-step_n"])
def test_truncation_at_launch_boundaries(board, mode, k):
    """st_rollout (k_rollout at 10x20, the generic k_rollout2 at 9x15) and
    st_step_n in launches of k steps, a reset of live envs between launches."""
    G = _engine()
    ref = _matrix_ref(board, k)
    H = board[1]
    b = G.TetrisBatch(N, autoreset="same_step", seeds=[SEED0 + e for e in range(N)], **_board_kw(board))
    b.reset()
    acts = torch.as_tensor(ref["acts"].copy(), device=b.device)
    try:
        for t0 in range(0, T, k):
            t1 = min(t0 + k, T)
            if mode == "step_n":
                check_step(ref, t1 - 1, *b.step_n(acts[t0:t1], obs="packed"))
            else:
                check_steps(ref, *b.rollout(acts[t0:t1], obs=mode), t0=t0, H=H if mode == "f32" else None)
            assert all(not r.any() for r in ref["rows"][t0:t1 - 1])  # resets between launches only
            _reset(b, ref["rows"][t1 - 1], t1 - 1)
        _check_final(b, ref)
    finally:
        b.close()


# ---------------------------------------------------------------- k_reset's draw paths
def _hard_drops(steps, n, seed):
    acts = np.full((steps, n), 2, np.uint8)
    acts[::3] = O.splitmix64_actions(seed, 0, steps, n)[::3]
    return acts


def _oracle_reset(ob, mask):
    for i in np.nonzero(mask)[0]:
        ob.reset(int(i))


def _state_then_steps(b, ob, steps=40, seed=5):
    """The engine's state and MT state against the oracle's, then `steps`
    steps of mostly hard drops, then both again."""
    check_engine_state(b, ob.packed_state(), "behind the reset")
    check_mt_state(b, ob, "behind the reset")
    acts = _hard_drops(steps, b.n, seed)
    ref = ob.rollout(acts)
    for t in range(steps):
        check_step(ref, t, *b.step(torch.as_tensor(acts[t], device=b.device)))
    check_engine_state(b, ob.packed_state())
    check_mt_state(b, ob)


def test_reset_mixed_preview_and_draw_lanes():
    """Lanes of one wave that hold a preview beside lanes that do not, under
    a partial mask: get_state gives every preview back; a reset of the odd
    envs draws their pieces and leaves them previews; with no step between, a
    reset of every third env finds both kinds."""
    n = 128
    b, ob = batch_and_oracle(n, [SEED0 + e for e in range(n)])
    acts = _hard_drops(30, n, 7)
    ref = ob.rollout(acts)
    for t in range(30):
        check_step(ref, t, *b.step(torch.as_tensor(acts[t], device=b.device)))
    b.get_state()
    e = np.arange(n)
    for mask in ((e % 2 == 1), (e % 3 == 0)):
        b.reset(torch.as_tensor(mask.astype(np.uint8), device=b.device))
        _oracle_reset(ob, mask)
    pv = (raw_state(b)["stats"][13, :n].astype(np.uint32) >> 24) & 1
    assert np.array_equal(pv.astype(bool), (e % 2 == 1) | (e % 3 == 0))  # a preview exactly where an env was reset
    _state_then_steps(b, ob)
    b.close()


def test_reset_at_generation_edge_under_mask():
    """Host-written MT indices 620..624: the masked envs' draws cross the
    generation's end (at 624 they start behind it) while the unmasked lanes of
    the same wave keep exactly the words and index that were written."""
    n = 128
    b, ob = batch_and_oracle(n, [SEED0 + e for e in range(n)])
    st = b.get_state(("mt", "stats"))
    mt, stats = st["mt"].copy(), st["stats"].copy()
    e = np.arange(n)
    stats[13] = 620 + e % 5
    set_mt_state(ob, mt, stats[13])
    b.set_state(mt=mt, stats=stats)
    mask = e % 2 == 0
    b.reset(torch.as_tensor(mask.astype(np.uint8), device=b.device))
    _oracle_reset(ob, mask)
    fin = b.get_state(("mt", "stats"))
    assert np.array_equal(fin["mt"][~mask], mt[~mask]) and np.array_equal(fin["stats"][13][~mask], stats[13][~mask])
    idx = np.ctypeslib.as_array(ob.envs)["rng"]["index"]
    assert (idx[mask & (e % 5 == 4)] < 620).all()  # (from 624 the oracle's draw twisted first)
    _state_then_steps(b, ob)
    b.close()


def test_reset_behind_rejection_runs():
    """20 rejected words and an accepted one at the index of every masked env
    (past k_reset's 8-word window: the dependent-load loop), a second such
    run behind it for every fourth (the preview's draw), and the same runs
    in unmasked envs, which must not consume them."""
    n = 128
    b, ob = batch_and_oracle(n, [SEED0 + e for e in range(n)])
    st = b.get_state(("mt", "stats"))
    mt, stats = st["mt"].copy(), st["stats"].copy()
    rej, acc = untemper(0xFFFFFFFF), untemper(0)
    e = np.arange(n)
    mask = e % 3 != 0
    for i in range(n):
        idx = int(stats[13, i])
        assert idx + 42 <= 624
        if mask[i] or i % 2:
            mt[i, idx:idx + 20], mt[i, idx + 20] = rej, acc
        if i % 4 == 2:
            mt[i, idx + 21:idx + 41], mt[i, idx + 41] = rej, acc
    set_mt_state(ob, mt, stats[13])
    b.set_state(mt=mt, stats=stats)
    b.reset(torch.as_tensor(mask.astype(np.uint8), device=b.device))
    _oracle_reset(ob, mask)
    idx = np.ctypeslib.as_array(ob.envs)["rng"]["index"]
    assert (idx[mask] - stats[13][mask] == 21).all() and (idx[~mask] == stats[13][~mask]).all()
    _state_then_steps(b, ob)
    b.close()


# ---------------------------------------------------------------- a reset that comes late
def _late_reset_ref():
    """autoreset='none': the oracle one step at a time (step_one never
    resets).  Env e is reset e % 4 steps after its death and steps on its dead
    state until then; live envs are truncated at random as above (a dead env
    the random mask hits is reset then)."""
    n, steps = 256, T
    kw = dict(width=10, height=20, lock_delay=1, **SCORING)
    ob = O.OracleBatch(n, [SEED0 + e for e in range(n)], **kw)
    ob.reset()
    acts = _actions(steps, n)
    rnd = _mask_rows(n, steps, 1 / 16, special=False)
    ref = dict(acts=acts, obs=np.empty((steps, n, 10), np.uint32), reward=np.empty((steps, n), np.int32),
               done=np.empty((steps, n), np.uint8), rows=[])
    due = np.full(n, -1)
    delays, on_dead, trunc_locked = np.zeros(4, int), 0, 0
    for t in range(steps):
        on_dead += int((due >= 0).sum())  # steps taken on a dead state
        for e in range(n):
            obs, r, d, _ = ob.step_one(e, int(acts[t, e]))
            ref["obs"][t, e], ref["reward"][t, e], ref["done"][t, e] = pack_cols(obs), r, d
        died = ref["done"][t].astype(bool) & (due < 0)
        due[died] = t + np.arange(n)[died] % 4
        late = due == t
        row = (rnd[t].astype(bool) | late).astype(np.uint8)
        np.add.at(delays, np.arange(n)[late] % 4, 1)
        trunc_locked += int(((row != 0) & (due < 0) & (ob.field("lock") != 0)).sum())
        _oracle_reset(ob, row)
        due[row != 0] = -1
        ref["rows"].append(row)
    ref.update(ob=ob, state=ob.packed_state(), kw=kw,
               cover=dict(delays=delays.tolist(), steps_on_dead=on_dead, locked=trunc_locked))
    assert (delays > 0).all() and on_dead > 0 and trunc_locked > 0, ref["cover"]
    return ref


def test_late_reset_without_autoreset():
    ref = cached_ref("late reset", _late_reset_ref)
    n = ref["acts"].shape[1]
    b = _engine().TetrisBatch(n, autoreset="none", seeds=[SEED0 + e for e in range(n)], **ref["kw"])
    b.reset()
    try:
        drive_surface(b, ref, "step", ref["acts"], on_step=lambda t: _reset(b, ref["rows"][t], t))
        _check_final(b, ref)
    finally:
        b.close()


# ---------------------------------------------------------------- the vector env's reset mid-run
def test_vec_env_reset_mid_run_then_steps():
    """TetrisVecEnv.reset(return_info=True) of a running batch whose pieces
    rest with live lock counters: the info against the oracle, then 40 more
    steps on the vector surface and the final state."""
    G = _engine()
    n, t0, t1 = N, 50, 90
    kw = dict(lock_delay=2, step_reset=True)
    v = G.TetrisVecEnv(n, seed=SEED0, obs_format="packed", **kw)
    v.reset()
    ob = O.OracleBatch(n, [SEED0 + e for e in range(n)], **kw)
    ob.reset()
    acts = _actions(t1, n)
    dev = torch.as_tensor(acts, device=v.device)
    try:
        drive_surface(v, ob.rollout(acts[:t0]), "vec", dev[:t0])
        lock = ob.field("lock").copy()
        assert (lock == 1).any() and (lock == 2).any()
        obs, info = v.reset(return_info=True)
        ob.reset()
        assert int(obs.abs().sum()) == 0
        for k, f in (("time", "time"), ("score", "score"), ("lines_cleared", "lines_cleared"), ("holes", "holes"),
                     ("piece_height", "piece_height"), ("deaths", "n_deaths"), ("current_piece", "shape_id")):
            assert np.array_equal(info[k].cpu().numpy(), ob.field(f)), k
        assert np.array_equal(info["statistics"].cpu().numpy().T, ob.field("counts", (7,)))
        assert int(info["ep_score"].abs().sum()) == 0 and int(info["time"].abs().sum()) == 0
        # the counters handed over (read without st_mt_sync: the steps below go on from the reset's own state)
        assert np.array_equal(raw_state(v)["piece"][:n].view(np.uint32), ob.packed_state()["piece"])
        assert np.array_equal(ob.packed_state()["piece"] >> 17, lock)
        drive_surface(v, ob.rollout(acts[t0:]), "vec", dev[t0:])
        check_engine_state(v, ob.packed_state())
        check_mt_state(v, ob)
    finally:
        v.close()
