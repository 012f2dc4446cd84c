"""The shared oracle harness (tests/harness.py, OracleBatch's state views) on
the CPU: a checker that silently compared nothing would hollow out the whole
GPU suite, so each one is shown to pass on the oracle's own rows and to fail
on one perturbed element, and the packers against their slow per-env forms."""
import random

import numpy as np
import pytest
import torch

import harness as Hn
from oracle import oracle as O


def _batch(n, W, H, seed0=50, **kw):
    ob = O.OracleBatch(n, [seed0 + e for e in range(n)], width=W, height=H, **kw)
    ob.reset()
    return ob


@pytest.mark.parametrize("W,H", [(4, 4), (5, 27), (32, 28), (10, 20)])
def test_packed_state_equals_the_per_env_reads(W, H):
    n = 5
    ob = _batch(n, W, H)
    ob.rollout(O.splitmix64_actions(3, 0, 40, n))
    st = ob.packed_state()
    assert st["board"].shape == (W, n) and st["board"].dtype == np.uint32 and st["piece"].dtype == np.uint32
    assert st["stats"].shape == (13, n) and st["stats"].dtype == np.int32
    assert ob.boards().shape == (n, 32, 32) and ob.boards().dtype == np.uint8
    for i in range(n):
        e = ob.envs[i]
        cols = [sum(int(c) << y for y, c in enumerate(col)) for col in ob.board(i)]
        assert list(st["board"][:, i]) == cols, i
        assert np.array_equal(ob.boards()[i, :W, :H], ob.board(i)), i
        assert int(st["piece"][i]) == e.shape_id | (e.rot & 3) << 3 | e.ax << 5 | e.ay << 11 | e.lock << 17, i
        assert list(st["stats"][:, i]) == [e.time, e.score, e.lines_cleared, e.holes, e.piece_height,
                                           e.n_deaths] + list(e.counts), i
    assert st["board"].any() and st["stats"][0].any()  # 40 steps in: something to compare
    ob.field("ax")[:] = np.arange(n) + 1  # the views write through
    ob.field("counts", (7,))[:, 6] = 77
    ob.boards()[:, 0, 0] = 1
    assert [ob.envs[i].ax for i in range(n)] == list(range(1, n + 1))
    assert all(ob.envs[i].counts[6] == 77 and ob.board(i)[0, 0] == 1 for i in range(n))


@pytest.mark.parametrize("seed", [0, 12345, 2**40 + 7])
def test_mt_twist_is_cpythons_refill(seed):
    r = random.Random(seed)
    before = r.getstate()[1]
    assert before[624] == 624  # the next draw refills
    r.getrandbits(32)
    after = r.getstate()[1]
    assert after[624] == 1
    got = Hn.mt_twist(np.array([before[:624], before[:624]], np.uint32))
    assert got.dtype == np.uint32 and np.array_equal(got[0], np.array(after[:624], np.uint32))
    assert np.array_equal(got[0], got[1])


def test_untemper_inverts_cpythons_tempering():
    """A state word untemper(y) at CPython's index comes out as y: the crafted
    MT states' all-ones words are rejected by every randint range, their zero
    words accepted."""
    r = random.Random(9)
    st = r.getstate()
    want = [0xFFFFFFFF, 0, 0x12345678, 0x80000001]
    words = list(st[1][:624])
    words[5:9] = [Hn.untemper(y) for y in want]
    r.setstate((st[0], tuple(words) + (5,), st[2]))
    assert [r.getrandbits(32) for _ in want] == want


@pytest.mark.parametrize("H", [4, 20, 28])
def test_unpack_f32_pack_cols_round_trip(H):
    cells = np.random.default_rng(H).integers(0, 2, (3, 7, H)).astype(np.uint8)
    cells[0, 0, :] = 1
    cells[0, 1, :] = 0
    cells[0, 1, H - 1] = 1  # the top bit alone
    cols = Hn.pack_cols(cells)
    assert cols.dtype == np.uint32 and cols.shape == (3, 7)
    assert cols[0, 0] == (1 << H) - 1 and cols[0, 1] == 1 << (H - 1)
    f32 = Hn.unpack_f32(cols, H)
    assert f32.dtype == np.float32 and np.array_equal(f32, cells)
    assert np.array_equal(Hn.pack_cols(f32), cols)
    assert np.array_equal(Hn.pack_cols(cells[1]), cols[1])  # one board [W, H]


N, W, H, T = 8, 6, 9, 3


@pytest.fixture(scope="module")
def run():
    """3 oracle steps of 8 envs on 6x9, 37 steps into their games (hard
    drops on every other step: an env dies within the three), and torch CPU
    tensors in the engine's layout standing in for its outputs."""
    ob = _batch(N, W, H, **Hn.C4)
    acts = O.splitmix64_actions(9, 0, 37 + T, N)
    acts[1::2] = 2
    ob.rollout(acts[:37])
    ref = Hn.record(ob, acts[37:])
    assert ref["done"].any() and not ref["done"].all(axis=1).any()
    outs = [(torch.from_numpy(np.ascontiguousarray(ref["obs"][t].T).view(np.int32)),
             torch.from_numpy(ref["reward"][t].copy()), torch.from_numpy(ref["done"][t].astype(bool)))
            for t in range(T)]
    return ref, outs


def _fails(fn, *a, **kw):
    with pytest.raises(AssertionError):
        fn(*a, **kw)


def test_check_step_passes_and_fails(run):
    ref, outs = run
    for t, (obs, rew, done) in enumerate(outs):
        Hn.check_step(ref, t, obs, rew, done)
        Hn.check_step(ref, t, obs.numpy(), rew.numpy(), done.numpy())
        Hn.check_step(ref, t, obs[:, 2:5], rew[2:5], done[2:5], sel=slice(2, 5))
        Hn.check_step(ref, t, torch.from_numpy(Hn.unpack_f32(ref["obs"][t], H)), rew, done, H=H)
        for x in range(W):  # one obs bit of any column, low or high
            bad = obs.clone()
            bad[x, N - 1] ^= 1 << (x % H)
            _fails(Hn.check_step, ref, t, bad, rew, done)
        bad = rew.clone()
        bad[3] += 1
        _fails(Hn.check_step, ref, t, obs, bad, done)
        bad = done.clone()
        bad[0] = ~bad[0]
        _fails(Hn.check_step, ref, t, obs, rew, bad)
        _fails(Hn.check_step, ref, (t + 1) % T, obs, rew, done)  # another step's row
    o, r, d = (torch.stack([x[i] for x in outs]) for i in range(3))
    Hn.check_steps(ref, o, r, d)
    Hn.check_steps(ref, o[1:], r[1:], d[1:], t0=1)
    _fails(Hn.check_steps, ref, o[1:], r[1:], d[1:])
    bad = r.clone()
    bad[T - 1, N - 1] -= 1
    _fails(Hn.check_steps, ref, o, bad, d)
    _fails(Hn.check_steps, ref, o[:0], r[:0], d[:0])  # nothing to compare is no pass


def test_check_f32_passes_and_fails(run):
    ref, _ = run
    f32 = torch.from_numpy(Hn.unpack_f32(ref["obs"][1], H))
    assert f32.shape == (N, W, H) and bool(f32.any())
    Hn.check_f32(f32, ref["obs"][1], H, 1)
    for cell in ((0, 0, 0), (N - 1, W - 1, H - 1)):
        bad = f32.clone()
        bad[cell] = 1 - bad[cell]
        _fails(Hn.check_f32, bad, ref["obs"][1], H, 1)


def _info(ref, t):
    """What the vector env reports for oracle row t (reset convention)."""
    st, done = ref["stats"][t], ref["done"][t].astype(bool)
    z = np.zeros_like(st[:, 0])
    live = dict(time=0, score=1, lines_cleared=2, holes=3, piece_height=6)
    info = {k: np.where(done, z, st[:, c]) for k, c in live.items()}
    info.update({"ep_" + k: np.where(done, st[:, c], z) for k, c in dict(time=0, score=1, lines=2, holes=3).items()})
    info.update(deaths=st[:, 4].copy(), current_piece=np.where(done, 7, st[:, 5]),  # (a reset env: a new piece)
                final_observation=np.ascontiguousarray(np.where(done[:, None], ref["obs"][t], 0).T).view(np.int32),
                _final_observation=done.copy())
    return {k: torch.from_numpy(v) for k, v in info.items()}, done


def test_check_info_and_final_observation_pass_and_fail(run):
    ref, _ = run
    t = int(np.argmax(ref["done"].any(axis=1)))
    info, done = _info(ref, t)
    live, dead = int(np.argmin(done)), int(np.argmax(done))
    Hn.check_info(info, ref["stats"][t], done, t)
    Hn.check_final_observation(info, ref["obs"][t], done, t)
    for k in ("time", "score", "lines_cleared", "holes", "deaths", "piece_height", "ep_time", "ep_score", "ep_lines",
              "ep_holes", "current_piece"):
        for e in (live, dead):
            if k == "current_piece" and e == dead:
                continue  # a reset env holds its new piece: not the oracle's row
            bad = dict(info, **{k: info[k].clone()})
            bad[k][e] += 1
            _fails(Hn.check_info, bad, ref["stats"][t], done, t)
    bad = dict(info, final_observation=info["final_observation"].clone())
    bad["final_observation"][W - 1, dead] ^= 1 << (H - 1)
    _fails(Hn.check_final_observation, bad, ref["obs"][t], done, t)
    bad["final_observation"] = info["final_observation"].clone()
    bad["final_observation"][0, live] = 1  # a live env's must be zero
    _fails(Hn.check_final_observation, bad, ref["obs"][t], done, t)
    bad = dict(info, _final_observation=~info["_final_observation"])
    _fails(Hn.check_final_observation, bad, ref["obs"][t], done, t)
    f32 = dict(info, final_observation=torch.from_numpy(Hn.unpack_f32(Hn.words(info["final_observation"]), H)))
    Hn.check_final_observation(f32, ref["obs"][t], done, t, H=H)
    f32["final_observation"][dead, 0, H - 1] = 1 - f32["final_observation"][dead, 0, H - 1]
    _fails(Hn.check_final_observation, f32, ref["obs"][t], done, t, H=H)


class _Engine:
    """get_state() of a TetrisBatch, from an oracle batch."""

    def __init__(self, ob):
        rng = np.ctypeslib.as_array(ob.envs)["rng"]
        self.st = dict(ob.packed_state(), mt=rng["mt"].copy())
        self.st["stats"] = np.concatenate([self.st["stats"], rng["index"][None], np.zeros((5, ob.n), np.int32)])

    def get_state(self, fields=("board", "piece", "stats", "mt")):
        return {k: self.st[k] for k in fields}


def test_state_checks_pass_and_fail():
    ob = _batch(N, W, H)
    ob.rollout(O.splitmix64_actions(1, 0, 30, N))
    a, b = _Engine(ob), _Engine(ob)
    snap = Hn.engine_state(a)
    assert sorted(snap) == ["board", "mt", "piece", "stats"] and snap["board"] is not a.st["board"]
    assert sorted(Hn.engine_state(a, ("board", "mt"))) == ["board", "mt"]
    Hn.assert_same_state(a, b)
    Hn.assert_same_state(snap, b)
    Hn.assert_same_state({k: torch.from_numpy(v) for k, v in snap.items()}, b)
    Hn.check_engine_state(a, ob.packed_state())
    Hn.check_mt_state(a, ob)
    for k, at in (("board", (W - 1, N - 1)), ("piece", (0,)), ("stats", (12, 3)), ("stats", (18, 0)),
                  ("mt", (N - 1, 623))):
        b.st[k] = a.st[k].copy()
        b.st[k][at] ^= 1
        _fails(Hn.assert_same_state, a, b)
        _fails(Hn.assert_same_state, snap, b)
        Hn.assert_same_state(a, b, fields=tuple(f for f in ("board", "piece", "stats", "mt") if f != k))
        if k != "mt" and at != (18, 0):  # (rows past the counters are not the oracle's)
            _fails(Hn.check_engine_state, b, ob.packed_state())
        b.st[k] = a.st[k]
    _fails(Hn.assert_same_state, snap, {k: snap[k] for k in ("board", "piece")})  # a field is missing
    _fails(Hn.assert_same_state, {}, {})
    for index, word in ((ob.field("time") + 3, 0), (a.st["stats"][13], 1 << 31)):  # one MT index, then one word, moved
        mt = a.st["mt"].copy()
        mt[0, 5] ^= word
        Hn.set_mt_state(ob, mt, index)
        assert [ob.envs[i].rng.index for i in range(N)] == list(index) and ob.envs[0].rng.mt[5] == mt[0, 5]
        _fails(Hn.check_mt_state, a, ob)
    Hn.set_mt_state(ob, a.st["mt"], a.st["stats"][13])
    Hn.check_mt_state(a, ob)


def test_record_equals_rollout_and_cached_ref_freezes():
    n, steps = 7, 60
    acts = O.splitmix64_actions(4, 0, steps, n)
    acts[::3] = 2
    a, b = _batch(n, 10, 20, **Hn.C4), _batch(n, 10, 20, **Hn.C4)
    seen = []
    rec = Hn.record(a, acts, before=lambda t: a.field("time").copy(),
                    after=lambda t, locked, pre: seen.append((t, pre, locked.copy(), a.field("time").copy())))
    ref = b.rollout(acts)
    for k in ("obs", "reward", "done", "stats"):
        assert rec[k].dtype == ref[k].dtype and np.array_equal(rec[k], ref[k]), k
    assert rec["acts"] is acts and rec["done"].any()
    # locked: the shape counts moved (a spawn) or the env died -- from per-env reads of a third batch
    c = _batch(n, 10, 20, **Hn.C4)
    for t in range(steps):
        spawned = [sum(c.envs[i].counts) for i in range(n)]
        died = c.rollout(acts[t:t + 1])["done"][0]
        assert list(rec["locked"][t]) == [sum(c.envs[i].counts) != spawned[i] or bool(died[i]) for i in range(n)], t
    assert rec["locked"].any() and not rec["locked"].all()
    # the hooks ran around every step, in order, with before's value handed on
    assert [s[0] for s in seen] == list(range(steps))
    assert all(np.array_equal(s[2], rec["locked"][s[0]]) for s in seen)
    assert all(np.array_equal(seen[t][1], seen[t - 1][3]) for t in range(1, steps))
    calls = []
    made = Hn.cached_ref(("test_harness", 1), lambda: calls.append(1) or dict(rec, nested=[dict(x=np.zeros(3))]))
    assert Hn.cached_ref(("test_harness", 1), lambda: calls.append(1)) is made and calls == [1]
    for arr in (made["obs"], made["nested"][0]["x"]):
        with pytest.raises(ValueError):
            arr[...] = 1


def test_parallel_oracle_equals_one_batch():
    n, steps = 37, 25
    orc = Hn.ParallelOracle(n, Hn.C4, parts=4, seed_base=321, aseed=0xABC, board=(6, 9))
    ob = _batch(n, 6, 9, seed0=321, **Hn.C4)
    ref = ob.rollout(O.splitmix64_actions(0xABC, 0, steps + 5, n))
    try:
        assert len(orc.sl) == 4 and orc.sl[0][0] == 0 and orc.sl[-1][1] == n
        got, more = orc.rollout(0, steps, stats=True), orc.rollout(steps, 5)
        for k in ("obs", "reward", "done", "stats"):
            assert np.array_equal(got[k], ref[k][:steps]), k
        assert np.array_equal(more["obs"], ref["obs"][steps:]) and "stats" not in more
        rng = np.ctypeslib.as_array(ob.envs)["rng"]
        Hn.assert_same_state(orc.packed_state(), dict(ob.packed_state(), mt=rng["mt"], mt_index=rng["index"]))
    finally:
        orc.close()
    d = Hn.ParallelOracle(3, {}, parts=1)  # the defaults: bench.py's seeds, action stream and board
    assert bytes(d.obs[0].envs) == bytes(_batch(3, 10, 20, seed0=1000).envs) and d.aseed == 0x5EED
    assert 1 <= Hn._threads() <= 16
    d.close()
