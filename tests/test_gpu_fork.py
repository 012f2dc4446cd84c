"""st_fork (TetrisBatch.fork / fork_groups): env states copied on the device,
against the oracle -- fork_ref's byte copies of its Env structs, whole or all
but `rng` -- between two batches and in place, with and without a pending
preview, across the end of an MT19937 generation, under another configuration,
and with indices outside the source.  A copy must then play exactly as the
oracle's copy does, and nothing else may change by a bit.

Ordering: every test enqueues fork() and the calls behind it (step,
next_piece, policy_linear) on one stream and never synchronises for the
engine's sake; where a test reads a state in between, it does so to check it.
test_fork_then_step_then_policy_without_a_read_between runs the three
back to back with no read at all."""
import ctypes

import numpy as np
import pytest
import torch

import fork_ref as FK
import lookahead_ref as LR
from oracle import oracle as O
from harness import (C4, batch_and_oracle, check_engine_state, check_mt_state, check_step, engine, engine_state,
                     raw_state, set_mt_state)

pytestmark = pytest.mark.gpu

BOARDS = {"10x20": (10, 20), "6x9": (6, 9)}
SIZES = ((70, 130), (256, 256))  # (src, dst): a ragged second wave into a ragged third; four full waves
SEED0 = 9700
PV_OK = 1 << 24  # the engine's "preview valid" bit of the MT index word (raw_state only)
MT_ROW = 13


def drop_heavy(T, n, seed=5):
    """actions [T, n]: about half hard drops, the rest uniform over the seven actions."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((T, n)) < 0.5, 2, rng.integers(0, 7, (T, n))).astype(np.uint8)


def _pair(board, n, seed0=SEED0, autoreset="same_step", **kw):
    W, H = BOARDS[board]
    return batch_and_oracle(n, [seed0 + e for e in range(n)], autoreset=autoreset, width=W, height=H, **kw)


def _index_word(b):
    return raw_state(b)["stats"][MT_ROW, :b.n].view(np.uint32)


def _has_preview(b):
    return (_index_word(b) & PV_OK) != 0


def _steps(b, ob, acts, t0=0):
    """b against ob over the rows of acts; under autoreset 'none' the dead envs
    are reset behind each step, as the oracle's rollout does by itself."""
    for t in range(len(acts)):
        ref = ob.rollout(acts[t:t + 1])
        check_step(ref, 0, *b.step(acts[t]), at=t0 + t)
        dead = ref["done"][0] != 0
        if b.autoreset == "none" and dead.any():
            b.reset(torch.as_tensor(dead.astype(np.uint8), device=b.device))


def _dev(b, a, dtype):
    return torch.as_tensor(np.asarray(a), device=b.device).to(dtype)


def _draw_index_mask(n_dst, n_src, seed):
    """A random index with repeats and a random half mask."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_src, n_dst).astype(np.int32), (rng.random(n_dst) < 0.5).astype(np.uint8)


def _full(b, wr):
    out = np.zeros(b.stride, bool)
    out[:b.n] = wr
    return out


def _assert_rows_kept(before, after, keep, what):
    """The envs `keep` (bool [stride], padding included) of a raw state: not a bit moved."""
    assert np.array_equal(before["board"][:, keep], after["board"][:, keep]), (what, "board")
    assert np.array_equal(before["stats"][:, keep], after["stats"][:, keep]), (what, "stats")
    assert np.array_equal(before["mt"][keep], after["mt"][keep]), (what, "mt")
    assert np.array_equal(before["piece"][keep], after["piece"][keep]), (what, "piece")


def _assert_same_raw(a, b, what):
    _assert_rows_kept(a, b, np.ones(a["piece"].shape[0], bool), what)


def _assert_deep_copies(raw_dst, raw_src, wr, index, what):
    """Written env e of dst is env index[e] of src bit for bit: board, every
    counter row, the index word with its engine bits and the whole MT row."""
    e = np.flatnonzero(wr)
    s = np.asarray(index)[e]
    assert np.array_equal(raw_dst["board"][:, e], raw_src["board"][:, s]), (what, "board")
    assert np.array_equal(raw_dst["stats"][:, e], raw_src["stats"][:, s]), (what, "stats")
    assert np.array_equal(raw_dst["mt"][e], raw_src["mt"][s]), (what, "mt")


# ------------------------------------------------------------------ the deep copy
@pytest.mark.parametrize("autoreset", ("same_step", "none"))
@pytest.mark.parametrize("sizes", SIZES)
@pytest.mark.parametrize("board", sorted(BOARDS))
def test_deep_copy_against_the_oracle(board, sizes, autoreset):
    ns, nd = sizes
    src, osrc = _pair(board, ns)
    dst, odst = _pair(board, nd, SEED0 + 3000, autoreset=autoreset)
    twin = engine().TetrisBatch(nd, width=src.width, height=src.height, seeds=[1] * nd)
    twin.reset()
    try:
        _steps(src, osrc, drop_heavy(30, ns, 1))
        _steps(dst, odst, drop_heavy(7, nd, 2))
        index, mask = _draw_index_mask(nd, ns, 3)
        pv = _has_preview(src)
        raw_src, raw_dst = raw_state(src), raw_state(dst)
        assert dst.fork(src, index=_dev(dst, index, torch.int32), mask=_dev(dst, mask, torch.uint8)) is dst
        wr = FK.fork(odst, osrc, index, mask)
        assert np.array_equal(wr, mask != 0)
        with_pv, without = int(pv[index[wr]].sum()), int((~pv[index[wr]]).sum())
        print("deep fork", board, sizes, "sources with a preview", with_pv, "without", without)
        assert with_pv > 0 and without > 0
        _assert_same_raw(raw_src, raw_state(src), "src is only read")
        after = raw_state(dst)
        _assert_rows_kept(raw_dst, after, ~_full(dst, wr), "unwritten envs")
        _assert_deep_copies(after, raw_src, wr, index, "written envs")
        # the state in st_mt_sync's form, through a whole copy of dst (NULL index, NULL mask) so that dst
        # itself keeps its previews for the steps below
        twin.fork(dst)
        es, et = engine_state(src), engine_state(twin)
        for k in es:
            a, b = (et[k][wr], es[k][index[wr]]) if k in ("mt", "piece") else (et[k][..., wr], es[k][..., index[wr]])
            assert np.array_equal(a, b), k
        _steps(dst, odst, drop_heavy(40, nd, 4), 7)
        check_engine_state(dst, odst.packed_state())
        check_mt_state(dst, odst)
    finally:
        src.close(), dst.close(), twin.close()


@pytest.mark.parametrize("waves", ("1", "4"))
def test_deep_copy_with_either_grid(waves, monkeypatch):
    """The deep copy's two grids (ST_FORK_WAVES, a diagnostic switch read per
    call): one wave or four per 64 envs, the same bits."""
    monkeypatch.setenv("ST_FORK_WAVES", waves)
    ns, nd = 70, 130
    src, osrc = _pair("10x20", ns)
    dst, odst = _pair("10x20", nd, SEED0 + 3000)
    try:
        _steps(src, osrc, drop_heavy(30, ns, 1))
        index, mask = _draw_index_mask(nd, ns, 6)
        mask[64:128] = 1  # a wave with every lane written
        raw_src, raw_dst = raw_state(src), raw_state(dst)
        dst.fork(src, index=_dev(dst, index, torch.int32), mask=_dev(dst, mask, torch.uint8))
        wr = FK.fork(odst, osrc, index, mask)
        after = raw_state(dst)
        _assert_rows_kept(raw_dst, after, ~_full(dst, wr), "unwritten envs")
        _assert_deep_copies(after, raw_src, wr, index, "written envs")
        _steps(dst, odst, drop_heavy(20, nd, 4))
        check_engine_state(dst, odst.packed_state())
        check_mt_state(dst, odst)
    finally:
        src.close(), dst.close()


# ------------------------------------------------------------------ ST_FORK_KEEP_RNG
@pytest.mark.parametrize("prep", ("reset", "synced"))
@pytest.mark.parametrize("sizes", SIZES)
@pytest.mark.parametrize("board", sorted(BOARDS))
def test_keep_rng_against_the_oracle(board, sizes, prep):
    """dst right after its reset (every env holds a preview, drawn under its
    own shape counts) or after some steps and sync_mt() (none does)."""
    ns, nd = sizes
    src, osrc = _pair(board, ns)
    dst, odst = _pair(board, nd, SEED0 + 3000)
    try:
        _steps(src, osrc, drop_heavy(30, ns, 1))
        if prep == "synced":
            _steps(dst, odst, drop_heavy(7, nd, 2))
            dst.sync_mt()
        assert _has_preview(dst).all() if prep == "reset" else not _has_preview(dst).any()
        index, mask = _draw_index_mask(nd, ns, 3)
        raw_src, raw_dst = raw_state(src), raw_state(dst)
        dst.fork(src, index=_dev(dst, index, torch.int32), mask=_dev(dst, mask, torch.uint8), keep_rng=True)
        wr = FK.fork(odst, osrc, index, mask, keep_rng=True)
        _assert_same_raw(raw_src, raw_state(src), "src is only read")
        after = raw_state(dst)
        _assert_rows_kept(raw_dst, after, ~_full(dst, wr), "unwritten envs")
        rows = [r for r in range(after["stats"].shape[0]) if r != MT_ROW]
        e = np.flatnonzero(wr)
        assert np.array_equal(after["board"][:, e], raw_src["board"][:, index[e]])
        assert np.array_equal(after["stats"][rows][:, e], raw_src["stats"][rows][:, index[e]])
        assert (after["stats"][MT_ROW, e].view(np.uint32) <= 624).all()  # CPython's form: no engine bits
        check_mt_state(dst, odst, "dst's own stream")
        check_engine_state(dst, odst.packed_state(), "copied")
        got = dst.next_piece().cpu().numpy()
        assert np.array_equal(got, LR.next_pieces(odst))  # drawn under the copied shape counts
        _steps(dst, odst, drop_heavy(40, nd, 4))
        check_engine_state(dst, odst.packed_state())
        check_mt_state(dst, odst)
    finally:
        src.close(), dst.close()


# ------------------------------------------------------------------ the end of an MT19937 generation
def _boundary(board, n, seed0):
    """A batch and its oracle whose envs hold host-written CPython states with
    index 618..624 (env e: 618 + e % 7); the even envs have then drawn their
    preview across the generation's end (next_piece), the odd ones hold none.
    The mix is made with the deep fork itself (from a batch in which every env
    drew); the reference sees no preview, so one oracle stands for both."""
    a, oa = _pair(board, n, seed0)
    b, _ = _pair(board, n, seed0)
    acts = drop_heavy(10, n, 11)
    _steps(a, oa, acts)
    for t in range(len(acts)):
        b.step(acts[t])
    st = a.get_state(("stats", "mt"))
    index = (618 + np.arange(n) % 7).astype(np.int32)
    st["stats"][MT_ROW] = index
    a.set_state(stats=st["stats"], mt=st["mt"])
    b.set_state(stats=st["stats"], mt=st["mt"])
    set_mt_state(oa, st["mt"], index)
    a.next_piece()
    even = np.arange(n) % 2 == 0
    b.fork(a, mask=_dev(b, even, torch.uint8))
    a.close()
    w = _index_word(b)
    assert np.array_equal((w & PV_OK) != 0, even)
    crossed = even & ((w & 0x3FF) <= ((w >> 25) & 63))
    at_624 = even & ((w & 0x3FF) == ((w >> 25) & 63))  # idx == c: the draw began exactly at 624
    print("boundary", board, n, "previews that crossed", int(crossed.sum()), "of them begun at 624", int(at_624.sum()))
    assert at_624.sum() > 0 and np.array_equal(at_624, even & (index == 624))
    return b, oa


@pytest.mark.parametrize("keep_rng", (False, True))
@pytest.mark.parametrize("n", (70, 256))
@pytest.mark.parametrize("board", sorted(BOARDS))
def test_generation_boundary(board, n, keep_rng):
    """Deep: the boundary states are the sources.  KEEP_RNG: they are dst's own,
    whose previews go back across index 624.  Then six hard drops (lock_delay 0:
    every one locks and spawns) against the oracle."""
    edge, oedge = _boundary(board, n, SEED0 + 500)
    other, oother = _pair(board, n, SEED0 + 900)
    try:
        _steps(other, oother, drop_heavy(12, n, 13))
        index = np.random.default_rng(14).integers(0, n, n).astype(np.int32)
        dst, odst, src, osrc = (edge, oedge, other, oother) if keep_rng else (other, oother, edge, oedge)
        dst.fork(src, index=_dev(dst, index, torch.int32), keep_rng=keep_rng)
        FK.fork(odst, osrc, index, None, keep_rng=keep_rng)
        if keep_rng:
            assert not _has_preview(dst).any()
            check_mt_state(dst, odst, "given back")
            assert np.array_equal(engine_state(dst, ("stats",))["stats"][MT_ROW], 618 + np.arange(n) % 7)
            assert np.array_equal(dst.next_piece().cpu().numpy(), LR.next_pieces(odst))
        hard = np.full((6, n), 2, np.uint8)
        spawned = odst.field("counts", (7,)).sum(axis=1).copy()
        _steps(dst, odst, hard)
        assert (odst.field("counts", (7,)).sum(axis=1) - spawned >= 2).all()
        check_engine_state(dst, odst.packed_state())
        check_mt_state(dst, odst)
        _steps(dst, odst, drop_heavy(10, n, 15), 6)
        check_mt_state(dst, odst, "end")
    finally:
        edge.close(), other.close()


# ------------------------------------------------------------------ in place
@pytest.mark.parametrize("keep_rng", (False, True))
@pytest.mark.parametrize("n,group", ((256, 8), (256, 64), (70, 3)))
def test_fork_groups_in_place(n, group, keep_rng):
    b, ob = _pair("10x20", n)
    try:
        _steps(b, ob, drop_heavy(20, n, 21))
        raw0 = raw_state(b)
        assert b.fork_groups(group, keep_rng=keep_rng) is b
        root = np.arange(n) // group * group
        wr = FK.fork(ob, ob, root, root != np.arange(n), keep_rng=keep_rng)
        assert wr.sum() == n - len(range(0, n, group))
        raw1 = raw_state(b)
        _assert_rows_kept(raw0, raw1, ~_full(b, wr), "roots and padding")
        rows = [r for r in range(raw1["stats"].shape[0]) if not (keep_rng and r == MT_ROW)]
        assert np.array_equal(raw1["board"][:, :n], raw0["board"][:, root])
        assert np.array_equal(raw1["stats"][rows][:, :n], raw0["stats"][rows][:, root])
        if not keep_rng:
            assert np.array_equal(raw1["mt"][:n], raw0["mt"][root])
        b.fork_groups(group, keep_rng=keep_rng)  # the cached index and mask; the same result
        if not keep_rng:
            _assert_same_raw(raw1, raw_state(b), "again")
        _steps(b, ob, drop_heavy(25, n, 22), 20)  # the members diverge under their own actions
        assert len({bytes(ob.envs[e])[FK._CFG[1]:FK._RNG[0]] for e in range(min(group, n))}) > 1
        check_engine_state(b, ob.packed_state())
        check_mt_state(b, ob)
    finally:
        b.close()


# ------------------------------------------------------------------ configuration is not state
@pytest.mark.parametrize("keep_rng", (False, True))
def test_dst_plays_by_its_own_rules(keep_rng):
    n = 70
    src, osrc = _pair("10x20", n, lock_delay=0)
    dst, odst = _pair("10x20", n, SEED0 + 3000, lock_delay=0, step_reset=True, **C4)
    try:
        _steps(src, osrc, drop_heavy(30, n, 31))
        index = np.random.default_rng(32).integers(0, n, n).astype(np.int32)
        dst.fork(src, index=index, keep_rng=keep_rng)  # (a host index: converted)
        FK.fork(odst, osrc, index, None, keep_rng=keep_rng)
        assert odst.envs[0].cfg.advanced_clears == 1 and osrc.envs[0].cfg.advanced_clears == 0
        ref = [odst.rollout(a[None]) for a in drop_heavy(30, n, 33)]
        assert any((r["reward"] != 0).any() for r in ref)
        acts = drop_heavy(30, n, 33)
        for t in range(30):
            check_step(ref[t], 0, *dst.step(acts[t]), at=t)
        check_engine_state(dst, odst.packed_state())
        check_mt_state(dst, odst)
    finally:
        src.close(), dst.close()


# ------------------------------------------------------------------ guards
def test_indices_outside_the_source_leave_their_envs_alone():
    from gym_simpletetris_amd import _lib as C
    ns, nd = 70, 130
    src, osrc = _pair("6x9", ns)
    dst, odst = _pair("6x9", nd, SEED0 + 3000)
    try:
        _steps(src, osrc, drop_heavy(15, ns, 41))
        _steps(dst, odst, drop_heavy(5, nd, 42))
        index = np.resize(np.array([-1, ns, 2**31 - 1, -2**31, ns + 1, 127, 128, 10**6], np.int32), nd)
        guard_i = torch.full((nd + 16,), 77, dtype=torch.int32, device=dst.device)
        guard_m = torch.full((nd + 16,), 1, dtype=torch.uint8, device=dst.device)
        guard_i[8:8 + nd] = _dev(dst, index, torch.int32)
        raw_src, raw_dst = raw_state(src), raw_state(dst)
        for flags in (0, C.FORK_KEEP_RNG):
            rc = dst._L.st_fork(dst._ctx, src._ctx, ctypes.c_void_p(guard_i[8:].data_ptr()),
                                ctypes.c_void_p(guard_m[8:].data_ptr()), flags, dst._stream())
            assert rc == C.ST_OK
            _assert_same_raw(raw_dst, raw_state(dst), ("every index outside [0, n)", flags))
        # among envs that are written: the others keep every bit
        index[::3] = np.arange(nd)[::3] % ns
        guard_i[8:8 + nd] = _dev(dst, index, torch.int32)
        dst.fork(src, index=guard_i[8:8 + nd], mask=guard_m[8:8 + nd])
        wr = FK.fork(odst, osrc, index, None)
        assert np.array_equal(wr, (index >= 0) & (index < ns)) and 0 < wr.sum() < nd
        after = raw_state(dst)
        _assert_rows_kept(raw_dst, after, ~_full(dst, wr), "unwritten envs")
        _assert_deep_copies(after, raw_src, wr, index, "written envs")
        _assert_same_raw(raw_src, raw_state(src), "src is only read")
        want_i = np.full(nd + 16, 77, np.int32)
        want_i[8:8 + nd] = index
        assert np.array_equal(guard_i.cpu().numpy(), want_i) and (guard_m == 1).all()  # fork writes no caller buffer
        _steps(dst, odst, drop_heavy(15, nd, 43), 5)
        check_mt_state(dst, odst)
    finally:
        src.close(), dst.close()


def test_mismatched_and_unready_batches_are_refused():
    from gym_simpletetris_amd import _lib as C
    G = engine()
    a, _ = _pair("10x20", 8)
    b, _ = _pair("6x9", 8)
    fresh = G.TetrisBatch(8, seeds=list(range(8)))  # seeded, never reset
    try:
        raw = raw_state(a)
        for dst, src, code in ((a, b, C.ST_EINVAL), (b, a, C.ST_EINVAL), (a, fresh, C.ST_ESTATE), (fresh, a, C.ST_ESTATE)):
            with pytest.raises(C.StError) as err:
                dst.fork(src)
            assert err.value.code == code and "st_fork" in str(err.value)
        dev = a.device
        i32 = torch.zeros(8, dtype=torch.int32, device=dev)
        for bad in (dict(index=i32.to(torch.int64)), dict(index=i32.float()), dict(index=i32[:7]), dict(index=i32.cpu()),
                    dict(index=torch.zeros(16, dtype=torch.int32, device=dev)[::2]), dict(index=[0] * 7),
                    dict(mask=i32), dict(mask=torch.ones(9, dtype=torch.uint8, device=dev)),
                    dict(mask=torch.ones(8, dtype=torch.uint8)), dict(src=object())):
            with pytest.raises((ValueError, TypeError)):
                a.fork(**bad)
        _assert_same_raw(raw, raw_state(a), "nothing was launched")
    finally:
        a.close(), b.close(), fresh.close()


# ------------------------------------------------------------------ ordering
def test_fork_then_step_then_policy_without_a_read_between():
    G = engine()
    ns, nd = 70, 130
    src, osrc = _pair("10x20", ns)
    seeds = [SEED0 + 3000 + e for e in range(nd)]
    dst = G.TetrisBatch(nd, seeds=seeds, autoreset="same_step", validate_actions=False)  # (no action check: no sync)
    odst = O.OracleBatch(nd, seeds)
    dst.reset()
    odst.reset()
    try:
        _steps(src, osrc, drop_heavy(30, ns, 51))
        index, mask = _draw_index_mask(nd, ns, 52)
        acts = drop_heavy(2, nd, 53)
        d_index, d_mask = _dev(dst, index, torch.int32), _dev(dst, mask, torch.uint8)
        d_acts = _dev(dst, acts, torch.uint8)
        out = tuple(t.clone() for t in (dst.obs, dst.reward, dst.done))
        torch.cuda.synchronize()
        dst.fork(src, index=d_index, mask=d_mask)
        dst.step(d_acts[0], out=out)
        choice = dst.policy_linear(G.GREEDY_WEIGHTS)
        src.step(_dev(src, drop_heavy(1, ns, 54)[0], torch.uint8))  # src moves on behind the fork
        FK.fork(odst, osrc, index, mask)
        check_step(odst.rollout(acts[:1]), 0, *out)
        assert torch.equal(choice.slots, dst.policy_linear(G.GREEDY_WEIGHTS).slots)
        check_engine_state(dst, odst.packed_state())
        check_mt_state(dst, odst)
        _steps(dst, odst, acts[1:], 1)
    finally:
        src.close(), dst.close()
