"""The lock path (paint_box, lock_board with its per-wave compaction loop, the
hole sums and the scoring rules -- inline in step_logic, lock_score in
rollout_wave) on crafted boards, in every kernel that runs it.

Uniform actions and the wall pattern almost never clear a row, so each env
starts from a host-written state: a vertical I over a one-column well whose
4-row window holds a chosen subset of rows that are full but for the well
column.  Env i selects how the lock is reached (m), the subset (s), where the
window lies (p: on the floor, on support rows, at row 0, one cell above the
board, over rows that are full already) and the well column (c).  Within a
wave p is constant while s and m take all 64 combinations, so the lanes of a
wave clear different row counts, and of every 4 envs two lock at step 0 and two
later.  Counters are host-written too.  Every output of every step and the
final state are bit-exact against the C oracle (pinned to the reference for
these rules by the top_lock_*, clipped_lock_clear, prefull_*, tall_tetris and
small_split cases of tests/golden/crafted.npz)."""
import ctypes

import numpy as np
import pytest
import torch

from harness import (C4, cached_ref, check_engine_state, check_step, check_steps, drive_surface,
                     engine as _engine, pack_cols, record)
from oracle import oracle as O

T = 16
SEED0 = 9090
ACT_SEED = 0x10C4
NGEN = 1320  # crafted states are drawn for this many envs; a run takes the first n
# n: 10x20 (the fixed-size kernel) a multiple of 4 with a partial last
# workgroup, so the 16-byte and the per-env store paths both run; the generic
# kernel at 6x9 / 4x4, with H > 25 (64-bit cell shifts) at 5x27, at W = 32
BOARDS = {(10, 20): 1320, (6, 9): 1280, (4, 4): 1280, (5, 27): 1280, (32, 28): 1280}
HHH = dict(high_scoring=True, penalise_height=True, penalise_holes=True)
SCORING = {"c3": {}, "c4": C4, "hhh": HHH}


def _ids(v):
    return v if isinstance(v, str) else "%dx%d" % v


def _index_fields(n):
    i = np.arange(n)
    return i % 4, (i // 4) % 16, (i // 64) % 5, (i // 320) % 4


_CRAFTED = {}


def crafted_state(W, H, adv):
    """The crafted state of NGEN envs: boards u8 [n, W, H], the I's column and
    start row, the host-written counters and the constructed clear count."""
    if (W, H, adv) not in _CRAFTED:
        _CRAFTED[(W, H, adv)] = _crafted_state(W, H, adv)
    return _CRAFTED[(W, H, adv)]


def _crafted_state(W, H, adv):
    rng = np.random.default_rng([77, W, H, int(adv)])
    n = NGEN
    m, s, p, ci = _index_fields(n)
    c = np.array([0, W - 1, W // 2, 1])[ci]
    r0 = np.select([p == 0, p == 1, p == 2, p == 3],
                   [H - 4, H - 4 - min(3, H - 4), 0, -1], H - 4 - min(6, H - 4))
    y, top = np.arange(H)[None, :], r0[:, None]
    window = (y >= top) & (y < top + 4)
    chosen = window & ((s[:, None] >> np.clip(y - top, 0, 3)) & 1).astype(bool)  # full but for the well
    below = y >= top + 4
    prefull = below & ((p == 4) & (not adv))[:, None]  # full before the lock; else a support row
    debris = (y < top) & (y >= top - 2) & (y >= 1)  # two rows above the window, never row 0
    gap = (c[:, None] + 1 + rng.integers(0, W - 1, (n, H))) % W  # per row, a column other than the well's
    x = np.arange(W)[None, :, None]
    cells = rng.integers(0, 2, (n, W, H)).astype(bool)
    board = (window | below)[:, None, :] | (debris[:, None, :] & cells)
    board &= ~((x == gap[:, None, :]) & ((window & ~chosen) | (below & ~prefull) | debris)[:, None, :])
    board = np.where(x == c[:, None, None], below[:, None, :], board).astype(np.uint8)  # the well's column
    ncl = chosen.sum(axis=1) + prefull.sum(axis=1)
    land = r0 + 3
    ay = np.select([m == 1, m == 2], [np.maximum(0, land - 1), np.maximum(0, land - 3)], 0)
    counters = dict(holes=rng.integers(0, 40, n), piece_height=rng.integers(0, H, n),
                    score=rng.integers(0, 2**20 + 1, n), lines_cleared=np.full(n, 1000))
    return dict(board=board, c=c, ay=ay, ncl=ncl, counters=counters)


def crafted_actions(n):
    """Uniform actions with a hard drop on every odd step; the first steps of
    env i by m: hard drop / one row above the landing row / three rows above
    it / soft drop, then hard drop."""
    acts = O.splitmix64_actions(ACT_SEED, 0, T, n)
    acts[1::2] = 2
    m = _index_fields(n)[0]
    for k, head in {0: [2], 1: [6], 2: [6, 6, 6], 3: [3, 2]}.items():
        for t, a in enumerate(head):
            acts[t, m == k] = a
    return acts


def oracle_run(W, H, n, kw):
    """The oracle from the crafted state: its outputs of every step, its state
    at the start and after every step, which envs locked in each step, and
    for the envs that die in step 0 the board before the reset (step_one: the
    locked piece erased)."""
    cs = crafted_state(W, H, bool(kw.get("advanced_clears")))
    ob = O.OracleBatch(n, [SEED0 + e for e in range(n)], width=W, height=H, **kw)
    ob.reset()
    ob.boards()[:, :W, :H] = cs["board"][:n]
    cells = np.array(O.rotate_cells(O.BASE_SHAPES[5], 0), np.int32)
    ob.field("shape", (4, 2))[:] = cells
    ob.field("shape_id")[:] = 5
    ob.field("rot")[:] = 0
    ob.field("ax")[:] = cs["c"][:n]
    ob.field("ay")[:] = cs["ay"][:n]
    for k, v in cs["counters"].items():
        ob.field(k)[:] = v[:n]
    assert np.array_equal(ob.board(n - 1), cs["board"][n - 1]) and ob.envs[n - 1].ax == cs["c"][n - 1]
    assert [tuple(x) for x in ob.envs[n - 1].shape] == [tuple(x) for x in cells]  # the views wrote through
    start = bytes(ob.envs)
    acts = crafted_actions(n)
    init, state = ob.packed_state(), []
    out = record(ob, acts, after=lambda t, locked, pre: state.append(ob.packed_state()))
    out.update(ncl=cs["ncl"][:n], init=init, state=state)
    twin = O.OracleBatch(n, [0] * n, width=W, height=H, **kw)
    ctypes.memmove(ctypes.addressof(twin.envs), start, len(start))
    death_board = np.zeros((W, n), np.uint32)
    for i in np.nonzero(out["done"][0])[0]:
        _, _, d, _ = twin.step_one(int(i), int(acts[0, i]))
        assert d
        death_board[:, i] = pack_cols(twin.board(i))
    out["death_board"] = death_board
    return out


def _ref(W, H, scoring, **extra):
    """One oracle run per board and scoring, shared by the tests (read-only)."""
    return cached_ref(("lock_matrix", W, H, scoring, tuple(sorted(extra.items()))),
                      lambda: oracle_run(W, H, BOARDS[(W, H)], dict(SCORING[scoring], **extra)))


# ------------------------------------------------------------------ coverage
@pytest.mark.parametrize("scoring", sorted(SCORING))
@pytest.mark.parametrize("board", sorted(BOARDS), ids=_ids)
def test_crafted_stream_coverage(board, scoring):
    """Needs no GPU: what the matrix reaches is a property of the oracle run."""
    W, H = board
    ref = _ref(W, H, scoring)
    n = BOARDS[board]
    m, s, p, _ = _index_fields(n)
    died = ref["done"][0].astype(bool)
    gained = ref["stats"][0][:, 2] - 1000
    now = m < 2
    assert ref["locked"][0][now].all()
    # the constructed clear counts are the oracle's
    assert np.array_equal(gained[now & ~died], ref["ncl"][now & ~died])
    assert (gained[died] == 0).all()
    for k in (0, 1, 2):  # every nonempty subset of window rows
        assert set(s[now & ~died & (p == k)]) >= set(range(1, 16)), k
    counts = set(gained[now & ~died])
    assert counts >= set(range(0 if H > 4 else 1, 5)), counts  # 4x4: no clear, no survival
    if H >= 10 and scoring != "c4":
        assert counts >= set(range(6, 11)), counts  # rows full before the lock
    if scoring == "c4":
        assert max(counts) == 4  # advanced_clears: the score table ends there
    # a piece in row 0, or partly above the board, survives only by clearing
    top = now & (p == 2)
    assert np.array_equal(died[top], s[top] == 0)
    clipped = now & (p == 3)
    assert np.array_equal(died[clipped], s[clipped] & 14 == 0)
    for w0 in range(0, n, 64):  # lanes of one wave clear different row counts
        w = slice(w0, w0 + 64)
        assert len(set(gained[w][now[w]])) >= 3, w0
    assert not ref["locked"][0].reshape(-1, 4).all(axis=1).any()  # st_step's groups of 4 envs
    assert ref["locked"][0].reshape(-1, 4).any(axis=1).all()
    assert ref["locked"][:3].any(axis=0).all()  # the crafted locks fall on steps 0, 1 and 2


# ------------------------------------------------------------------ GPU side
def _upload(b, ref, sel=slice(None)):
    """The crafted state into a batch that was just reset (shape counts, the
    MT state and the preview stay the engine's own); env e takes the
    oracle's env sel[e]."""
    st = b.get_state(("board", "piece", "stats"))
    init = ref["init"]
    assert np.array_equal(st["stats"][6:13], init["stats"][6:13][:, sel])  # same first draws
    st["board"][:] = init["board"][:, sel]
    st["piece"][:] = init["piece"][sel]
    st["stats"][1:5] = init["stats"][1:5][:, sel]
    b.set_state(**st)


def _batch(board, scoring, autoreset="same_step", **extra):
    G = _engine()
    W, H = board
    n = BOARDS[board]
    ref = _ref(W, H, scoring, **extra)
    b = G.TetrisBatch(n, width=W, height=H, autoreset=autoreset, seeds=[SEED0 + e for e in range(n)],
                      **SCORING[scoring], **extra)
    b.reset()
    _upload(b, ref)
    return b, ref


SURFACE_CASES = [((10, 20), sf, sc) for sf in ("step", "f32", "wire", "vec", "gated")
                 for sc in ("c3", "c4", "hhh")] + \
    [(bd, sf, sc) for bd in ((6, 9), (4, 4), (5, 27), (32, 28)) for sf, sc in (("step", "c4"), ("step", "hhh"),
                                                                                ("vec", "c3"))] + \
    [((10, 20), "step_states", "c4")]


@pytest.mark.gpu
@pytest.mark.parametrize("board,surface,scoring", SURFACE_CASES, ids=_ids)
def test_step_surfaces(board, surface, scoring):
    """st_step, st_step_f32, st_step_wire + st_unwire, st_step_vec (with
    final_obs and info) and the gated st_step: every output of every step and
    the final state.  step / f32 take their actions from the host: checked
    there, the launch is not gated and runs st_step's own instantiation, the
    one with the late-loaded counters (score, lines and deaths as deltas, the
    old holes and height read per locking lane); from a device tensor step()
    gates the launch, which runs the vector env's instantiation ("gated").
    step_states also compares the state after each of the first three steps
    (get_state completes the MT generation and rewinds the preview, so that
    is a run of its own)."""
    W, H = board
    if surface == "vec":
        ref = _ref(W, H, scoring)
        target = _engine().TetrisVecEnv(BOARDS[board], width=W, height=H, seed=SEED0, obs_format="packed",
                                        **SCORING[scoring])
        target.reset()
        _upload(target.engine, ref)
    else:
        target, ref = _batch(board, scoring)

    def first_states(t):
        if surface == "step_states" and t < 3:
            check_engine_state(target, ref["state"][t], t)

    try:
        host = surface in ("step", "f32", "step_states")
        drive_surface(target, ref, "step" if surface == "step_states" else surface,
                      ref["acts"] if host else torch.as_tensor(ref["acts"].copy(), device=target.device),
                      on_step=first_states)
        check_engine_state(target, ref["state"][T - 1])
    finally:
        target.close()


@pytest.mark.gpu
@pytest.mark.parametrize("board,scoring", [((10, 20), "c4"), ((6, 9), "c3")], ids=_ids)
def test_no_autoreset_step_then_reset(board, scoring):
    """autoreset='none': step, then reset(done), equals the same reference;
    an env that dies in step 0 keeps its board minus the locked piece until
    the reset."""
    b, ref = _batch(board, scoring, autoreset="none")
    try:
        for t in range(T):
            obs, rew, dn = b.step(ref["acts"][t], obs="packed")  # (host actions: st_step ungated)
            check_step(ref, t, obs, rew, dn)
            done = ref["done"][t].astype(bool)
            if t == 0:
                assert done.any()
                got = b.get_state(("board",))["board"]
                assert np.array_equal(got[:, done], ref["death_board"][:, done]), "board of a dead env"
            if done.any():
                b.reset(torch.as_tensor(done.astype(np.uint8), device=b.device))
        check_engine_state(b, ref["state"][T - 1])
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["step", "rollout"])
def test_lock_delay(mode):
    """lock_delay=2 with step_reset: the crafted locks come after the delay,
    through st_step and through one rollout launch."""
    b, ref = _batch((10, 20), "c4", lock_delay=2, step_reset=True)
    try:
        assert ref["locked"][:6].any(axis=0).all() and not ref["locked"][:2].any()
        acts = torch.as_tensor(ref["acts"].copy(), device=b.device)
        if mode == "rollout":
            check_steps(ref, *b.rollout(acts, obs="packed"))
        else:
            drive_surface(b, ref, "step", ref["acts"])
        check_engine_state(b, ref["state"][T - 1])
    finally:
        b.close()


ROLLOUT_CASES = [(bd, sc, "packed") for bd in sorted(BOARDS) for sc in ("c4", "hhh")] + \
    [((10, 20), "c3", "packed"), ((10, 20), "c4", "f32")]


@pytest.mark.gpu
@pytest.mark.parametrize("split", [(16,), (2, 14)], ids=["one_launch", "2+14"])
@pytest.mark.parametrize("board,scoring,obs", ROLLOUT_CASES, ids=_ids)
def test_three_wave_rollout(board, scoring, obs, split):
    """k_rollout (lock_score): T steps in one launch, and as 2 + 14 -- the
    m = 2 lanes then lock on the first step after a state store and reload."""
    W, H = board
    assert BOARDS[board] <= 64 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
    b, ref = _batch(board, scoring)
    try:
        acts = torch.as_tensor(ref["acts"].copy(), device=b.device)
        t0 = 0
        for K in split:
            check_steps(ref, *b.rollout(acts[t0:t0 + K], obs=obs), t0=t0, H=H if obs == "f32" else None)
            t0 += K
        check_engine_state(b, ref["state"][T - 1])
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", ["c3", "c4"])
def test_two_wave_rollout(scoring):
    """k_rollout2 (step_logic with KSTEPS > 1; st_rollout above 4 workgroups
    per CU): env e runs crafted state e % 1280 with seed SEED0 + e % 1280, so
    the expectation is the oracle's first 1280 columns tiled."""
    G = _engine()
    W, H = 10, 20
    n0, K = 1280, 8
    n = 64 * 4 * torch.cuda.get_device_properties(0).multi_processor_count + 72
    ref = _ref(W, H, scoring)
    sel = np.arange(n) % n0
    b = G.TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[SEED0 + int(e) for e in sel],
                      **SCORING[scoring])
    try:
        b.reset()
        _upload(b, ref, sel)
        acts = torch.as_tensor(ref["acts"][:K][:, sel].copy(), device=b.device)
        check_steps(ref, *b.rollout(acts, obs="packed"), sel=sel)
        exp = ref["state"][K - 1]
        check_engine_state(b, dict(board=exp["board"][:, sel], piece=exp["piece"][sel], stats=exp["stats"][:, sel]))
    finally:
        b.close()
