"""st_step's draw in the prologue: a lock leaves the MT word without a preview,
and the next st_step's draw wave fills it before the lock ballot.

So "no valid preview" is no longer the rare state after st_seed / st_mt_sync:
every env is in it for the step after each of its locks, an env that locks
twice in a row takes its piece from the draw wave's pick of the same launch,
and every other kernel (rollouts, the reset, the placement step, the export
record, st_mt_sync, save / load) meets such states all the time.  Every case
here runs against the C oracle on every step."""
import ctypes

import numpy as np
import pytest
import torch

import placement_ref as P
from harness import (C4, batch_and_oracle, cached_ref, check_engine_state, check_mt_state, check_step, check_steps,
                     drive_surface, engine, record)
from gym_simpletetris_amd.engine import unwire
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SEED0 = 8800
DROP_SEED = 5      # chosen on the CPU: the oracle meets the 5% bound below for every config here
SCORING = {"c3": {}, "c4": C4}


def drop_heavy(T, n, seed=DROP_SEED):
    """actions [T, n]: about half hard drops, the rest uniform over the seven actions."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((T, n)) < 0.5, 2, rng.integers(0, 7, (T, n))).astype(np.uint8)


def _ref(n, T, scoring, **kw):
    def make():
        ob = O.OracleBatch(n, [SEED0 + e for e in range(n)], **SCORING[scoring], **kw)
        ob.reset()
        out = record(ob, drop_heavy(T, n))
        out["final"], out["ob"] = ob.packed_state(), ob
        return out
    return cached_ref(("prologue_draw", n, T, scoring, tuple(sorted(kw.items()))), make)


def _batch(n, scoring, autoreset="same_step", **kw):
    b = engine().TetrisBatch(n, autoreset=autoreset, seeds=[SEED0 + e for e in range(n)], **SCORING[scoring], **kw)
    b.reset()
    return b


def lock_after_lock(ref):
    """Share of env-steps that lock in the step right after a lock of the same env."""
    lk = ref["locked"]
    return float((lk[1:] & lk[:-1]).mean())


# ------------------------------------------------------------------ 1. locking without a preview is common
@pytest.mark.parametrize("scoring", ["c3", "c4"])
def test_lock_without_preview_is_common(scoring):
    """10x20, n = 100 (two workgroups, the second ragged), same-step auto-reset,
    400 steps of the drop-heavy stream through st_step (host actions: the
    ungated k_step).  At least 5% of env-steps lock right after a lock -- a
    condition on the inputs, from the oracle's own record: those steps take
    the piece the draw wave picked in the same launch (pick1 / f2)."""
    n, T = 100, 400
    ref = _ref(n, T, scoring)
    assert lock_after_lock(ref) >= 0.05, lock_after_lock(ref)
    b = _batch(n, scoring)
    try:
        drive_surface(b, ref, "step", ref["acts"])
        check_engine_state(b, ref["final"])
        check_mt_state(b, ref["ob"])
    finally:
        b.close()


# ------------------------------------------------------------------ 2. generation switch
def test_generation_switch():
    """n = 64 on the same kind of stream until the oracle shows that every env
    has refilled its 624 words at least once; the MT state after st_mt_sync
    once mid-run (when half the envs have switched: previews missing and
    drawn across a switch, successors built by the chunks and finished by
    draws) and at the end."""
    n, cap = 64, 3000
    b, ob = batch_and_oracle(n, [SEED0 + 500 + e for e in range(n)])
    acts = drop_heavy(cap, n, DROP_SEED + 1)
    idx = np.ctypeslib.as_array(ob.envs)["rng"]["index"]
    wrapped, last, mid_done, t = np.zeros(n, bool), idx.copy(), False, 0
    try:
        while not wrapped.all():
            assert t < cap, "the oracle's envs did not all refill within the cap"
            check_step(ob.rollout(acts[t:t + 1]), 0, *b.step(acts[t]), at=t)
            wrapped |= idx < last
            last = idx.copy()
            if not mid_done and wrapped.sum() >= n // 2:
                check_mt_state(b, ob, ("mid", t))
                mid_done = True
            t += 1
        assert mid_done
        check_engine_state(b, ob.packed_state())
        check_mt_state(b, ob, "end")
    finally:
        b.close()


# ------------------------------------------------------------------ 3. hand-offs between kernels on one context
def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _handoffs(n, n_slots_envs):
    """One context (a TetrisVecEnv's engine) through st_step x5, st_rollout of
    7, st_step_vec with final_obs and info, st_step_f32, st_step_wire,
    st_step_export and a placement step, with st_mt_sync and a save / load in
    the middle, twice round; the oracle on every step.  The first
    n_slots_envs envs take random placement slots (per-env oracle commits),
    the rest slot -1: the hard drop from where the piece is, which the
    oracle's batch step gives."""
    from gym_simpletetris_amd import _lib as C
    G = engine()
    seeds = [SEED0 + 900 + e for e in range(n)]
    venv = G.TetrisVecEnv(n, seed=seeds[0], obs_format="packed")
    venv.reset()
    b = venv.engine
    k = n_slots_envs
    oa = O.OracleBatch(k, seeds[:k])
    ob = O.OracleBatch(n - k, seeds[k:]) if n > k else None
    for o in (oa, ob):
        if o is not None:
            o.reset()
    W, H, S = 10, 20, 4 * 16
    rng = np.random.default_rng(31)
    acts = drop_heavy(64, n, DROP_SEED + 2)
    dev = b.device
    state = dict(t=0)

    def oracle(K):
        t = state["t"]
        rs = [o.rollout(acts[t:t + K, lo:lo + o.n]) for o, lo in ((oa, 0), (ob, k)) if o is not None]
        state["t"] = t + K
        return {f: np.concatenate([r[f] for r in rs], axis=1) for f in ("obs", "reward", "done", "stats")}, \
            torch.as_tensor(acts[t:t + K], device=dev)

    rec = torch.empty(b._L.st_export_words(W, H), dtype=torch.int32, device=dev)
    try:
        for rnd in range(2):
            ref, a = oracle(5)
            for j in range(5):
                check_step(ref, j, *b.step(acts[state["t"] - 5 + j]), at=("step", rnd, j))  # host actions: k_step
            ref, a = oracle(7)
            check_steps(ref, *b.rollout(a))
            ref, a = oracle(1)
            drive_surface(venv, ref, "vec", a)
            if rnd == 0:
                b.sync_mt()
            ref, a = oracle(1)
            f32, rew, dn = b.step(a[0], obs="f32")
            check_step(ref, 0, f32, rew, dn, H=H, at=("f32", rnd))
            ref, a = oracle(1)
            check_step(ref, 0, *unwire(b.step_wire(a[0]), W, H), at=("wire", rnd))
            if rnd == 0:
                b.load(b.save())
            ref, a = oracle(1)
            C.check(b._L.st_step_export(b._ctx, _P(a[0]), n - 1, C.EXPORT_MT, _P(rec), _P(b.obs), _P(b.reward),
                                        _P(b.done), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            check_step(ref, 0, b.obs, b.reward, b.done, at=("export", rnd))
            # the placement step
            slots = np.full(n, -1, np.int64)
            slots[:k] = rng.integers(-2, S + 2, k)
            rows = [P.ref_place_step(oa, i, slots[i], "same_step") for i in range(k)]
            pref = dict(obs=np.stack([r[0] for r in rows])[None], reward=np.array([r[1] for r in rows], np.int32)[None],
                        done=np.array([r[2] for r in rows], np.uint8)[None])
            if ob is not None:
                r2 = ob.rollout(np.full((1, n - k), 2, np.uint8))
                pref = {f: np.concatenate([pref[f], r2[f]], axis=1) for f in pref}
            check_step(pref, 0, *b.step_placements(slots), at=("placements", rnd))
            assert np.array_equal(b.placed.cpu().numpy()[:k], np.array([r[3] for r in rows], np.uint8))
        # the end: the whole state and the MT state of both oracle parts
        st = b.get_state(("board", "piece", "stats", "mt"))
        lo = 0
        for o in (oa, ob):
            if o is None:
                continue
            hi, exp = lo + o.n, o.packed_state()
            rngs = np.ctypeslib.as_array(o.envs)["rng"]
            assert np.array_equal(st["board"][:, lo:hi], exp["board"]), "board"
            assert np.array_equal(st["piece"][lo:hi], exp["piece"]), "piece"
            assert np.array_equal(st["stats"][:13, lo:hi], exp["stats"]), "counters"
            assert np.array_equal(st["stats"][13, lo:hi], rngs["index"]), "MT index"
            assert np.array_equal(st["mt"][lo:hi], rngs["mt"]), "MT words"
            lo = hi
    finally:
        venv.close()


def test_handoffs_three_wave_rollout():
    """n = 100: the two-wave st_step and the three-wave k_rollout."""
    _handoffs(100, 100)


def test_handoffs_two_wave_rollout():
    """The smallest n at which st_rollout launches k_rollout2 (above 4
    workgroups per CU), which shares step_logic / step_draw with st_step."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _handoffs(64 * 4 * cus + 1, 100)


# ------------------------------------------------------------------ 4. auto-reset off
def test_autoreset_off_masked_reset():
    """autoreset='none': an env that dies keeps (or, having drawn in this very
    launch, gains) its valid preview; the masked st_reset behind the step
    spawns it; stepping goes on bit-exactly.  The oracle resets on done, which
    is the same game."""
    n, T = 100, 300
    ref = _ref(n, T, "c4")
    assert ref["done"].sum() >= 20
    b = _batch(n, "c4", autoreset="none")
    try:
        def reset_dead(t):
            if ref["done"][t].any():
                b.reset(torch.as_tensor(ref["done"][t].copy(), device=b.device))
        drive_surface(b, ref, "step", ref["acts"][:T], on_step=reset_dead)
        check_engine_state(b, ref["final"])
        check_mt_state(b, ref["ob"])
    finally:
        b.close()


# ------------------------------------------------------------------ 5. lock_delay = 2
def test_lock_delay_two():
    """lock_delay = 2, n = 64, 200 steps: locks come two steps after the piece
    lands, so previews are filled long before they spawn."""
    n, T = 64, 200
    ref = _ref(n, T, "c3", lock_delay=2)
    assert ref["locked"].any()
    b = _batch(n, "c3", lock_delay=2)
    try:
        drive_surface(b, ref, "step", ref["acts"])
        check_engine_state(b, ref["final"])
        check_mt_state(b, ref["ob"])
    finally:
        b.close()
