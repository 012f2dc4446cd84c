"""st_step_export: st_step + st_export_env in one launch (k_step_export).

The fused launch is checked against the two launches it replaces, on twins
with equal seeds: after every step the record and the step's outputs are
identical, and at the end so is the whole state."""
import ctypes

import numpy as np
import pytest
import torch

from harness import assert_same_state, engine

pytestmark = pytest.mark.gpu

N = 300                   # stride 320: five workgroups, the last one ragged
ENVS = (0, 63, 64, 299)   # first / last lane of a workgroup, the next workgroup's first, the ragged one's last
CONFIGS = {               # one per instantiation of k_step_export
    "10x20_sc0": dict(),
    "10x20_scoring": dict(advanced_clears=True, penalise_holes_increase=True),
    "7x12_generic": dict(width=7, height=12),
}


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(b):
    return ctypes.c_void_p(torch.cuda.current_stream(b.device).cuda_stream)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_fused_equals_step_then_export(name):
    """One reference batch stepped with st_step + st_export_env of envs 0, 63,
    64 and 299, and one fused twin per env stepped with st_step_export: 150
    steps of gen_actions, then 700 hard drops (a spawn per step: every env's
    MT index and its preview's draw cross 624, the part of the record that is
    computed, not copied); `parts` cycles through its four values.  With
    parts = 0 the words past the head keep the buffer's fill."""
    G = engine()
    from gym_simpletetris_amd import _lib as C
    kw = CONFIGS[name]
    W, H = kw.get("width", 10), kw.get("height", 20)
    seeds = [500 + e for e in range(N)]
    ref = G.TetrisBatch(N, autoreset="same_step", seeds=seeds, **kw)
    twins = [G.TetrisBatch(N, autoreset="same_step", seeds=seeds, **kw) for _ in ENVS]
    for b in [ref] + twins:
        b.reset()
    L, s = ref._L, _stream(ref)
    nw = L.st_export_words(W, H)
    head = W + 2 + C.NSTAT
    rec_a = torch.empty((len(ENVS), nw), dtype=torch.int32, device=ref.device)
    rec_b = torch.empty_like(rec_a)
    drop = torch.full((N,), 2, dtype=torch.uint8, device=ref.device)
    crossed = 0
    last_idx = None
    for t in range(850):
        parts = t % 4
        acts = ref.gen_actions(t, 77) if t < 150 else drop
        rec_a.fill_(-7)
        rec_b.fill_(-7)
        C.check(L.st_step(ref._ctx, P(acts), P(ref.obs), P(ref.reward), P(ref.done), s))
        for k, env in enumerate(ENVS):
            C.check(L.st_export_env(ref._ctx, env, P(ref.obs), P(ref.reward), P(ref.done), parts, P(rec_a[k]), s))
            b = twins[k]
            C.check(L.st_step_export(b._ctx, P(acts), env, parts, P(rec_b[k]), P(b.obs), P(b.reward), P(b.done), s))
        assert torch.equal(rec_a, rec_b), (t, parts, (rec_a != rec_b).nonzero()[:8].tolist())
        for k, b in enumerate(twins):
            assert torch.equal(b.obs, ref.obs) and torch.equal(b.reward, ref.reward) \
                and torch.equal(b.done, ref.done), (t, ENVS[k])
        if parts == 0:
            assert bool((rec_b[:, head:] == -7).all()), t
        elif parts == C.EXPORT_MT:
            assert bool((rec_b[:, head + C.MT_N:] == -7).all()), t
        elif parts == C.EXPORT_OBS_F32:
            assert bool((rec_b[:, head:head + C.MT_N] == -7).all()), t
        idx = rec_b[:, W + 2 + C.STAT["mt_index"]].cpu().numpy()
        assert ((idx >= 0) & (idx <= 624)).all(), (t, idx)  # CPython's form
        if last_idx is not None:
            crossed += int((idx < last_idx).sum())  # the index wrapped: a new generation
        last_idx = idx
    assert crossed >= len(ENVS), crossed  # every exported env passed index 624
    for k, b in enumerate(twins):
        assert_same_state(ref, b, what=(name, ENVS[k]))
    for b in [ref] + twins:
        b.close()


def test_fused_single_env_pinned_record():
    """n = 1 with the record in pinned host memory mapped for the device: the
    single-env arrangement (TetrisEnv, TetrisEngine)."""
    G = engine()
    from gym_simpletetris_amd import _lib as C
    kw = dict(advanced_clears=True, penalise_height_increase=True)
    a = G.TetrisBatch(1, autoreset="none", seeds=[9], **kw)
    b = G.TetrisBatch(1, autoreset="none", seeds=[9], **kw)
    a.reset()
    b.reset()
    L, s = a._L, _stream(a)
    nw = L.st_export_words(10, 20)
    ra, rb = a._pinned(nw, torch.int32), b._pinned(nw, torch.int32)
    parts = C.EXPORT_MT | C.EXPORT_OBS_F32
    acts = [torch.full((1,), v, dtype=torch.uint8, device=a.device) for v in range(7)]
    rng = np.random.default_rng(3)
    deaths = 0
    for t in range(600):
        act = acts[int(rng.integers(0, 7)) if t < 250 else 2]
        C.check(L.st_step(a._ctx, P(act), P(a.obs), P(a.reward), P(a.done), s))
        C.check(L.st_export_env(a._ctx, 0, P(a.obs), P(a.reward), P(a.done), parts, ra.dst, s))
        C.check(L.st_step_export(b._ctx, P(act), 0, parts, rb.dst, P(b.obs), P(b.reward), P(b.done), s))
        for r in (ra, rb):
            if r.staged:
                r.land(s)
        C.check(L.st_stream_sync(s))
        ha, hb = ra.host.numpy(), rb.host.numpy()
        assert np.array_equal(ha, hb), (t, np.flatnonzero(ha != hb)[:8])
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), t
        if hb[11]:  # done: the caller resets (autoreset 'none')
            deaths += 1
            a.reset()
            b.reset()
    assert deaths > 0
    assert_same_state(a, b)
    a.close()
    b.close()


def test_fused_error_paths_and_gate():
    """Bad arguments are refused before any launch; the call is not gated and
    leaves an armed gate to the next st_step."""
    G = engine()
    from gym_simpletetris_amd import _lib as C
    n = 300
    a = G.TetrisBatch(n, autoreset="same_step", seeds=range(n))
    b = G.TetrisBatch(n, autoreset="same_step", seeds=range(n))
    a.reset()
    b.reset()
    L, s = a._L, _stream(a)
    rec = torch.zeros(L.st_export_words(10, 20), dtype=torch.int32, device=a.device)
    good = a.gen_actions(0, 5).clone()
    args = lambda env, parts, obs: (a._ctx, P(good), env, parts, P(rec), obs, P(a.reward), P(a.done), s)  # noqa: E731
    before = {k: v.copy() for k, v in a.get_state().items()}
    for env, parts, obs in ((n, 0, P(a.obs)), (-1, 0, P(a.obs)), (0, 4, P(a.obs)), (0, 0, None)):
        assert L.st_step_export(*args(env, parts, obs)) == C.ST_EINVAL, (env, parts)
    assert L.st_step_export(a._ctx, P(good), 0, 0, None, P(a.obs), P(a.reward), P(a.done), s) == C.ST_EINVAL
    assert_same_state(before, a, "a refused call changed the state")
    # a fresh context: ST_ESTATE before st_seed + st_reset
    fresh = G.TetrisBatch(4)
    fa = torch.zeros(4, dtype=torch.uint8, device=fresh.device)
    call = lambda: L.st_step_export(fresh._ctx, P(fa), 0, 0, P(rec), P(fresh.obs), P(fresh.reward),  # noqa: E731
                                    P(fresh.done), s)
    assert call() == C.ST_ESTATE
    fresh.seed(range(4))
    assert call() == C.ST_ESTATE  # seeded, never reset
    fresh.close()
    # a gate armed on bad actions: st_step_export steps all the same (it is
    # not gated) and the gate stays for the next st_step, which it shuts
    bad = good.clone()
    bad[7] = 9
    assert L.st_gate_actions(a._ctx, P(bad), s) == 0
    C.check(L.st_step_export(*args(5, 0, P(a.obs))))
    b.step(good)
    torch.cuda.synchronize()
    assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward)
    assert_same_state(a, b, "the ungated fused step")
    C.check(L.st_step(a._ctx, P(bad), P(a.obs), P(a.reward), P(a.done), s))  # gated: skipped
    assert L.st_gate_wait(a._ctx) == 1
    assert_same_state(a, b, "the gated step behind it changed nothing")
    assert L.st_gate_wait(a._ctx) == C.ST_ESTATE
    a.close()
    b.close()
