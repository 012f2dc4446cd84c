"""The timed bench workload itself, at full size and over the bench's horizon,
bit-exact against the C oracle (VERDICT r1 "next" #1).

bench.py times 65,536 envs (seeds 1000 + e), synthetic actions
splitmix64(0x5EED ^ (t << 32 ^ e)) % 7, same-step auto-reset, W eager warm-up
st_step launches and then K st_step launches captured in one hipGraph.  These
tests run exactly that (W = 100, K = 4,000: a second MT generation switch for
most envs, boards at full occupancy, every auto-reset path) with each step's
outputs written to its own slot, and compare every step's reward, done and
packed obs, then the final board / piece / counters / MT19937 state, with the
oracle (TetrisEngine.step restated, tetris_env.py:243-304; CPython's random,
:183-191), for BASELINE configs C3 and C4.  The same for st_rollout: 10
launches of 100 steps.  The oracle runs on host threads over env slices
(ctypes releases the GIL), so the check takes seconds.
"""
import ctypes

import numpy as np
import pytest
import torch

from harness import ASEED, C4, SEED_BASE, ParallelOracle, check_engine_state, mt_twist
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N, W, H = 65536, 10, 20
WU, K = 100, 4000
CONFIGS = {"c3": dict(), "c4": C4}


def _seeded_words(n):
    """random.seed(SEED_BASE + e) words of every env (the oracle's seeding)."""
    out = np.empty((n, 624), np.uint32)
    for e in range(n):
        out[e] = np.ctypeslib.as_array(O.MTRandom(SEED_BASE + e)._mt.mt)
    return out


def _check_final(eng, orc):
    exp = orc.packed_state()
    check_engine_state(eng, exp)
    st = eng.get_state(("stats", "mt"))  # st_mt_sync first: CPython's exact MT state
    assert np.array_equal(st["stats"][13], exp["mt_index"]), "MT index"
    assert np.array_equal(st["mt"], exp["mt"]), "MT words"


def _compare(t0, got_r, got_d, got_o, ref):
    assert np.array_equal(got_r, ref["reward"]), f"reward, steps {t0}.."
    assert np.array_equal(got_d.astype(np.uint8), ref["done"]), f"done, steps {t0}.."
    bad = np.argwhere((got_o.transpose(0, 2, 1) != ref["obs"]).any(axis=2))
    assert bad.size == 0, f"obs mismatch at (step, env) {bad[:4] + [t0, 0]}"


def _bench_batch(n, kw, T):
    """bench.py's batch of n envs on cuda:0 and T rows of its action stream
    (generated ahead of the reset, as the bench does)."""
    import gym_simpletetris_amd as G
    dev = torch.device("cuda", 0)
    eng = G.TetrisBatch(n, autoreset="same_step", seeds=[SEED_BASE + e for e in range(n)],
                        device=dev, width=W, height=H, **kw)
    acts = torch.empty((T, n), dtype=torch.uint8, device=dev)
    for t in range(T):
        eng.gen_actions(t, ASEED, out=acts[t])
    eng.reset()
    return eng, acts, dev


def _st_step(eng, acts, obs, rew, done, t, sp):
    """One st_step launch at the C ABI: step t's outputs into their own slot."""
    from gym_simpletetris_amd import _lib as C
    vp = ctypes.c_void_p
    C.check(eng._L.st_step(eng._ctx, vp(acts[t].data_ptr()), vp(obs[t].data_ptr()), vp(rew[t].data_ptr()),
                           vp(done[t].data_ptr()), sp))


def _compare_slots(orc, obs, rew, done, CH):
    """Every step's slot against the oracle, CH steps at a time."""
    T = len(rew)
    for t0 in range(0, T, CH):
        t1 = min(t0 + CH, T)
        _compare(t0, rew[t0:t1].cpu().numpy(), done[t0:t1].cpu().numpy(), obs[t0:t1].cpu().numpy().view(np.uint32),
                 orc.rollout(t0, t1 - t0))


@pytest.mark.parametrize("config,launch", [("c3", "eager"), ("c3", "graph"), ("c4", "eager")])
def test_bench_workload_st_step(config, launch):
    """bench.py's headline region (eager: the default; graph: `--launch
    graph`, K launches captured in one hipGraph and replayed).  In the graph
    case the outputs of the timed steps hold a sentinel after the capture
    (capturing runs nothing) and the oracle's values after the replay: the
    compared steps really came from the graph."""
    kw = CONFIGS[config]
    T = WU + K
    eng, acts, dev = _bench_batch(N, kw, T)
    SENT = -12345
    obs = torch.full((T, W, N), SENT, dtype=torch.int32, device=dev)
    rew = torch.full((T, N), SENT, dtype=torch.int32, device=dev)
    done = torch.full((T, N), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    sp = ctypes.c_void_p(s.cuda_stream)
    with torch.cuda.stream(s):
        for t in range(WU):  # bench warm-up: eager launches
            _st_step(eng, acts, obs, rew, done, t, sp)
    torch.cuda.synchronize(dev)
    if launch == "graph":
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):  # bench --launch graph: one graph of K launches
            for t in range(WU, T):
                _st_step(eng, acts, obs, rew, done, t, sp)
        torch.cuda.synchronize(dev)
        # captured, not run: every timed step's outputs still hold the sentinel
        assert bool((rew[WU:] == SENT).all()) and bool((obs[WU:] == SENT).all()) and bool((done[WU:] == 7).all())
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize(dev)
        del g
    else:
        assert launch == "eager"
        with torch.cuda.stream(s):  # bench default: K eager launches
            for t in range(WU, T):
                _st_step(eng, acts, obs, rew, done, t, sp)
        torch.cuda.synchronize(dev)
    assert not bool((rew == SENT).any()) and not bool((done == 7).any())
    orc = ParallelOracle(N, kw)
    try:
        _compare_slots(orc, obs, rew, done, 100)
        _check_final(eng, orc)
        # the regime the bench times: most envs went past their first generation
        fin = orc.final_state()["rng"]["mt"].astype(np.uint32)
        gen1 = mt_twist(_seeded_words(N))
        assert (fin != gen1).any(axis=1).mean() > 0.5
    finally:
        orc.close()
        eng.close()


def test_c2_shape_eager_long():
    """BASELINE C2 at its own shape: 4,096 10x20 boards, C3 (default)
    rewards, same-step auto-reset, 1,200 eager st_step launches (one per
    step, as bench.py times C2), every step's reward / done / packed obs and
    the final state bit-exact against the oracle."""
    n, T = 4096, 1200
    eng, acts, dev = _bench_batch(n, {}, T)
    obs = torch.empty((T, W, n), dtype=torch.int32, device=dev)
    rew = torch.empty((T, n), dtype=torch.int32, device=dev)
    done = torch.empty((T, n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for t in range(T):
        _st_step(eng, acts, obs, rew, done, t, sp)
    torch.cuda.synchronize(dev)
    orc = ParallelOracle(n, {})
    try:
        _compare_slots(orc, obs, rew, done, 200)
        _check_final(eng, orc)
        assert int(done.sum()) > n  # episodes turned over inside the compared span
    finally:
        orc.close()
        eng.close()


def _rollouts_vs_oracle(n, kw, CH, NL):
    """NL st_rollout launches of CH steps: every step's outputs and the final
    state against the oracle."""
    eng, acts, _ = _bench_batch(n, kw, CH * NL)
    orc = ParallelOracle(n, kw)
    buf = {}
    try:
        for c in range(NL):
            o, r, d = eng.rollout(acts[c * CH:(c + 1) * CH], obs="packed", out=buf)
            ref = orc.rollout(c * CH, CH)
            _compare(c * CH, r.cpu().numpy(), d.cpu().numpy(), o.cpu().numpy().view(np.uint32), ref)
        _check_final(eng, orc)
    finally:
        orc.close()
        eng.close()


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_bench_workload_st_rollout(config):
    _rollouts_vs_oracle(N, CONFIGS[config], 100, 10)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_rollout_large_batch_two_wave_kernel(config):
    """st_rollout above 4 workgroups per CU runs the two-wave rollout kernel
    (launch_rollout's choice; the three-wave kernel below it): 2x the CUs'
    4-workgroup batch plus a ragged tail, 3 launches x 100 steps, every step's
    outputs and the final state bit-exact against the oracle."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 4 * 64 * cus + 37
    assert n > 4 * 64 * cus
    _rollouts_vs_oracle(n, CONFIGS[config], 100, 3)


@pytest.mark.parametrize("n,steps", [(65537, 600), (1 << 20, 24)])
def test_ragged_and_large_batches(n, steps):
    """A ragged batch (65,537 envs: the last wave holds one real env, the
    stride is padded) over 600 graph-replayed steps, and 2^20 envs (16x the
    headline batch) over 24 steps, both bit-exact vs the oracle, C4 scoring."""
    kw = CONFIGS["c4"]
    eng, acts, dev = _bench_batch(n, kw, steps)
    obs = torch.empty((steps, W, n), dtype=torch.int32, device=dev)
    rew = torch.empty((steps, n), dtype=torch.int32, device=dev)
    done = torch.empty((steps, n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for t in range(steps):
            _st_step(eng, acts, obs, rew, done, t, ctypes.c_void_p(s.cuda_stream))
    with torch.cuda.stream(s):
        g.replay()
    torch.cuda.synchronize(dev)
    del g
    orc = ParallelOracle(n, kw)
    try:
        _compare_slots(orc, obs, rew, done, 100)
        _check_final(eng, orc)
    finally:
        orc.close()
        eng.close()


def test_soak_many_generations():
    """100,000 steps of 8,192 envs (st_rollout, 1,000 steps per launch): ~40
    MT generation switches and ~1,800 episodes per env; every step's
    reward and done, then the final board / piece / counters / MT state,
    bit-exact against the oracle (C4 scoring)."""
    import gym_simpletetris_amd as G
    n, T, CH = 8192, 100000, 1000
    kw = CONFIGS["c4"]
    eng = G.TetrisBatch(n, autoreset="same_step", seeds=[SEED_BASE + e for e in range(n)],
                        width=W, height=H, **kw)
    eng.reset()
    orc = ParallelOracle(n, kw)
    acts = torch.empty((CH, n), dtype=torch.uint8, device=eng.device)
    try:
        deaths = 0
        for t0 in range(0, T, CH):
            for t in range(CH):
                eng.gen_actions(t0 + t, ASEED, out=acts[t])
            _, r, d = eng.rollout(acts, obs="none")
            ref = orc.rollout(t0, CH, obs=False)
            assert np.array_equal(r.cpu().numpy(), ref["reward"]), f"reward, steps {t0}.."
            dn = d.cpu().numpy().astype(np.uint8)
            assert np.array_equal(dn, ref["done"]), f"done, steps {t0}.."
            deaths += int(dn.sum())
        _check_final(eng, orc)
        assert deaths > 1000 * n  # the episodes really turned over
        fin = orc.final_state()["rng"]["mt"].astype(np.uint32)
        gen = mt_twist(_seeded_words(n))
        for _ in range(12):  # far past them: none of the first twelve generations remains
            assert not (fin == gen).all(axis=1).any()
            gen = mt_twist(gen)
    finally:
        orc.close()
        eng.close()
