"""The inputs of test_gpu_call_sequences.py, judged on the oracle alone: for
every (config, seed) the GPU test runs, the model is driven through the op
list without an engine, and the sequence must be one in which the hand-offs
under test really occur.  These are conditions on the inputs, read from the
oracle's own record; none of them reads the code under test.

A sequence that misses one is mended in sequence_ref.CONFIGS -- start indices,
seeds, op counts, the placement runs of the configs whose pieces lock late --
never by changing a bound here.  (Consecutive locks of one env need
lock_delay <= 0 or a placement step, which sets the lock counter so that the
hard drop locks: the lock_delay 2 and 5 configs reach condition 7 through
runs of placement steps, and draw `placements` more often for it.)
"""
import numpy as np
import pytest

import sequence_ref as SR

CASES = [(cid, seed) for cid in SR.CONFIGS for seed in SR.CONFIGS[cid]["seeds"]]
_RUNS = {}


def _run(cid, seed):
    if (cid, seed) not in _RUNS:
        ops = SR.make_ops(cid, seed)
        _RUNS[cid, seed] = ops, SR.run(ops, SR.Model(cid, seed))
    return _RUNS[cid, seed]


@pytest.mark.parametrize("cid,seed", CASES)
def test_ops_are_deterministic_and_prefix_stable(cid, seed):
    """1. make_ops gives the same list twice, and a prefix of it for a smaller n_ops."""
    ops = SR.make_ops(cid, seed)
    assert ops == SR.make_ops(cid, seed) and len(ops) == SR.CONFIGS[cid]["n_ops"]
    for k in (1, len(ops) // 3, len(ops) - 1):
        assert SR.make_ops(cid, seed, k) == ops[:k], k
    assert all(isinstance(op, tuple) and all(isinstance(a, (str, int)) for a in op) for op in ops)
    assert SR.make_ops(cid, seed + 1) != ops


@pytest.mark.parametrize("cid,seed", CASES)
def test_every_kind_occurs_twice(cid, seed):
    """2. Every op kind of the config's list at least twice per sequence."""
    ops, _ = _run(cid, seed)
    count = {}
    for op in ops:
        count[op[0]] = count.get(op[0], 0) + 1
    st, fm, rd = SR.kinds(cid)
    assert len(st) >= 5 and fm and rd
    for kind in st + fm + rd + ("checkpoint",) * ("checkpoint" in SR.bag_of(cid)):
        assert count.get(kind, 0) >= 2, (kind, count.get(kind, 0))


@pytest.mark.parametrize("cid,seed", CASES)
def test_most_envs_cross_a_generation_end(cid, seed):
    """3. At least 80% of the envs cross: the oracle's rng.index decreases across a state-changing op."""
    _, m = _run(cid, seed)
    assert m.crossed.mean() >= 0.8, m.crossed.mean()
    start = SR.start_indices(cid, m.n)
    assert ((start >= 0) & (start <= SR.MT_N)).all() and np.array_equal(start, m.start)


@pytest.mark.parametrize("cid", sorted(SR.CONFIGS))
def test_every_kind_meets_a_generation_end(cid):
    """4. Over a config's seeds every state-changing kind has an instance in
    which an env crosses; 5. every form-changing and read-only kind has one
    executed while an env's index is within kMtWin words of 624 (its draw
    window then reads into the successor)."""
    st, fm, rd = SR.kinds(cid)
    crossing, near = set(), set()
    for seed in SR.CONFIGS[cid]["seeds"]:
        for e in _run(cid, seed)[1].log:
            if e["crossed"].any():
                crossing.add(e["kind"])
            if e["near"]:
                near.add(e["kind"])
    assert not set(st) - crossing, sorted(set(st) - crossing)
    assert not set(fm + rd) - near, sorted(set(fm + rd) - near)


@pytest.mark.parametrize("cid,seed", CASES)
def test_deaths_and_consecutive_locks(cid, seed):
    """6. At least 10 deaths; under autoreset 'none' at least 5 masked resets
    that hit a dead env.  7. At least 5% of env-steps lock right after a lock
    of the same env: the same-launch pick, as in
    test_gpu_prologue_draw.py::test_lock_without_preview_is_common."""
    _, m = _run(cid, seed)
    assert m.deaths >= 10, m.deaths
    if m.none:
        assert m.dead_resets >= 5, m.dead_resets
    assert m.env_steps > 0 and m.lock_pairs / m.env_steps >= 0.05, m.lock_pairs / m.env_steps


def test_config_table():
    """The configs are the ones the hand-offs differ in: the wire alignments,
    the lock_delay range and the fork source whose lock counters exceed the
    target's lock_delay."""
    C = SR.CONFIGS
    assert (7 * 9) % 32 == 31 and C["7x9_lock2"]["board"] == (7, 9)      # done is bit 31 of the last wire word
    assert (8 * 4) % 32 == 0 and C["8x4_extreme"]["board"] == (8, 4)     # the reward word-aligned, done alone
    assert C["10x20_lock5"]["kw"]["lock_delay"] > SR.REACH_MAX_LOCK and C["6x9_lockneg"]["kw"]["lock_delay"] < 0
    m = SR.Model("10x20_lock5", 1)
    assert (m.alt.field("lock") > C["10x20_lock5"]["kw"]["lock_delay"]).sum() >= m.n // 2
    assert SR.n_envs("10x20_two_wave", 256) == 65537
    for cid in C:
        lanes = np.arange(SR.n_envs(cid)) % 64
        start = SR.start_indices(cid, SR.n_envs(cid))
        assert start[lanes >= 4].max() == SR.MT_N and start[lanes < 4].max() < SR.MT_N
