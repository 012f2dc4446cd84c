"""Box-column piece descriptors in the one-launch-per-step kernels (step_logic
and step_draw: st_step, st_step_vec, st_step_wire, st_step_f32 and the
two-wave rollout) and the step rules they share with the three-wave rollout.

A rotation is read, painted and erased as four consecutive board columns from
its leftmost one, so a piece held against a wall reaches into the pad columns
beside the board.  Uniform random actions rarely hold a piece there in every
rotation; the action pattern below does, per env: a run of left or right
moves, a run of rotations (either order, either sense) and a hard drop, with
same-step auto-reset.  Every output of every step and the state after the
last step are bit-exact against the C oracle."""
import numpy as np
import pytest
import torch

from harness import (C4, assert_same_state, cached_ref, check_engine_state, check_steps, drive_surface,
                     engine as _engine, record, wall_pattern)
from oracle import oracle as O

T = 200
SEED0 = 4242
# n: whole workgroups on the 16-byte store path and a last, partial one on
# the per-env path; 10x20 the fixed-size kernel, 6x9 / 4x4 the generic one,
# 5x27 the generic one with H > 25 (64-bit cell shifts)
BOARDS = {(10, 20): 1000, (6, 9): 300, (4, 4): 300, (5, 27): 300}


def oracle_run(W, H, n, kw):
    """The oracle's outputs for the wall pattern, its state after the last
    step, and the coverage of the locks by hard drop (the piece locks where
    it stood before the step, so the oracle's piece state before the step is
    the locked pose): (shape, rotation) -> locks with a cell in column 0 /
    in column W - 1, and locks of a one-column rotation in column W - 1."""
    ob = O.OracleBatch(n, [SEED0 + e for e in range(n)], width=W, height=H, **kw)
    ob.reset()
    acts = wall_pattern(W, T, n)
    cover = dict(left=np.zeros((7, 4), np.int64), right=np.zeros((7, 4), np.int64), thin_right=0)

    def pose(t):
        return (ob.field("shape_id").copy(), ob.field("rot").copy(),
                ob.field("ax")[:, None] + ob.field("shape", (4, 2))[:, :, 0])

    def count(t, locked, pre):
        sid, rot, cols = pre
        locked = locked & (acts[t] == 2)
        at_l = locked & (cols.min(axis=1) == 0)
        at_r = locked & (cols.max(axis=1) == W - 1)
        np.add.at(cover["left"], (sid[at_l], rot[at_l] & 3), 1)
        np.add.at(cover["right"], (sid[at_r], rot[at_r] & 3), 1)
        cover["thin_right"] += int((at_r & (cols.min(axis=1) == cols.max(axis=1))).sum())

    out = record(ob, acts, before=pose, after=count)
    out.update(cover, final=ob.packed_state())
    return out


def _ref(W, H, kw_name="c3"):
    """One oracle run per board and scoring, shared by the tests (read-only)."""
    return cached_ref(("box_descriptors", W, H, kw_name),
                      lambda: oracle_run(W, H, BOARDS[(W, H)], C4 if kw_name == "c4" else {}))


def _batch(board, scoring="c3"):
    W, H = board
    n = BOARDS[board]
    b = _engine().TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[SEED0 + e for e in range(n)],
                              **(C4 if scoring == "c4" else {}))
    b.reset()
    return b, _ref(W, H, scoring)


def _assert_coverage(ref):
    """The condition the stream has to meet, from the oracle alone (10x20):
    every (shape, rotation) locks with a cell in column 0 and with a cell in
    column W - 1, and a one-column rotation (the vertical I) locks in column
    W - 1 -- its box lies in the right pad columns but for its first column."""
    assert (ref["left"] > 0).all(), ref["left"]
    assert (ref["right"] > 0).all(), ref["right"]
    assert ref["thin_right"] > 0
    assert ref["done"].sum() > 0  # same-step resets inside the span


def test_wall_pattern_covers_every_rotation_at_both_walls():
    """Needs no GPU: the stream's coverage is a property of the oracle run."""
    _assert_coverage(_ref(10, 20))


@pytest.mark.gpu
@pytest.mark.parametrize("surface", ["step", "f32", "wire", "vec"])
@pytest.mark.parametrize("board", sorted(BOARDS))
def test_every_step_surface_vs_oracle(board, surface):
    """st_step, st_step_f32, st_step_wire + st_unwire and st_step_vec (with
    final_obs and info) on the same stream: obs, reward and done of every
    step, the vector env's terminal obs and counters, and the final state.
    Every surface takes its actions from a device tensor."""
    W, H = board
    if surface == "vec":
        ref = _ref(W, H)
        target = _engine().TetrisVecEnv(BOARDS[board], width=W, height=H, seed=SEED0, obs_format="packed")
        target.reset()
    else:
        target, ref = _batch(board)
    if board == (10, 20):
        _assert_coverage(ref)
    try:
        drive_surface(target, ref, surface, torch.as_tensor(ref["acts"].copy(), device=target.device))
        check_engine_state(target, ref["final"])  # (a board row the store phase wrongly took for clean shows here)
    finally:
        target.close()


@pytest.mark.gpu
def test_step_scoring_flags_vs_oracle():
    """The same stream with C4's scoring flags (the non-SC0 instantiation of
    the fixed-size kernel: late counters feed the height / holes rewards)."""
    b, ref = _batch((10, 20), "c4")
    try:
        drive_surface(b, ref, "step", torch.as_tensor(ref["acts"].copy(), device=b.device))
        check_engine_state(b, ref["final"])
    finally:
        b.close()


@pytest.mark.gpu
def test_two_wave_rollout_equals_steps():
    """k_rollout2 (st_rollout above 4 workgroups per CU) at the smallest env
    count that selects it, 8 steps of the wall pattern against 8 st_step
    calls on a twin batch: outputs and final state."""
    G = _engine()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, K = 64 * 4 * cus + 1, 8
    seeds = [SEED0 + e for e in range(n)]
    a = G.TetrisBatch(n, autoreset="same_step", seeds=seeds)
    b = G.TetrisBatch(n, autoreset="same_step", seeds=seeds)
    try:
        a.reset()
        b.reset()
        acts = torch.as_tensor(wall_pattern(10, K, n), device=a.device)
        ro, rr, rd = b.rollout(acts, obs="packed")
        for t in range(K):
            so, sr, sd = a.step(acts[t], obs="packed")
            assert torch.equal(so, ro[t]), ("obs", t)
            assert torch.equal(sr, rr[t]) and torch.equal(sd, rd[t]), t
        assert_same_state(a, b)
    finally:
        a.close()
        b.close()


ROLLOUT_CASES = [((10, 20), "c3", "packed"), ((10, 20), "c4", "packed"), ((10, 20), "c3", "f32"),
                 ((6, 9), "c3", "packed"), ((4, 4), "c3", "packed"), ((5, 27), "c3", "packed")]


@pytest.mark.gpu
@pytest.mark.parametrize("board,scoring,obs", ROLLOUT_CASES, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_three_wave_rollout_vs_oracle(board, scoring, obs):
    """k_rollout (st_rollout up to 4 workgroups per CU: every n here) on the
    wall pattern, the surface of the shared move / lock / scoring rules that
    the step tests above do not reach.  T steps as four launches, so the state
    is stored and reloaded and the piece queue restarts three times: obs,
    reward and done of every step, and the final state."""
    assert BOARDS[board] <= 64 * 4 * torch.cuda.get_device_properties(0).multi_processor_count  # the three-wave kernel
    b, ref = _batch(board, scoring)
    try:
        acts = torch.as_tensor(ref["acts"].copy(), device=b.device)
        K = T // 4
        for t0 in range(0, T, K):
            check_steps(ref, *b.rollout(acts[t0:t0 + K], obs=obs), t0=t0, H=board[1] if obs == "f32" else None)
        check_engine_state(b, ref["final"])
    finally:
        b.close()
