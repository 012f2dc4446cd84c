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
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_parity import _engine

T = 200
SEED0 = 4242
# n: whole workgroups on the 16-byte store path and a last, partial one on
# the per-env path; 10x20 the fixed-size kernel, 6x9 / 4x4 the generic one,
# 5x27 the generic one with H > 25 (64-bit cell shifts)
BOARDS = {(10, 20): 1000, (6, 9): 300, (4, 4): 300, (5, 27): 300}
C4 = dict(advanced_clears=True, penalise_holes_increase=True, penalise_height_increase=True)


def wall_pattern(W, steps, n):
    """actions [steps, n]: env i repeats W // 2 + 1 moves towards one wall
    (enough to reach it from the spawn column), 0..3 rotations and a hard
    drop; i selects the wall, the rotation count, which run comes first, the
    rotation's sense and the phase."""
    i = np.arange(n)
    k = i % 16
    side = (k & 1).astype(np.uint8)  # 0: left, 1: right
    nrot = (k >> 1) & 3
    rot_first = ((k >> 3) & 1).astype(bool)
    rot_act = np.where((i >> 4) & 1, 5, 4).astype(np.uint8)
    moves = W // 2 + 1
    period = moves + nrot + 1
    phase = (i >> 5) % period
    acts = np.empty((steps, n), np.uint8)
    for t in range(steps):
        u = (t + phase) % period
        first = np.where(rot_first, nrot, moves)
        in_first = u < first
        in_second = ~in_first & (u < moves + nrot)
        rot_now = np.where(rot_first, in_first, in_second)
        mov_now = np.where(rot_first, in_second, in_first)
        acts[t] = np.where(rot_now, rot_act, np.where(mov_now, side, 2))
    return acts


def _field(ob, name, shape=()):
    """View of one int32 field of every oracle env (no copy)."""
    raw = np.frombuffer(ob.envs, dtype=np.uint8).reshape(ob.n, ctypes.sizeof(O.Env))
    off = getattr(O.Env, name).offset
    cnt = int(np.prod(shape)) if shape else 1
    v = raw[:, off:off + 4 * cnt].view(np.int32)
    return v.reshape((ob.n,) + tuple(shape)) if shape else v[:, 0]


def oracle_run(W, H, n, kw):
    """The oracle's outputs for the wall pattern, its state after the last
    step, and the coverage of the locks by hard drop (the piece locks where
    it stood before the step, so the oracle's piece state before the step is
    the locked pose): (shape, rotation) -> locks with a cell in column 0 /
    in column W - 1, and locks of a one-column rotation in column W - 1."""
    seeds = [SEED0 + e for e in range(n)]
    ob = O.OracleBatch(n, seeds, width=W, height=H, **kw)
    ob.reset()
    acts = wall_pattern(W, T, n)
    out = dict(acts=acts, obs=np.empty((T, n, W), np.uint32), reward=np.empty((T, n), np.int32),
               done=np.empty((T, n), np.uint8), stats=np.empty((T, n, 8), np.int32))
    left = np.zeros((7, 4), np.int64)
    right = np.zeros((7, 4), np.int64)
    thin_right = 0
    for t in range(T):
        sid, rot, ax = _field(ob, "shape_id").copy(), _field(ob, "rot").copy(), _field(ob, "ax").copy()
        cols = ax[:, None] + _field(ob, "shape", (4, 2))[:, :, 0]
        before = _field(ob, "counts", (7,)).sum(axis=1)
        r = ob.rollout(acts[t:t + 1])
        for k in ("obs", "reward", "done", "stats"):
            out[k][t] = r[k][0]
        locked = ((_field(ob, "counts", (7,)).sum(axis=1) != before) | (r["done"][0] != 0)) & (acts[t] == 2)
        at_l = locked & (cols.min(axis=1) == 0)
        at_r = locked & (cols.max(axis=1) == W - 1)
        np.add.at(left, (sid[at_l], rot[at_l] & 3), 1)
        np.add.at(right, (sid[at_r], rot[at_r] & 3), 1)
        thin_right += int((at_r & (cols.min(axis=1) == cols.max(axis=1))).sum())
    board = np.zeros((W, n), np.uint32)
    for i in range(n):
        board[:, i] = (ob.board(i).astype(np.uint32) << np.arange(H, dtype=np.uint32)).sum(axis=1)
    piece = (_field(ob, "shape_id") | (_field(ob, "rot") & 3) << 3 | _field(ob, "ax") << 5 |
             _field(ob, "ay") << 11 | _field(ob, "lock") << 17).astype(np.uint32)
    stats = np.stack([_field(ob, k) for k in ("time", "score", "lines_cleared", "holes", "piece_height",
                                              "n_deaths")] + list(_field(ob, "counts", (7,)).T))
    out.update(left=left, right=right, thin_right=thin_right, board=board, piece=piece, stats_end=stats)
    return out


_REF = {}


def _ref(W, H, kw_name="c3"):
    """One oracle run per board and scoring, shared by the tests (read-only)."""
    key = (W, H, kw_name)
    if key not in _REF:
        _REF[key] = oracle_run(W, H, BOARDS[(W, H)], C4 if kw_name == "c4" else {})
        for v in _REF[key].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REF[key]


def _check_final_state(b, ref):
    """Board, piece word and counter rows after the last step (a board row
    the store phase wrongly took for clean would show here)."""
    st = b.get_state(("board", "piece", "stats"))
    assert np.array_equal(st["board"], ref["board"]), "board"
    assert np.array_equal(st["piece"], ref["piece"]), "piece"
    assert np.array_equal(st["stats"][:13], ref["stats_end"]), "counters"


def _unpack_f32(words, H):
    return ((words[:, :, None] >> np.arange(H, dtype=np.uint32)) & 1).astype(np.float32)


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
    step, the vector env's terminal obs and counters, and the final state."""
    G = _engine()
    from gym_simpletetris_amd.engine import unwire
    W, H = board
    n = BOARDS[board]
    ref = _ref(W, H)
    if board == (10, 20):
        _assert_coverage(ref)
    if surface == "vec":
        env = G.TetrisVecEnv(n, width=W, height=H, seed=SEED0, obs_format="packed")
        env.reset()
        b = env.engine
    else:
        env = None
        b = G.TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[SEED0 + e for e in range(n)])
        b.reset()
    try:
        acts = torch.as_tensor(ref["acts"].copy(), device=b.device)
        for t in range(T):
            done = ref["done"][t].astype(bool)
            robs = ref["obs"][t]
            if surface == "vec":
                obs, rew, dn, info = env.step(acts[t])
                fin = info["final_observation"].cpu().numpy().view(np.uint32).T
                assert np.array_equal(fin, np.where(done[:, None], robs, 0)), ("final_observation", t)
                st = ref["stats"][t]  # time, score, lines, holes, deaths, piece id, height, lock
                zero = np.zeros(n, np.int32)
                for k, col, ep in (("time", 0, "ep_time"), ("score", 1, "ep_score"),
                                   ("lines_cleared", 2, "ep_lines"), ("holes", 3, "ep_holes")):
                    assert np.array_equal(info[k].cpu().numpy(), np.where(done, zero, st[:, col])), (k, t)
                    assert np.array_equal(info[ep].cpu().numpy(), np.where(done, st[:, col], zero)), (ep, t)
                assert np.array_equal(info["deaths"].cpu().numpy(), st[:, 4]), ("deaths", t)
                assert np.array_equal(info["piece_height"].cpu().numpy(), np.where(done, zero, st[:, 6])), t
                robs = np.where(done[:, None], 0, robs)  # the reset convention
            elif surface == "wire":
                obs, rew, dn = unwire(b.step_wire(acts[t]), W, H)
            elif surface == "f32":
                f32, rew, dn = b.step(acts[t], obs="f32")
                assert np.array_equal(f32.cpu().numpy(), _unpack_f32(robs, H)), ("f32 obs", t)
                obs = b.obs
            else:
                obs, rew, dn = b.step(acts[t], obs="packed")
            assert np.array_equal(rew.cpu().numpy(), ref["reward"][t]), ("reward", t)
            assert np.array_equal(dn.cpu().numpy().astype(bool), done), ("done", t)
            assert np.array_equal(obs.cpu().numpy().view(np.uint32).T, robs), ("obs", t)
        _check_final_state(b, ref)
    finally:
        (env or b).close()


@pytest.mark.gpu
def test_step_scoring_flags_vs_oracle():
    """The same stream with C4's scoring flags (the non-SC0 instantiation of
    the fixed-size kernel: late counters feed the height / holes rewards)."""
    G = _engine()
    W, H = 10, 20
    n = BOARDS[(W, H)]
    ref = _ref(W, H, "c4")
    b = G.TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[SEED0 + e for e in range(n)], **C4)
    b.reset()
    try:
        acts = torch.as_tensor(ref["acts"].copy(), device=b.device)
        for t in range(T):
            obs, rew, dn = b.step(acts[t], obs="packed")
            assert np.array_equal(rew.cpu().numpy(), ref["reward"][t]), ("reward", t)
            assert np.array_equal(dn.cpu().numpy().astype(np.uint8), ref["done"][t]), ("done", t)
            assert np.array_equal(obs.cpu().numpy().view(np.uint32).T, ref["obs"][t]), ("obs", t)
        _check_final_state(b, ref)
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
        sa, sb = a.get_state(), b.get_state()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
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
    G = _engine()
    W, H = board
    n = BOARDS[board]
    assert n <= 64 * 4 * torch.cuda.get_device_properties(0).multi_processor_count  # the three-wave kernel
    ref = _ref(W, H, scoring)
    b = G.TetrisBatch(n, width=W, height=H, autoreset="same_step", seeds=[SEED0 + e for e in range(n)],
                      **(C4 if scoring == "c4" else {}))
    b.reset()
    try:
        acts = torch.as_tensor(ref["acts"].copy(), device=b.device)
        K = T // 4
        for t0 in range(0, T, K):
            o, rew, dn = b.rollout(acts[t0:t0 + K], obs=obs)
            o, rew, dn = o.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy()
            for k in range(K):
                t = t0 + k
                assert np.array_equal(rew[k], ref["reward"][t]), ("reward", t)
                assert np.array_equal(dn[k].astype(np.uint8), ref["done"][t]), ("done", t)
                if obs == "f32":
                    assert np.array_equal(o[k], _unpack_f32(ref["obs"][t], H)), ("f32 obs", t)
                else:
                    assert np.array_equal(o[k].view(np.uint32).T, ref["obs"][t]), ("obs", t)
        _check_final_state(b, ref)
    finally:
        b.close()
