"""search.rollout_values / policy_rollout: the rollout algorithm on st_fork,
against the same loop whose branch states are built by the host route
(get_state -> set_state), bit for bit: values, the valid mask and the choice.
Two roots on 10x20, horizon 2, one or two samples (128 / 256 branch envs); root
1 is crafted so that some placements end the game at once, which shows the
alive masking: with reward_step every step behind the death would add 1 to the
death's -100."""
import numpy as np
import pytest
import torch

from harness import engine

pytestmark = pytest.mark.gpu

R, HORIZON = 2, 2
KW = dict(reward_step=True)
MT_ROW = 13


def _roots(G):
    """Two roots aged 12 BCTS placements; root 1 then gets columns 0..5 filled
    up to row 2: whatever lands on them reaches row 0 (tetris_env.py:277)."""
    root = G.TetrisBatch(R, seeds=[8800, 8801], autoreset="same_step", **KW)
    root.reset()
    root.play_linear(G.BCTS_WEIGHTS, 12, placements=True, features="bcts")
    board = root.get_state(("board",))["board"]
    board[:, 1] = 0
    board[:6, 1] = ((1 << 20) - 1) & ~0b11
    root.set_state(board=board)
    return root


def _branch(G, n, autoreset):
    b = G.TetrisBatch(n, seeds=[7000 + 3 * j for j in range(n)], autoreset=autoreset, **KW)
    b.reset()
    return b


@pytest.mark.parametrize("autoreset", ("same_step", "none"))
@pytest.mark.parametrize("samples,keep_rng", ((1, None), (2, None), (2, False)))
def test_rollout_equals_the_host_route(samples, keep_rng, autoreset):
    G = engine()
    from gym_simpletetris_amd import search as SR
    root = _roots(G)
    S = root.n_slots
    n = R * S * samples
    A, B, C = (_branch(G, n, autoreset) for _ in range(3))
    W = torch.as_tensor(G.engine.weight_rows(G.BCTS_WEIGHTS, "bcts"), device=root.device)
    try:
        values, valid = SR.rollout_values(root, A, W, HORIZON, samples, "bcts", keep_rng)
        assert values.dtype == torch.float32 and tuple(values.shape) == (R, S)
        assert valid.dtype == torch.bool and tuple(valid.shape) == (R, S)
        choice = SR.choose(values, valid)
        assert torch.equal(SR.policy_rollout(root, C, W, HORIZON, samples, "bcts", keep_rng), choice)

        # the parent's route: the roots' states through host memory into B
        keep = samples > 1 if keep_rng is None else keep_rng
        j_root = SR.branch_layout(R, S, samples)[0]
        rs, bs = root.get_state(), B.get_state(("stats", "mt"))
        stats, mt = rs["stats"][:, j_root].copy(), rs["mt"][j_root]
        if keep:  # the branch column's own synced MT index and words
            stats[MT_ROW], mt = bs["stats"][MT_ROW], bs["mt"]
        B.set_state(board=rs["board"][:, j_root], stats=stats, piece=rs["piece"][j_root], mt=mt)
        v2, ok2 = SR.rollout_branches(B, R, W, HORIZON, samples, "bcts")
        print("rollout", samples, keep, autoreset, "values of root 1", values[1][valid[1]].tolist())
        assert torch.equal(valid, ok2)
        assert torch.equal(values, v2)
        assert torch.equal(choice, SR.choose(v2, ok2))

        # root 1: the placements that die are worth the death's -100 and nothing behind it
        af = root.afterstates(boards=False)
        assert torch.equal(valid, af.valid != 0)
        assert (values[~valid] == float("-inf")).all() and torch.isfinite(values[valid]).all()
        dead = valid[1] & (af.dead[1] != 0)
        live = valid[1] & ~dead
        assert dead.any() and live.any()
        assert (values[1][dead] == -100.0).all()
        assert (values[1][live] > -100.0).all()
        assert (choice >= 0).all() and bool(live[int(choice[1])])
        assert not (valid[0] & (af.dead[0] != 0)).any() and (values[0][valid[0]] >= 1.0).all()
    finally:
        for b in (root, A, B, C):
            b.close()


def test_sizes_are_checked():
    G = engine()
    from gym_simpletetris_amd import search as SR
    root = _roots(G)
    small = _branch(G, R * root.n_slots - 1, "same_step")
    other = G.TetrisBatch(R * 4 * (6 + 6), width=6, height=9, seeds=list(range(R * 48)))
    try:
        for bad in (dict(branch=small), dict(branch=other), dict(branch=small, samples=0)):
            with pytest.raises(ValueError):
                SR.rollout_values(root, bad.pop("branch"), G.BCTS_WEIGHTS, 1, features="bcts", **bad)
        with pytest.raises(ValueError):
            SR.rollout_branches(small, R, G.BCTS_WEIGHTS, -1, features="bcts")
    finally:
        for b in (root, small, other):
            b.close()
