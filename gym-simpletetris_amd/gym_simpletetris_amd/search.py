"""The rollout algorithm (Bertsekas & Ioffe's rollout on Tetris) over
TetrisBatch's public calls: every placement of every root's piece is tried in a
branch env of its own and played on by a base policy, and the placement whose
branches collect the most reward wins.

The helpers are Python loops; the hot paths are TetrisBatch.fork (st_fork),
which puts the roots' states into the branch batch on the device, and the
kernels behind step_placements and policy_linear.  Nothing here reads a result
back to the host.

Branch layout: with R roots, S = root.n_slots placements and M samples, branch
env j = (r * S + s) * M + m tries slot s of root r, sample m.
"""
from __future__ import annotations

import numpy as np
import torch

from .engine import TetrisBatch


def branch_layout(roots: int, slots: int, samples: int = 1):
    """(root[j], slot[j], sample[j]), int32 numpy arrays over the branch envs
    j = (r * slots + s) * samples + m.  Pure host code."""
    if min(roots, slots, samples) < 1:
        raise ValueError(f"roots, slots and samples must be >= 1, got {(roots, slots, samples)}")
    j = np.arange(roots * slots * samples, dtype=np.int64)
    return ((j // (slots * samples)).astype(np.int32), (j // samples % slots).astype(np.int32),
            (j % samples).astype(np.int32))


_LAYOUTS: dict = {}


def _layout_on(device, roots: int, slots: int, samples: int):
    """branch_layout's root[j] and slot[j] as int32 tensors on `device`, made once per shape."""
    key = (str(device), roots, slots, samples)
    if key not in _LAYOUTS:
        root, slot, _ = branch_layout(roots, slots, samples)
        _LAYOUTS[key] = (torch.as_tensor(root, device=device), torch.as_tensor(slot, device=device))
    return _LAYOUTS[key]


def _sizes(root: TetrisBatch, branch: TetrisBatch, samples: int):
    if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or samples < 1:
        raise ValueError(f"samples must be an integer >= 1, got {samples!r}")
    R, S, M = root.n, root.n_slots, int(samples)
    if branch.n != R * S * M:
        raise ValueError(f"branch must have root.n * n_slots * samples = {R} * {S} * {M} = {R * S * M} envs, "
                         f"got {branch.n}")
    if (branch.width, branch.height) != (root.width, root.height):
        raise ValueError("root and branch must have the same board size")
    return R, S, M


def rollout_branches(branch: TetrisBatch, roots: int, weights, horizon: int, samples: int = 1,
                     features: str = "base"):
    """The rollout from branch envs that already hold their roots' states
    (rollout_values without its fork): branch env j places slot[j], then
    plays `horizon` placements of policy_linear(weights, features).  Returns
    (values float32 [R, S], valid bool [R, S]) as rollout_values does."""
    if isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)) or horizon < 0:
        raise ValueError(f"horizon must be an integer >= 0, got {horizon!r}")
    R, S, M = int(roots), branch.n_slots, int(samples)
    if branch.n != R * S * M:
        raise ValueError(f"branch must have {R} * {S} * {M} envs, got {branch.n}")
    slot = _layout_on(branch.device, R, S, M)[1]
    _, reward, done = branch.step_placements(slot, obs="none")
    valid = branch.placed.view(R, S, M)[:, :, 0] != 0
    # V(j) = sum of reward_t * alive_t: alive falls to 0 behind the first done,
    # so the sum is the same under both autoreset modes
    total = reward.to(torch.int64)
    alive = ~done.to(torch.bool)
    for _ in range(int(horizon)):
        choice = branch.policy_linear(weights, features=features)
        _, reward, done = branch.step_placements(choice.slots, obs="none")
        total += reward * alive
        alive &= ~done.to(torch.bool)
    values = (total.view(R, S, M).sum(-1).to(torch.float64) / M).to(torch.float32)
    return torch.where(valid, values, torch.full_like(values, float("-inf"))), valid


def rollout_values(root: TetrisBatch, branch: TetrisBatch, weights, horizon: int, samples: int = 1,
                   features: str = "base", keep_rng=None):
    """The value of every placement of every root's current piece under the
    rollout algorithm.  `branch` (root.n * root.n_slots * samples envs, same
    board) is overwritten: branch.fork(root, index=root[j]) puts root r's state
    into its S * samples branch envs, branch env j places slot[j]
    (step_placements), and `horizon` further placements follow the base policy
    policy_linear(weights, features).  V(j) is the reward collected until the
    branch's first done, the death's own reward included; values[r, s]
    (float32 [R, S]) is its mean over the samples, -inf where slot s is not a
    valid placement for root r; valid (bool [R, S]) says which are.
    keep_rng (default: samples > 1): the branch envs keep their own MT19937
    streams, so the samples of one placement see different piece futures (seed
    the branch batch's envs differently); False gives every branch the root's
    own future.  `root` is only read.  Everything stays on the device."""
    R, S, M = _sizes(root, branch, samples)
    index = _layout_on(branch.device, R, S, M)[0]
    branch.fork(root, index=index, keep_rng=(M > 1) if keep_rng is None else bool(keep_rng))
    return rollout_branches(branch, R, weights, horizon, M, features)


def choose(values: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    """The valid slot with the largest value per root (int32 [R]), ties to the
    lowest slot; -1 where none is valid."""
    S = values.shape[1]
    best = torch.where(valid, values, torch.full_like(values, float("-inf"))).max(dim=1, keepdim=True).values
    cand = valid & (values == best)
    slots = torch.arange(S, device=values.device, dtype=torch.int32).expand_as(cand)
    first = torch.where(cand, slots, torch.full_like(slots, S)).min(dim=1).values
    return torch.where(first < S, first, torch.full_like(first, -1))


def policy_rollout(root: TetrisBatch, branch: TetrisBatch, weights, horizon: int, samples: int = 1,
                   features: str = "base", keep_rng=None) -> torch.Tensor:
    """The rollout player's choice for every root: choose(*rollout_values(...)),
    int32 [R] -- what root.step_placements() takes."""
    return choose(*rollout_values(root, branch, weights, horizon, samples, features, keep_rng))
