"""The reachability sample's conditions, on the oracle alone (no GPU): the
sample that test_gpu_reachable.py checks st_reachable / st_route_actions on
must hold what makes the check worth something -- unreachable slots, long
routes, slots the greedy rule misses, live lock counters, every first action --
and reach_ref must give the hand-computed answers of three crafted states."""
import numpy as np
import pytest

import reach_ref as R


@pytest.mark.parametrize("board,config", R.CASES)
def test_sample_has_unreachable_long_and_missed_slots(board, config):
    smp = R.sample(board, config)
    valid, steps = smp["valid"], smp["steps"]
    reach = steps > 0
    assert not (reach & ~valid).any()
    n_valid, n_reach = int(valid.sum()), int(reach.sum())
    print(board, config, "valid", n_valid, "reachable", n_reach, "steps >= 4", int((steps >= 4).sum()),
          "longest", int(steps.max()), "layers", int(smp["layers"].max()))
    assert n_valid - n_reach >= 0.10 * n_valid
    assert n_reach >= 0.50 * n_valid
    assert int((steps >= 4).sum()) >= 100
    assert (steps[reach] >= 1).all() and (smp["first"][~reach] == 2).all()
    # st_placement_actions's rule, played out on the oracle, misses reachable slots
    kw = R.case_kw(board, config)
    h, hf = R.helpers(kw)
    ob, missed = smp["ob"], 0
    for e in range(R.N):
        env = ob.envs[e]
        h.load(ob.board(e), env.shape_id)
        hf.load(ob.board(e), env.shape_id)
        for s in np.flatnonzero(reach[e]):
            missed += not R.greedy_lands(h, hf, env.rot, env.ax, env.ay, env.lock, kw["width"], int(s), smp["Y"][e, s])
    print("missed by the greedy rule", missed)
    assert missed >= 50
    if kw.get("lock_delay", 0) > 0:
        assert int((smp["lock"] > 0).sum()) >= 10


def test_every_first_action_but_idle_occurs():
    seen = np.zeros(7, np.int64)
    for board, config in R.CASES:
        smp = R.sample(board, config)
        seen += np.bincount(smp["first"][smp["steps"] > 0], minlength=7)
    print("first actions", seen)
    assert (seen[:6] > 0).all()
    assert seen[6] == 0  # idle never beats a lower-numbered action with the same effect (soft drop)


@pytest.mark.parametrize("case", R.HAND, ids=[c[0] for c in R.HAND])
def test_crafted_states_by_hand(case):
    want = case[8]
    steps, first, valid, _ = R.crafted_answer(case)
    S = 4 * (R.CW + 6)
    exp_steps, exp_first = np.zeros(S, np.int32), np.full(S, 2, np.uint8)
    for s, (k, a) in want.items():
        exp_steps[s], exp_first[s] = k, a
    assert valid[list(want)].all()
    assert np.array_equal(steps, exp_steps), np.flatnonzero(steps != exp_steps)
    assert np.array_equal(first, exp_first), np.flatnonzero(first != exp_first)


def test_under_overhang_slot_is_valid_but_unreachable():
    case = R.HAND[2]
    steps, _, valid, Y = R.crafted_answer(case)
    s = R._sl(0, 0)
    assert valid[s] and Y[s] == 3 and steps[s] == 0
