"""The parts of st_afterstates / st_placement_actions that need no GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from gym_simpletetris_amd import _lib as C
    return C, C.load()


@pytest.mark.parametrize("call", ["st_afterstates", "st_placement_actions"])
def test_null_context_is_einval_and_names_the_function(call):
    C, L = _lib()
    buf = (ctypes.c_uint32 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert getattr(L, call)(None, p, p, None) == C.ST_EINVAL
    assert call.encode() in L.st_last_error()


def test_after_slots_values_and_range():
    C, L = _lib()
    assert [L.st_after_slots(w) for w in (4, 10, 13, 32)] == [40, 64, 76, 152]
    for w in range(4, 33):
        assert L.st_after_slots(w) == 4 * (w + 6)
    for w in (-1, 0, 3, 33, 1 << 20):
        assert L.st_after_slots(w) == C.ST_EINVAL, w
        assert b"st_after_slots" in L.st_last_error()


def test_feature_rows_agree_with_the_header_enum():
    """AFTER / AFTER_NFEAT are the header's st_after_feat, in its order."""
    from gym_simpletetris_amd import _lib as C
    text = open(os.path.join(ROOT, "include", "simpletetris.h")).read()
    body = re.search(r"enum\s+st_after_feat\s*\{(.*?)\}", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [x.strip() for x in body.split(",") if x.strip()]
    assert all(re.fullmatch(r"ST_AFTER_[A-Z_]+", x) for x in names), names  # no explicit values: 0, 1, 2, ...
    assert names[-1] == "ST_AFTER_NFEAT" and C.AFTER_NFEAT == len(names) - 1 == 11
    want = {x[len("ST_AFTER_"):].lower(): i for i, x in enumerate(names[:-1])}
    assert C.AFTER == want
    assert list(C.AFTER) == [x[len("ST_AFTER_"):].lower() for x in names[:-1]]


@pytest.mark.parametrize("W", [4, 10, 13, 32])
def test_slot_round_trip(W):
    from gym_simpletetris_amd.engine import placement_rot_x, placement_slot
    _, L = _lib()
    S = L.st_after_slots(W)
    seen = []
    for rot in range(4):          # the (rot, x) loop order is the slot order
        for x in range(-3, W + 3):
            s = placement_slot(W, rot, x)
            assert placement_rot_x(W, s) == (rot, x)
            seen.append(s)
    assert seen == list(range(S))
    for rot, x in ((-1, 0), (4, 0), (0, -4), (0, W + 3)):
        with pytest.raises(ValueError):
            placement_slot(W, rot, x)
    for s in (-1, S):
        with pytest.raises(ValueError):
            placement_rot_x(W, s)


def test_batch_methods_use_the_same_slot_rule():
    """TetrisBatch.slot / slot_rot_x / n_slots without a device: the methods
    read only the width."""
    from gym_simpletetris_amd.engine import TetrisBatch, placement_slot

    class Stub:
        width = 13
    assert TetrisBatch.n_slots.fget(Stub) == 76
    assert TetrisBatch.slot(Stub, 2, -3) == placement_slot(13, 2, -3) == 38
    assert TetrisBatch.slot_rot_x(Stub, 75) == (3, 15)


def test_result_rows_by_name():
    import torch
    from gym_simpletetris_amd import _lib as C
    from gym_simpletetris_amd.engine import Afterstates
    feat = torch.arange(2 * C.AFTER_NFEAT * 5, dtype=torch.int32).reshape(2, C.AFTER_NFEAT, 5)
    a = Afterstates(feat, None)
    for name, row in C.AFTER.items():
        assert torch.equal(getattr(a, name), feat[:, row]), name
    assert a.boards is None
    with pytest.raises(AttributeError):
        a.no_such_row
