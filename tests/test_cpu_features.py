"""The parts of the ST_FEATS_BCTS feature set (st_feature_rows,
st_afterstates_set, st_policy_linear_set, st_play_linear_set) that need no
GPU: the reference rows pinned to hand-worked values, the ABI, and the host
layer's names, weights and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import feature_ref as FR
import placement_ref as PR
from harness import C4
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("st_afterstates_set", "st_policy_linear_set", "st_play_linear_set")

BOARD_A = """
....
X..X
..XX
X.XX
"""
BOARD_B = """
......
......
X.X..X
X.XX.X
X.X.XX
XX.XXX
"""


def _lib():
    from gym_simpletetris_amd import _lib as C
    return C, C.load()


# ------------------------------------------------------------------ the reference rows
def test_worked_boards():
    """The issue's two worked boards and the empty 10x20 board, literally."""
    a = FR.board_rows(BOARD_A)
    assert a.shape == (4, 4)
    assert FR.board_features(a) == (8, 6, 1, 1, 1) and len(FR.holes(a)) == 1
    b = FR.board_rows(BOARD_B)
    assert b.shape == (6, 6)
    assert FR.board_features(b) == (18, 10, 9, 4, 2) and len(FR.holes(b)) == 2
    assert FR.board_features(np.zeros((10, 20), bool)) == (40, 10, 0, 0, 0)


def test_landing_and_eroded_by_hand():
    """A flat I on the floor of an empty board: LANDING2 1, ERODED 0.  A
    vertical I that completes exactly one row: LINES 1, ERODED 1 -- through
    slot_features_bcts, the oracle playing the slots."""
    W, H = 10, 20
    h = PR.helper_oracle(dict(width=W, height=H, **C4))
    per = W + 6
    # the I's rotations: one of them lies flat (four cells in one row)
    flat = [r for r in range(4) if len({j for _, j in O.rotate_cells(O.BASE_SHAPES[5], r)}) == 1]
    upright = [r for r in range(4) if len({i for i, _ in O.rotate_cells(O.BASE_SHAPES[5], r)}) == 1]
    f = FR.slot_features_bcts(h, np.zeros((W, H), bool), 5, 0, 0)
    for r in flat:
        s = np.flatnonzero(f[PR.VALID, r * per:(r + 1) * per]) + r * per
        assert len(s) == W - 3
        assert (f[FR.LANDING2, s] == 1).all() and (f[FR.ERODED, s] == 0).all() and (f[PR.Y, s] == H - 1).all()
        # (the I against a wall closes one gap of its row: 40; elsewhere its row has four transitions)
        assert list(f[FR.ROW_TRANS, s]) == [40] + [42] * (W - 5) + [40] and (f[FR.COL_TRANS, s] == W).all()
    # the bottom row full but for column 4: an upright I there clears one row with one of its cells
    b = np.zeros((W, H), bool)
    b[:, H - 1] = True
    b[4, H - 1] = False
    f = FR.slot_features_bcts(h, b, 5, 0, 0)
    for r in upright:
        s = r * per + 4 + 3
        assert f[PR.VALID, s] == 1 and f[PR.LINES, s] == 1 and f[FR.ERODED, s] == 1
        assert f[FR.LANDING2, s] == 2 * H - 1 - ((H - 4) + (H - 1)) == 4
        # three cells are left in column 4 on the floor: a pillar of three
        assert f[FR.COL_TRANS, s] == W and f[FR.ROW_TRANS, s] == 2 * H + 2 * 3 - 0 and f[FR.WELLS, s] == 0
    # a row of f is zero exactly where the slot is invalid
    assert not f[:, f[PR.VALID] == 0].any()


# ------------------------------------------------------------------ the ABI
def test_feature_rows_values_and_errors():
    C, L = _lib()
    assert L.st_feature_rows(0) == 11 == C.AFTER_NFEAT and L.st_feature_rows(1) == 18 == len(C.AFTER_BCTS)
    for bad in (-1, 2, 1 << 20):
        assert L.st_feature_rows(bad) == C.ST_EINVAL
        assert b"st_feature_rows" in L.st_last_error()


def _call(L, call, ctx, fset, weights=None, n_w=1):
    buf = (ctypes.c_uint32 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    if call == "st_afterstates_set":
        return L.st_afterstates_set(ctx, fset, p, None, None)
    if call == "st_policy_linear_set":
        return L.st_policy_linear_set(ctx, fset, weights, n_w, None, p, None, None, None, None)
    return L.st_play_linear_set(ctx, fset, weights, n_w, 1, 1, p, None, None, None, None, None)


@pytest.mark.parametrize("call", NEW_CALLS)
def test_null_context_and_bad_set_are_einval_and_name_the_function(call):
    """A zeroed block stands in for a context: were it used, it would say
    "not seeded" (ST_ESTATE), which is what a good set then gives."""
    C, L = _lib()
    w = ctypes.cast((ctypes.c_float * 18)(), ctypes.c_void_p)
    assert _call(L, call, None, 1, w) == C.ST_EINVAL
    assert call.encode() in L.st_last_error()
    fake = (ctypes.c_uint64 * 512)()
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    for bad in (-1, 2, 77):
        assert _call(L, call, ctx, bad, w) == C.ST_EINVAL, bad
        assert call.encode() in L.st_last_error() and b"feature set" in L.st_last_error()
    for good in (0, 1):
        assert _call(L, call, ctx, good, w) == C.ST_ESTATE
        assert call.encode() in L.st_last_error()
    if call != "st_afterstates_set":
        assert _call(L, call, ctx, 1, None) == C.ST_EINVAL
        assert _call(L, call, ctx, 1, w, 0) == C.ST_EINVAL
        assert call.encode() in L.st_last_error()
    if call == "st_policy_linear_set":
        assert L.st_policy_linear_set(ctx, 1, w, 1, None, None, None, None, None, None) == C.ST_EINVAL
        assert b"st_policy_linear_set" in L.st_last_error()
    if call == "st_afterstates_set":
        assert L.st_afterstates_set(ctx, 1, None, None, None) == C.ST_EINVAL


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    C, L = _lib()
    assert L.st_abi_version() == C.ABI_VERSION == 4
    text = open(os.path.join(ROOT, "include", "simpletetris.h")).read()
    for name in NEW_CALLS + ("st_feature_rows",):
        assert name in C.SIG and hasattr(L, name)
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert C.FEATURE_SETS == dict(base=0, bcts=1)
    assert re.search(r"ST_FEATS_BASE\s*=\s*0\s*,\s*ST_FEATS_BCTS\s*=\s*1", text)


def _enum_names(text, enum, prefix):
    body = re.search(r"enum\s+%s\s*\{(.*?)\}" % enum, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [x.strip()[len(prefix):].lower() for x in body.split(",") if x.strip()][:-1]


def test_extension_names_follow_the_header_enum():
    from gym_simpletetris_amd import _lib as C
    text = open(os.path.join(ROOT, "include", "simpletetris.h")).read()
    ext = _enum_names(text, "st_after_ext", "ST_AFTER_EXT_")
    assert ext == list(C.AFTER_EXT) == list(FR.EXT_NAMES) and len(ext) == 7
    assert [C.AFTER_EXT[k] for k in ext] == list(range(11, 18))
    base = _enum_names(text, "st_after_feat", "ST_AFTER_")
    assert list(C.AFTER_BCTS) == base + ext and list(C.AFTER_BCTS.values()) == list(range(18))
    assert C.AFTER == {k: i for i, k in enumerate(base)} and C.AFTER_NFEAT == 11  # untouched


# ------------------------------------------------------------------ the host layer
def test_weight_rows_bcts_and_default_unchanged():
    from gym_simpletetris_amd import _lib as C
    from gym_simpletetris_amd.engine import weight_rows
    one11, one18 = list(range(11)), list(range(18))
    assert weight_rows(one11).shape == (1, 11) and weight_rows(one11, features="base").shape == (1, 11)
    for bad in (np.ones((2, 12)), one18, dict(wells=1.0)):  # the default set knows no extension row
        with pytest.raises(ValueError):
            weight_rows(bad)
    assert np.array_equal(weight_rows(one18, features="bcts"), np.arange(18, dtype=np.float32)[None])
    assert weight_rows(np.ones((5, 18)), features="bcts").shape == (5, 18)
    for name, row in C.AFTER_BCTS.items():
        v = weight_rows({name: 2.5}, features="bcts")
        assert v.shape == (1, 18) and v[0, row] == 2.5 and np.count_nonzero(v) == 1, name
    mixed = weight_rows([dict(wells=-1.0, lines=2.0), one18], features="bcts")
    assert mixed.shape == (2, 18) and mixed[0, 15] == -1.0 and mixed[0, 2] == 2.0 and mixed[1, 17] == 17.0
    for bad in (one11, np.ones((2, 11)), np.ones((2, 19)), dict(no_such_row=1.0), np.ones((0, 18))):
        with pytest.raises(ValueError):
            weight_rows(bad, features="bcts")
    for bad in ("dellacherie", None, 1):
        with pytest.raises(ValueError):
            weight_rows(one11, features=bad)


def test_published_weights_equal_the_table_and_are_read_only():
    import gym_simpletetris_amd as G
    assert dict(G.DELLACHERIE_WEIGHTS) == dict(landing2=-0.5, eroded=1, row_trans=-1, col_trans=-1, holes=-4, wells=-1)
    assert dict(G.BCTS_WEIGHTS) == dict(landing2=-6.315, eroded=6.60, row_trans=-9.22, col_trans=-19.77,
                                        holes=-13.08, wells=-10.49, hole_depth=-1.61, hole_rows=-24.04)
    for m in (G.DELLACHERIE_WEIGHTS, G.BCTS_WEIGHTS):
        with pytest.raises(TypeError):
            m["wells"] = 0.0
        assert G.engine.weight_rows(m, features="bcts").shape == (1, 18)
        with pytest.raises(ValueError):  # rows the base set does not have
            G.engine.weight_rows(m)
    assert dict(G.GREEDY_WEIGHTS) == dict(lines=80, holes=-12, height=-3, above=-2000)


def test_result_rows_by_name_with_18_rows():
    import torch
    from gym_simpletetris_amd import _lib as C
    from gym_simpletetris_amd.engine import Afterstates, LinearChoice
    feat = torch.arange(18 * 5, dtype=torch.int32).reshape(18, 5)
    c = LinearChoice(None, None, None, feat)
    for name, row in C.AFTER_BCTS.items():
        assert torch.equal(getattr(c, name), feat[row]), name
    small = LinearChoice(None, None, None, feat[:11])
    assert torch.equal(small.holes, feat[3])
    for obj in (small, LinearChoice(None, None, None, None), c):
        with pytest.raises(AttributeError):
            obj.wells if obj is not c else obj.no_such_row
    af = torch.arange(2 * 18 * 3, dtype=torch.int32).reshape(2, 18, 3)
    a = Afterstates(af, None)
    for name, row in C.AFTER_BCTS.items():
        assert torch.equal(getattr(a, name), af[:, row]), name
    a11 = Afterstates(af[:, :11], None)
    assert torch.equal(a11.bumpiness, af[:, 10])
    with pytest.raises(AttributeError):
        a11.landing2


def test_methods_reject_bad_arguments_before_any_device_call():
    """Unknown `features` and an `allowed` of the wrong shape, dtype or kind,
    on a stub whose device is the CPU: nothing reaches the library."""
    import torch
    from gym_simpletetris_amd.engine import TetrisBatch

    class Stub:
        n, width, n_slots, device = 4, 10, 64, torch.device("cpu")
        _weights = TetrisBatch._weights

    stub = Stub()
    for call in (lambda f: TetrisBatch.afterstates(stub, features=f),
                 lambda f: TetrisBatch.policy_linear(stub, [0.0] * 11, features=f),
                 lambda f: TetrisBatch.play_linear(stub, [0.0] * 11, 1, features=f)):
        for bad in ("dellacherie", "BCTS", None, 1):
            with pytest.raises(ValueError, match="features"):
                call(bad)
    w18 = [0.0] * 18
    with pytest.raises(ValueError):  # eleven weights for eighteen rows
        TetrisBatch.policy_linear(stub, [0.0] * 11, features="bcts")
    for bad in (torch.ones((4, 63), dtype=torch.int32), torch.ones((3, 64), dtype=torch.int32),
                torch.ones((4, 64), dtype=torch.int64), torch.ones((4, 64), dtype=torch.bool),
                torch.ones(4 * 64, dtype=torch.int32)):
        with pytest.raises((ValueError, TypeError)):
            TetrisBatch.policy_linear(stub, w18, features="bcts", allowed=bad)
    with pytest.raises((ValueError, TypeError)):
        TetrisBatch.policy_linear(stub, w18, features="bcts", allowed=np.ones((4, 64), np.int32))
