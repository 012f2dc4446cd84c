"""The parts of st_policy_linear / st_play_linear that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from gym_simpletetris_amd import _lib as C
    return C, C.load()


def _call(L, call, ctx, weights, n_w):
    """The call with one output buffer (so that only ctx / weights / n_w can be at fault)."""
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    if call == "st_policy_linear":
        return L.st_policy_linear(ctx, weights, n_w, p, None, None, None, None)
    return L.st_play_linear(ctx, weights, n_w, 1, p, None, None, None, None, None)


@pytest.mark.parametrize("call", ["st_policy_linear", "st_play_linear"])
def test_null_context_is_einval_and_names_the_function(call):
    C, L = _lib()
    w = (ctypes.c_float * C.AFTER_NFEAT)()
    assert _call(L, call, None, ctypes.cast(w, ctypes.c_void_p), 1) == C.ST_EINVAL
    assert call.encode() in L.st_last_error()


@pytest.mark.parametrize("call", ["st_policy_linear", "st_play_linear"])
def test_null_weights_and_bad_row_count_are_einval(call):
    """Argument errors come before the context is used and before any GPU
    call: a zeroed block stands in for a context (were it read, it would say
    "not seeded", ST_ESTATE)."""
    C, L = _lib()
    fake = (ctypes.c_uint64 * 512)()
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    w = ctypes.cast((ctypes.c_float * C.AFTER_NFEAT)(), ctypes.c_void_p)
    assert _call(L, call, ctx, None, 1) == C.ST_EINVAL
    assert call.encode() in L.st_last_error()
    for n_w in (0, -1, -(1 << 40)):
        assert _call(L, call, ctx, w, n_w) == C.ST_EINVAL, n_w
        assert call.encode() in L.st_last_error()


def test_all_outputs_null_is_einval():
    C, L = _lib()
    fake = (ctypes.c_uint64 * 512)()
    w = ctypes.cast((ctypes.c_float * C.AFTER_NFEAT)(), ctypes.c_void_p)
    assert L.st_policy_linear(ctypes.cast(fake, ctypes.c_void_p), w, 1, None, None, None, None, None) == C.ST_EINVAL
    assert b"st_policy_linear" in L.st_last_error()


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    C, L = _lib()
    assert L.st_abi_version() == C.ABI_VERSION == 4
    assert "st_policy_linear" in C.SIG and "st_play_linear" in C.SIG
    text = open(os.path.join(ROOT, "include", "simpletetris.h")).read()
    for name in ("st_policy_linear", "st_play_linear"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_weights_by_name_follow_the_header_enum():
    """GREEDY_WEIGHTS and the dict-to-vector helper place values by the
    header's st_after_feat order; missing names are 0."""
    from gym_simpletetris_amd import GREEDY_WEIGHTS
    from gym_simpletetris_amd.engine import weight_rows
    text = open(os.path.join(ROOT, "include", "simpletetris.h")).read()
    body = re.search(r"enum\s+st_after_feat\s*\{(.*?)\}", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [x.strip()[len("ST_AFTER_"):].lower() for x in body.split(",") if x.strip()][:-1]
    assert len(names) == 11
    assert dict(GREEDY_WEIGHTS) == dict(lines=80, holes=-12, height=-3, above=-2000)
    g = weight_rows(GREEDY_WEIGHTS)
    assert g.dtype == np.float32 and g.shape == (1, 11)
    want = np.zeros(11, np.float32)
    want[names.index("lines")], want[names.index("holes")] = 80, -12
    want[names.index("height")], want[names.index("above")] = -3, -2000
    assert np.array_equal(g[0], want)
    for i, name in enumerate(names):  # every name lands in its own row
        v = weight_rows({name: 2.5})
        assert v[0, i] == 2.5 and np.count_nonzero(v) == 1, name
    with pytest.raises(TypeError):  # a constant
        GREEDY_WEIGHTS["lines"] = 1.0


def test_weight_rows_shapes_and_errors():
    from gym_simpletetris_amd.engine import weight_rows
    one = list(range(11))
    assert np.array_equal(weight_rows(one), np.arange(11, dtype=np.float32)[None])
    assert weight_rows([one, one, one]).shape == (3, 11)
    assert weight_rows(np.ones((5, 11), np.float64)).dtype == np.float32
    mixed = weight_rows([dict(valid=1.0), one])
    assert mixed.shape == (2, 11) and mixed[0, 0] == 1.0 and mixed[1, 10] == 10.0
    for bad in (list(range(10)), np.ones((2, 12)), np.ones((2, 3, 11)), np.ones((0, 11)), dict(no_such_row=1.0),
                [dict(lines=1.0), list(range(10))]):
        with pytest.raises(ValueError):
            weight_rows(bad)
    for bad in (3.0, "lines", None, np.array(["a"] * 11)):
        with pytest.raises(TypeError):
            weight_rows(bad)


def test_result_rows_by_name():
    import torch
    from gym_simpletetris_amd import _lib as C
    from gym_simpletetris_amd.engine import LinearChoice
    feat = torch.arange(C.AFTER_NFEAT * 5, dtype=torch.int32).reshape(C.AFTER_NFEAT, 5)
    sl, ac, sc = torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8), torch.zeros(5)
    c = LinearChoice(sl, ac, sc, feat)
    assert c.slots is sl and c.actions is ac and c.scores is sc and c.feat is feat
    for name, row in C.AFTER.items():
        assert torch.equal(getattr(c, name), feat[row]), name
    with pytest.raises(AttributeError):
        c.no_such_row
    with pytest.raises(AttributeError):  # the feature rows were not asked for
        LinearChoice(sl, None, None, None).lines


def test_methods_reject_bad_arguments_before_any_device_call():
    """play_linear's k / obs checks and policy_linear's `out` arity run ahead
    of everything that needs a device."""
    from gym_simpletetris_amd.engine import TetrisBatch

    class Stub:
        n = 4
    for k in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError):
            TetrisBatch.play_linear(Stub, [0.0] * 11, k)
    with pytest.raises(ValueError):
        TetrisBatch.play_linear(Stub, [0.0] * 11, 1, obs="f32")
