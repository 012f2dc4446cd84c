"""The parts of st_fork / TetrisBatch.fork / search that need no GPU: the
ABI, the host layer's argument checks, branch_layout, and the oracle-side
reference (fork_ref) held to the oracle's own stepping."""
import ctypes
import os
import re

import numpy as np
import pytest

import fork_ref as FK
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from gym_simpletetris_amd import _lib as C
    return C, C.load()


# ------------------------------------------------------------------ the ABI
def test_the_flag_and_the_symbol_match_the_header():
    C, L = _lib()
    text = open(os.path.join(ROOT, "include", "simpletetris.h")).read()
    m = re.search(r"ST_FORK_KEEP_RNG\s*=\s*1u\s*<<\s*(\d+)", text)
    assert m and 1 << int(m.group(1)) == C.FORK_KEEP_RNG
    assert re.search(r"\bint\s+st_fork\s*\(", text)
    assert "st_fork" in C.SIG and hasattr(L, "st_fork") and L.st_fork.argtypes == C.SIG["st_fork"][0]
    assert L.st_abi_version() == C.ABI_VERSION == 4
    assert "st_fork" in text[:text.index("#define ST_ABI_VERSION")]  # the version comment lists it


def test_argument_errors_come_before_any_gpu_call():
    """Zeroed blocks stand in for contexts: were they used, they would say "not
    seeded" (ST_ESTATE), which is what good arguments then give."""
    C, L = _lib()
    assert L.st_fork(None, None, None, None, 0, None) == C.ST_EINVAL
    assert b"st_fork" in L.st_last_error()
    a = ctypes.cast((ctypes.c_uint64 * 512)(), ctypes.c_void_p)
    b = ctypes.cast((ctypes.c_uint64 * 512)(), ctypes.c_void_p)
    assert L.st_fork(a, None, None, None, 0, None) == C.ST_EINVAL
    assert L.st_fork(None, b, None, None, 0, None) == C.ST_EINVAL
    for flags in (2, 3, 1 << 31):
        assert L.st_fork(a, b, None, None, flags, None) == C.ST_EINVAL
        assert b"flag" in L.st_last_error()
    for flags in (0, C.FORK_KEEP_RNG):
        assert L.st_fork(a, b, None, None, flags, None) == C.ST_ESTATE
        assert L.st_fork(a, a, None, None, flags, None) == C.ST_ESTATE
        assert b"st_fork" in L.st_last_error()
    # the config is the struct's first member: another width is refused before the state is looked at
    wide = (ctypes.c_uint64 * 512)()
    ctypes.cast(wide, ctypes.POINTER(C.Config))[0] = C.Config(12, 0, 0, 0, 0)
    assert L.st_fork(a, ctypes.cast(wide, ctypes.c_void_p), None, None, 0, None) == C.ST_EINVAL


# ------------------------------------------------------------------ the host layer
def test_fork_rejects_bad_arguments_before_any_device_call():
    import torch
    from gym_simpletetris_amd.engine import TetrisBatch

    class Stub:
        n, width, height, device = 4, 10, 20, torch.device("cpu")
        _intake = TetrisBatch._intake
        _need = TetrisBatch._need
        _fork_index = TetrisBatch._fork_index
        _fork_groups = {}

    stub = Stub()
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.float32), torch.zeros(5, dtype=torch.int32),
                torch.zeros((2, 4), dtype=torch.int32)[0:2, 0], torch.zeros(4, dtype=torch.int32, device="meta"),
                [0, 1, 2], [0.5, 1, 2, 3], np.zeros((2, 3), np.int32)):
        with pytest.raises((ValueError, TypeError)):
            TetrisBatch._fork_index(stub, bad)
    assert TetrisBatch._fork_index(stub, None) is None
    got = TetrisBatch._fork_index(stub, [3, -1, 2**31 - 1, 2**40])
    assert got.dtype == torch.int32 and got.tolist() == [3, -1, 2**31 - 1, 2**31 - 1]
    keep = torch.arange(4, dtype=torch.int32)
    assert TetrisBatch._fork_index(stub, keep) is keep
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8),
                torch.zeros(4, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError):
            TetrisBatch.fork(stub, None, mask=bad)  # (index and mask are checked before src is looked at)
    with pytest.raises(TypeError):
        TetrisBatch.fork(stub, object())
    for bad in (0, -2, 1.5, True, None):
        with pytest.raises(ValueError):
            TetrisBatch.fork_groups(stub, bad)


def test_branch_layout_against_a_triple_loop():
    from gym_simpletetris_amd.search import branch_layout
    for R, S, M in ((1, 1, 1), (2, 64, 2), (3, 40, 1), (5, 7, 3)):
        root, slot, sample = branch_layout(R, S, M)
        want = [(r, s, m) for r in range(R) for s in range(S) for m in range(M)]
        assert [tuple(x) for x in zip(root.tolist(), slot.tolist(), sample.tolist())] == want
        assert all(a.dtype == np.int32 and a.shape == (R * S * M,) for a in (root, slot, sample))
        j = (root.astype(np.int64) * S + slot) * M + sample
        assert np.array_equal(j, np.arange(R * S * M))
    for bad in ((0, 4, 1), (2, 0, 1), (2, 4, 0)):
        with pytest.raises(ValueError):
            branch_layout(*bad)


def test_choose_takes_the_lowest_best_valid_slot():
    import torch
    from gym_simpletetris_amd.search import choose
    inf = float("inf")
    values = torch.tensor([[1.0, 3.0, 3.0, -inf], [-inf, -inf, -inf, -inf], [9.0, -2.0, -2.0, -5.0],
                           [-inf, -100.0, -inf, -100.0]])
    valid = torch.tensor([[True, True, True, False], [False] * 4, [False, True, True, True],
                          [False, True, False, True]])
    got = choose(values, valid)
    assert got.dtype == torch.int32 and got.tolist() == [1, -1, 1, 1]


# ------------------------------------------------------------------ the reference's two copies
KW = dict(width=6, height=9)


def _aged(n, seed0, steps=25, **kw):
    ob = O.OracleBatch(n, [seed0 + e for e in range(n)], **dict(KW, **kw))
    ob.reset()
    rng = np.random.default_rng(seed0)
    ob.rollout(np.where(rng.random((steps, n)) < 0.5, 2, rng.integers(0, 7, (steps, n))).astype(np.uint8))
    return ob


def _bytes(ob):
    return np.frombuffer(ob.envs, dtype=np.uint8).reshape(ob.n, -1).copy()


def test_the_whole_copy_steps_like_its_source():
    src, dst = _aged(6, 8100), _aged(9, 8200, steps=5)
    index = np.array([5, 0, 0, -1, 6, 3, 2, 2**31 - 1, 1])
    mask = np.array([1, 1, 1, 1, 1, 0, 1, 1, 1], np.uint8)
    before_src, before_dst = _bytes(src), _bytes(dst)
    wr = FK.fork(dst, src, index, mask)
    assert wr.tolist() == [True, True, True, False, False, False, True, False, True]
    assert np.array_equal(_bytes(src), before_src)
    assert np.array_equal(_bytes(dst)[~wr], before_dst[~wr])
    assert np.array_equal(_bytes(dst)[wr], before_src[index[wr]])  # (one configuration here)
    # every written env now plays its source's game: the source itself, driven by the copy's actions
    acts = np.random.default_rng(3).integers(0, 7, (30, 9)).astype(np.uint8)
    a = dst.rollout(acts)
    for e in np.flatnonzero(wr):
        one = O.OracleBatch(1, [0], **KW)
        ctypes.memmove(ctypes.byref(one.envs[0]), ctypes.byref(src.envs[int(index[e])]), ctypes.sizeof(O.Env))
        b = one.rollout(acts[:, e:e + 1])
        for k in ("reward", "done", "obs", "stats"):
            assert np.array_equal(a[k][:, e], b[k][:, 0]), (k, e)
        assert bytes(dst.envs[e]) == bytes(one.envs[0])


def test_the_copy_without_rng_keeps_its_own_stream():
    src = _aged(4, 8300, penalise_holes=True)
    dst = _aged(4, 8400, steps=7)  # another configuration: it stays dst's
    rng0 = np.ctypeslib.as_array(dst.envs)["rng"].copy()
    cfg0 = _bytes(dst)[:, :ctypes.sizeof(O.Config)]
    FK.fork(dst, src, [1, 1, 3, 0], [1, 0, 1, 1], keep_rng=True)
    rng1 = np.ctypeslib.as_array(dst.envs)["rng"]
    assert np.array_equal(rng1["index"], rng0["index"]) and np.array_equal(rng1["mt"], rng0["mt"])
    assert np.array_equal(_bytes(dst)[:, :ctypes.sizeof(O.Config)], cfg0) and dst.envs[0].cfg.penalise_holes == 0
    ps, pd = src.packed_state(), dst.packed_state()
    for e, s in ((0, 1), (2, 3), (3, 0)):
        for k in ps:
            assert np.array_equal(pd[k][..., e], ps[k][..., s]), (k, e)
    # in place: a group broadcast reads every root as it was
    roots = _bytes(src)[[0, 0, 2, 2]]
    FK.fork(src, src, [0, 0, 2, 2], [0, 1, 0, 1])
    assert np.array_equal(_bytes(src), roots)
