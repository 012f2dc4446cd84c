"""The parts of st_place / st_step_placements / st_play_linear_placements that
need no GPU, and the conditions on the oracle samples test_gpu_placements.py
checks the engine against (placement_ref.py: no engine code runs here)."""
import ctypes
import os
import re

import pytest

import placement_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("st_place", "st_step_placements", "st_play_linear_placements")


def _lib():
    from gym_simpletetris_amd import _lib as C
    return C, C.load()


def _call(L, call, ctx, arg):
    """The call with `arg` as its slots (or weights) and one output buffer."""
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    if call == "st_place":
        return L.st_place(ctx, arg, p, None)
    if call == "st_step_placements":
        return L.st_step_placements(ctx, arg, p, None, None, None, None)
    return L.st_play_linear_placements(ctx, arg, 1, 1, p, None, None, None, None, None)


@pytest.mark.parametrize("call", CALLS)
def test_null_context_is_einval_and_names_the_function(call):
    C, L = _lib()
    arg = ctypes.cast((ctypes.c_uint32 * 64)(), ctypes.c_void_p)
    assert _call(L, call, None, arg) == C.ST_EINVAL
    assert call.encode() in L.st_last_error()


@pytest.mark.parametrize("call", CALLS)
def test_null_slots_or_weights_are_einval(call):
    """Argument errors come before the context is used and before any GPU
    call: a zeroed block stands in for a context (were it read, it would say
    "not seeded", ST_ESTATE)."""
    C, L = _lib()
    fake = (ctypes.c_uint64 * 512)()
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    assert _call(L, call, ctx, None) == C.ST_EINVAL
    assert call.encode() in L.st_last_error()
    if call == "st_play_linear_placements":
        w = ctypes.cast((ctypes.c_float * C.AFTER_NFEAT)(), ctypes.c_void_p)
        for n_w in (0, -1, -(1 << 40)):
            assert L.st_play_linear_placements(ctx, w, n_w, 1, w, None, None, None, None, None) == C.ST_EINVAL, n_w
            assert call.encode() in L.st_last_error()


@pytest.mark.parametrize("call", CALLS)
def test_a_context_never_seeded_is_estate(call):
    """The zeroed block read as a context: not seeded, so ST_ESTATE -- still
    before any GPU call (there is no GPU here)."""
    C, L = _lib()
    fake = (ctypes.c_uint64 * 512)()
    arg = ctypes.cast((ctypes.c_uint32 * 64)(), ctypes.c_void_p)
    assert _call(L, call, ctypes.cast(fake, ctypes.c_void_p), arg) == C.ST_ESTATE
    assert call.encode() in L.st_last_error()


def test_abi_version_is_unchanged_and_the_symbols_are_bound():
    C, L = _lib()
    assert L.st_abi_version() == C.ABI_VERSION == 4
    text = open(os.path.join(ROOT, "include", "simpletetris.h")).read()
    for name in CALLS:
        assert name in C.SIG and getattr(L, name).argtypes == C.SIG[name][0], name
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_methods_reject_bad_arguments_before_any_device_call():
    from gym_simpletetris_amd.engine import TetrisBatch

    class Stub:
        n = 4
    with pytest.raises(ValueError):
        TetrisBatch.step_placements(Stub, [0] * 4, obs="f32")


# ------------------------------------------------------------------ conditions on the samples (the oracle alone)
def test_cpu_player_sample_holds_an_episode_end_a_line_and_a_fallback():
    """The run test_engine_loop_equals_the_cpu_player is held against: at
    least one episode end, one cleared line and one step without a valid slot
    (slot -1: the hard drop of the live piece)."""
    ref = P.tiny_ref()
    assert ref["done"].sum() >= 1 and ref["lines"] >= 1, (ref["done"].sum(), ref["lines"])
    none = ref["slots"] < 0
    assert none.sum() >= 1 and not ref["placed"][none].any()
    assert ref["placed"][~none].all()
    assert len(set(ref["slots"].ravel().tolist())) >= 8


@pytest.mark.parametrize("autoreset", P.AUTORESETS)
@pytest.mark.parametrize("config", sorted(P.CONFIGS))
@pytest.mark.parametrize("board", sorted(P.BOARDS))
def test_random_slot_stream_mixes_valid_and_invalid_and_holds_a_death(board, config, autoreset):
    """Between 20% and 80% of test_step_placements_against_the_oracle's slots
    are valid, for every board and config, and some env dies."""
    ref = P.random_run(board, config, autoreset)
    S = 4 * (P.BOARDS[board][0] + 6)
    assert 0.2 <= ref["placed"].mean() <= 0.8, ref["placed"].mean()
    assert ref["done"].sum() >= 1
    sl = ref["slots"]
    assert (sl < 0).any() and (sl >= S).any() and sl.min() == -2 and sl.max() == S + 1
    in_range = (sl >= 0) & (sl < S)
    assert (in_range & (ref["placed"] == 0)).any()  # in range, occupied at row 0 or off the board
