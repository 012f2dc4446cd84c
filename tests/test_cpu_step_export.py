"""The parts of st_step_export and TetrisEngine that need no GPU."""
import ctypes

from oracle import oracle as O


def test_step_export_null_context_is_einval():
    from gym_simpletetris_amd import _lib as C
    L = C.load()
    buf = (ctypes.c_uint32 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.st_step_export(None, p, 0, 0, p, p, p, p, None) == C.ST_EINVAL
    assert b"st_step_export" in L.st_last_error()


def test_engine_cell_table_is_the_rotation_rule():
    from gym_simpletetris_amd.envs.tetris_engine import CELLS
    assert len(CELLS) == 7 and all(len(r) == 4 for r in CELLS)
    for sid in range(7):
        for rot in range(4):
            want = [tuple(c) for c in O.rotate_cells(O.BASE_SHAPES[sid], rot)]
            assert [tuple(c) for c in CELLS[sid][rot]] == want, (sid, rot)


def test_tetris_engine_is_exported():
    import gym_simpletetris_amd as G
    from gym_simpletetris_amd.envs import TetrisEngine
    assert G.TetrisEngine is TetrisEngine
    assert TetrisEngine.step.__doc__ and TetrisEngine.clear.__doc__


def test_missing_symbol_is_an_import_error_that_says_rebuild(monkeypatch):
    """A library built before an addition that kept the ABI number (a stale
    build) is refused when its symbols are bound: ImportError, not a bare
    AttributeError at the first call."""
    import pytest
    from gym_simpletetris_amd import _lib as C
    C.load()
    monkeypatch.setattr(C, "_lib", None)
    monkeypatch.setitem(C.SIG, "st_added_after_this_build", ([], ctypes.c_int))
    with pytest.raises(ImportError, match="rebuild"):
        C.load()
