"""ctypes binding of libsimpletetris.so (include/simpletetris.h).

There is deliberately no CPU fallback: if the in-tree HIP library is missing
or cannot be loaded, importing the engine raises.  Build it with
`make -C gym-simpletetris_amd/csrc` (or `python -c "import __graft_entry__ as g; g.build()"`).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ST_LIB overrides the library path (a custom or variant build).  A build of
# another ABI version is refused unless ST_AB_OLD_ABI=1 (diagnostic A/Bs of
# older builds only: then missing entry points are tolerated and st_state is
# disabled, with a warning).
LIB_PATH = os.environ.get("ST_LIB") or os.path.join(_HERE, "libsimpletetris.so")

ST_OK, ST_EINVAL, ST_ENOMEM, ST_EHIP, ST_ESTATE = 0, -1, -2, -3, -4
ABI_VERSION = 4  # ST_ABI_VERSION of include/simpletetris.h

# st_flags (include/simpletetris.h) keyed by the reference kwarg names
# (TetrisEngine.__init__, tetris_env.py:126-137).
FLAGS = {
    "reward_step": 1 << 0,
    "penalise_height": 1 << 1,
    "penalise_height_increase": 1 << 2,
    "advanced_clears": 1 << 3,
    "high_scoring": 1 << 4,
    "penalise_holes": 1 << 5,
    "penalise_holes_increase": 1 << 6,
    "step_reset": 1 << 7,
}
AUTORESET = {"none": 0, "same_step": 1}

# st_stat rows
STAT = dict(time=0, score=1, lines=2, holes=3, piece_height=4, deaths=5, count0=6, mt_index=13,
            piece=14, ep_time=15, ep_score=16, ep_lines=17, ep_holes=18)
NSTAT = 19
MT_N = 624
EXPORT_MT, EXPORT_OBS_F32 = 1, 2  # st_export_env parts
# st_after_feat: the feature rows of st_afterstates, by name
AFTER = dict(valid=0, y=1, lines=2, holes=3, height=4, rows=5, above=6, dead=7, reward=8, agg_height=9,
             bumpiness=10)
AFTER_NFEAT = 11
# st_after_ext: the rows ST_FEATS_BCTS adds behind AFTER's, by name -> extended row index
AFTER_EXT = dict(landing2=11, eroded=12, row_trans=13, col_trans=14, wells=15, hole_depth=16, hole_rows=17)
AFTER_BCTS = {**AFTER, **AFTER_EXT}  # the 18 rows of ST_FEATS_BCTS, in row order
FEATURE_SETS = dict(base=0, bcts=1)  # st_feature_set
FEATURE_NAMES = {"base": AFTER, "bcts": AFTER_BCTS}  # feature set -> its rows by name
REACH_MAX_LOCK = 3  # ST_REACH_MAX_LOCK: the largest lock_delay st_reachable / st_route_actions take
ROUTE_MAX, ROUTE_WORDS = 42, 2  # ST_ROUTE_MAX, ST_ROUTE_WORDS: a packed route's actions and uint64 words
FORK_KEEP_RNG = 1 << 0  # st_fork_flags: ST_FORK_KEEP_RNG
NTUPLE_MAX_TUPLES, NTUPLE_MAX_BITS = 4096, 16  # ST_NTUPLE_MAX_TUPLES, ST_NTUPLE_MAX_BITS


class StError(RuntimeError):
    """A C-ABI call returned a negative st_status."""

    def __init__(self, code, msg):
        super().__init__(f"[st {code}] {msg}")
        self.code = code


class Config(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("lock_delay", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("autoreset", ctypes.c_int32)]


class StateViews(ctypes.Structure):
    _fields_ = [("board", ctypes.c_void_p), ("piece", ctypes.c_void_p),
                ("stats", ctypes.c_void_p), ("mt", ctypes.c_void_p),
                ("n_envs", ctypes.c_int64), ("stride", ctypes.c_int64),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("mt_pitch", ctypes.c_int64)]


# every function of include/simpletetris.h: (argument types, result type)
_vp, _i32, _i64, _u32, _u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
SIG = {
    "st_create": ([ctypes.POINTER(_vp), ctypes.POINTER(Config), ctypes.c_int, _i64], ctypes.c_int),
    "st_destroy": ([_vp], ctypes.c_int),
    "st_seed": ([_vp, _vp, _vp], ctypes.c_int),
    "st_reset": ([_vp, _vp, _vp], ctypes.c_int),
    "st_step": ([_vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_step_f32": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_step_n": ([_vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_step_vec": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_rollout": ([_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_wire_words": ([_i32, _i32], ctypes.c_int),
    "st_step_wire": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "st_unwire": ([_i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_unwire_shards": ([_i32, _i32, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_obs_to_f32": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "st_render": ([_vp, _vp, _vp], ctypes.c_int),
    "st_grayscale": ([_vp, _vp, _i32, _i32, _i32, _vp, _vp], ctypes.c_int),
    "st_state": ([_vp, ctypes.POINTER(StateViews)], ctypes.c_int),
    "st_copy": ([_vp, _vp, _i64, _vp], ctypes.c_int),
    "st_mt_sync": ([_vp, _vp], ctypes.c_int),
    "st_state_bytes": ([_vp], _i64),
    "st_save": ([_vp, _vp, _i64], ctypes.c_int),
    "st_load": ([_vp, _vp, _i64], ctypes.c_int),
    "st_export_env": ([_vp, _i64, _vp, _vp, _vp, _u32, _vp, _vp], ctypes.c_int),
    "st_export_words": ([_i32, _i32], ctypes.c_int),
    "st_step_export": ([_vp, _vp, _i64, _u32, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_check_actions": ([_vp, _i64, _vp, _vp], ctypes.c_int),
    "st_set_action_flag": ([_vp, _vp], ctypes.c_int),
    "st_gate_actions": ([_vp, _vp, _vp], ctypes.c_int),
    "st_gate_wait": ([_vp], ctypes.c_int),
    "st_stream_sync": ([_vp], ctypes.c_int),
    "st_host_device_ptr": ([_vp, ctypes.POINTER(_vp)], ctypes.c_int),
    "st_stream_wait": ([_vp, _vp], ctypes.c_int),
    "st_gen_actions": ([_vp, _i64, _i64, _u64, _i64, _vp], ctypes.c_int),
    "st_policy_greedy": ([_vp, _u64, _i64, ctypes.c_uint32, _vp, _vp], ctypes.c_int),
    "st_after_slots": ([_i32], ctypes.c_int),
    "st_afterstates": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "st_placement_actions": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "st_reachable": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "st_route_actions": ([_vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_policy_linear": ([_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_play_linear": ([_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_place": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "st_step_placements": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_play_linear_placements": ([_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_feature_rows": ([_i32], ctypes.c_int),
    "st_afterstates_set": ([_vp, _i32, _vp, _vp, _vp], ctypes.c_int),
    "st_policy_linear_set": ([_vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_play_linear_set": ([_vp, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_next_piece": ([_vp, _vp, _vp], ctypes.c_int),
    "st_policy_lookahead": ([_vp, _i32, _vp, _vp, _i64, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
                            ctypes.c_int),
    "st_play_lookahead": ([_vp, _i32, _vp, _vp, _i64, ctypes.c_float, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
                          ctypes.c_int),
    "st_next_weights": ([_vp, _vp, _vp], ctypes.c_int),
    "st_policy_expect": ([_vp, _i32, _vp, _vp, _i64, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
                         ctypes.c_int),
    "st_play_expect": ([_vp, _i32, _vp, _vp, _i64, ctypes.c_float, _i64, _vp, _vp, _vp, _vp, _vp, _vp],
                       ctypes.c_int),
    "st_routes": ([_vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_policy_routed": ([_vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_play_routed": ([_vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_fork": ([_vp, _vp, _vp, _vp, _u32, _vp], ctypes.c_int),
    "st_lock_set": ([_vp, _vp, _vp, _i64, _vp, _vp], ctypes.c_int),
    "st_afterstates_at": ([_vp, _i32, _vp, _i64, _vp, _vp, _vp], ctypes.c_int),
    "st_routes_at": ([_vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_policy_locks": ([_vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_play_locks": ([_vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_ntuple_set": ([_vp, _vp, _i32], ctypes.c_int),
    "st_ntuple_table_len": ([_vp], _i64),
    "st_ntuple_eval": ([_vp, _vp, _vp, _i64, _vp, _vp, _vp], ctypes.c_int),
    "st_policy_ntuple": ([_vp, _i32, _vp, _i64, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
                         ctypes.c_int),
    "st_play_ntuple": ([_vp, _i32, _vp, _i64, _vp, ctypes.c_float, _i64, _vp, _vp, _vp, _vp, _vp, _vp], ctypes.c_int),
    "st_debug_stamps": ([_vp, _vp, _i64], ctypes.c_int),
    "st_last_error": ([], ctypes.c_char_p),
    "st_abi_version": ([], ctypes.c_int),
}
EXPORTS = tuple(SIG)


_lib = None


def load(path: str = LIB_PATH):
    """Load the HIP engine library (raises if it is absent: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(
            f"libsimpletetris.so not found at {path}; build it with "
            "`make -C gym-simpletetris_amd/csrc` (the engine has no CPU fallback)")
    L = ctypes.CDLL(path)
    # ST_AB_OLD_ABI=1: a diagnostic A/B of an older build -- tolerate the
    # entry points it predates (never the default, not even with ST_LIB set)
    ab_override = os.environ.get("ST_AB_OLD_ABI") == "1"
    L.st_abi_version.argtypes = []
    L.st_abi_version.restype = ctypes.c_int
    abi = L.st_abi_version()
    if abi != ABI_VERSION and not ab_override:
        raise ImportError(f"{path}: libsimpletetris ABI {abi} != {ABI_VERSION} (rebuild it, or set "
                          "ST_AB_OLD_ABI=1 for a diagnostic A/B of an older build)")
    for name, (args, res) in SIG.items():
        if not hasattr(L, name):
            if ab_override:
                continue
            # an addition that did not change the ABI number (st_step_export, st_afterstates,
            # st_policy_linear, st_place, st_reachable, st_afterstates_set, st_next_piece, st_routes,
            # st_fork, st_next_weights, st_lock_set, st_ntuple_set):
            # the library on disk was built before it
            raise ImportError(f"{path}: no symbol {name} (a stale build of ABI {abi}: rebuild it with "
                              "`make -C gym-simpletetris_amd/csrc`)")
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    if abi != ABI_VERSION:
        import warnings
        warnings.warn(f"ST_AB_OLD_ABI=1: {path} has ABI {abi}, this package {ABI_VERSION}; "
                      "st_state disabled (raw ctypes A/Bs only)")
        # the state-view struct may differ across ABIs: an older build
        # serves raw ctypes A/Bs only (views read through the wrong struct
        # size tensors from garbage)
        L.st_state = None
    _lib = L
    return L


def check_count(rc: int) -> int:
    """A non-negative count, or the library's error for a negative code."""
    if rc < 0:
        check(rc)
    return rc


def check(rc: int):
    if rc != ST_OK:
        msg = load().st_last_error()
        raise StError(rc, msg.decode() if msg else "")
    return rc
