"""TetrisBatch: N independent SimpleTetris engines resident on one MI355X.

Host mirror of TetrisEngine (the reference's gym_simpletetris/envs/tetris_env.py:125-335)
for N envs at once.  All game logic runs in the HIP kernels of
libsimpletetris.so (csrc/: the core and the library's own kernels in
st_kernels.hip, every planner family in a unit of its own beside it, the C
ABI in st_capi.cpp); this class only owns the context,
the output buffers (torch tensors on the device) and the stream plumbing.
"""
from __future__ import annotations

import ctypes
import os
from collections.abc import Mapping
from types import MappingProxyType
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as C

SHAPE_NAMES = ("T", "J", "L", "Z", "S", "I", "O")  # tetris_env.py:19

# Reference constructor kwargs (TetrisEngine.__init__ / TetrisEnv.__init__).
SCORING_KWARGS = ("reward_step", "penalise_height", "penalise_height_increase",
                  "advanced_clears", "high_scoring", "penalise_holes",
                  "penalise_holes_increase")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(device: torch.device) -> ctypes.c_void_p:
    """torch's current stream on `device` (the raw-handle query costs ~0.2 us
    against ~2 us for building the Stream object; per-step hot path)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(device.index))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]) -> Optional[ctypes.c_void_p]:
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _mapped(t: torch.Tensor):
    """Device address of a pinned host tensor (st_host_device_ptr, i.e.
    hipHostGetDevicePointer in the runtime the kernels use), or None if the
    runtime does not map it for the device."""
    L = C.load()
    dp = ctypes.c_void_p()
    rc = L.st_host_device_ptr(ctypes.c_void_p(t.data_ptr()), ctypes.byref(dp))
    return dp if rc == 0 and dp.value else None


class _Pinned:
    """A pinned host tensor (`host`) that a library call's result is read
    back into.  The call writes at the device address `dst`: the host tensor
    itself where the runtime maps it for the device, else (`staged`) a
    device buffer of the same size, which land(stream) then copies to the
    host tensor on the stream -- `if p.staged: p.land(s)` after the call (the
    test is the call site's: a Python call per step shows in TetrisEnv.step)."""

    def __init__(self, shape, dtype, device):
        self.host = torch.empty(shape, dtype=dtype, pin_memory=True)
        self.dst = _mapped(self.host)
        self.staged = self.dst is None
        if self.staged:
            self._dev = torch.empty(shape, dtype=dtype, device=device)
            self.dst = _ptr(self._dev)

    def land(self, s) -> None:
        C.check(C.load().st_copy(_ptr(self.host), self.dst, self.host.numel() * self.host.element_size(), s))


def scalar_action(a) -> int:
    """value_action_map[a] (tetris_env.py:152-160, :245) for one action: ints,
    bools and numpy integers index by value; a float finds a key only when it
    equals one (2.0 -> 2, as in a dict lookup); anything else raises KeyError."""
    if isinstance(a, (bool, np.bool_, int, np.integer)):
        v = int(a)
    elif isinstance(a, (float, np.floating)) and float(a).is_integer():
        v = int(a)
    else:
        raise KeyError(a)
    if not 0 <= v < 7:
        raise KeyError(a)
    return v


def _bad_actions(x):
    """Elementwise "not a key of value_action_map" for an action array, a
    numpy array or a torch tensor alike (the same rule as scalar_action:
    floats must be integral).  A numpy array is judged in numpy: torch cannot
    compare uint16 / uint32 / uint64."""
    if isinstance(x, np.ndarray):
        if x.dtype.kind not in "fiub":
            raise TypeError(f"actions must be numbers, got {x.dtype}")
        is_float, unsigned, floor = x.dtype.kind == "f", x.dtype.kind in "ub", np.floor
    else:
        is_float, unsigned, floor = x.dtype.is_floating_point, x.dtype in (torch.uint8, torch.bool), torch.floor
    if is_float:
        return ~((x >= 0) & (x <= 6) & (x == floor(x)))
    if unsigned:
        return x > 6
    return (x < 0) | (x > 6)


def _raise_bad_actions(x) -> None:
    """The reference's KeyError (tetris_env.py:245) if `x` (numpy array or
    torch tensor; on a device: one device->host sync) holds a bad action."""
    bad = _bad_actions(x)
    if bool(bad.any()):
        raise KeyError(f"action {x[bad].reshape(-1)[0].item()} not in 0..6 (tetris_env.py:245)")


def _check_tensor(t, name: str, shape, dtypes, device=None) -> None:
    """ValueError unless `t` is a contiguous torch tensor of `shape` (None:
    any extent) with one of `dtypes` on `device` (None: any GPU) -- the
    kernels read and write it through its raw pointer."""
    if not (isinstance(t, torch.Tensor) and t.dim() == len(shape) and t.dtype in dtypes and t.is_contiguous()
            and all(w is None or w == g for w, g in zip(shape, t.shape))
            and (t.device.type == "cuda" if device is None else t.device == device)):
        got = (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t)
        want = "[%s]" % ", ".join("*" if w is None else str(w) for w in shape)
        raise ValueError(f"{name}: need a contiguous {'/'.join(map(str, dtypes))} {want} tensor "
                         f"on {device or 'a GPU'}, got {got}")


def _check_out(out, width: int, n: int, device):
    """A caller's (packed obs int32 [width, n], reward int32 [n], done
    bool/uint8 [n]) output tensors on `device`, checked (_check_tensor)."""
    obs, reward, done = out
    _check_tensor(obs, "out obs", (width, n), (torch.int32,), device)
    _check_tensor(reward, "out reward", (n,), (torch.int32,), device)
    _check_tensor(done, "out done", (n,), (torch.bool, torch.uint8), device)
    return obs, reward, done


def _from_dlpack(x):
    """A foreign device array (any DLPack producer: __dlpack__ /
    __dlpack_device__, e.g. a learner's action buffer) as a torch tensor over
    the same memory -- no copy; torch tensors and numpy arrays pass through."""
    if isinstance(x, (torch.Tensor, np.ndarray)) or not hasattr(x, "__dlpack__"):
        return x
    return torch.from_dlpack(x)


def placement_slot(width: int, rot: int, x: int) -> int:
    """The placement slot of rotation `rot` (0..3 applications of
    rotated(cclk=False), tetris_env.py:22-26) at anchor column `x`
    (-3..width+2) on a board `width` wide: rot * (width + 6) + (x + 3),
    st_policy_greedy's (rot, x) loop order."""
    if not (0 <= rot < 4 and -3 <= x < width + 3):
        raise ValueError(f"rot {rot} outside 0..3 or x {x} outside -3..{width + 2}")
    return rot * (width + 6) + (x + 3)


def placement_rot_x(width: int, slot: int):
    """placement_slot's inverse: (rot, x) of a slot in [0, 4 * (width + 6))."""
    if not 0 <= slot < 4 * (width + 6):
        raise ValueError(f"slot {slot} outside [0, {4 * (width + 6)})")
    return slot // (width + 6), slot % (width + 6) - 3


def lock_pos(width: int, rot: int, x: int, y: int) -> int:
    """The lock position (ST_LOCK_POS) of rotation `rot` at anchor (x, y) on a
    board `width` wide: placement_slot(width, rot, x) * 32 + y, y in 0..31."""
    if not 0 <= y < 32:
        raise ValueError(f"y {y} outside 0..31")
    return placement_slot(width, rot, x) * 32 + y


def lock_rot_x_y(width: int, pos: int):
    """lock_pos's inverse: (rot, x, y) of a position in [0, 32 * 4 * (width + 6))."""
    if pos < 0:
        raise ValueError(f"pos {pos} < 0")
    return placement_rot_x(width, pos >> 5) + (pos & 31,)


def _row_names(rows: int):
    """The rows by name of a feature tensor with `rows` rows: _lib.AFTER, or
    _lib.AFTER_BCTS where it holds the 18 rows of features='bcts'."""
    return C.AFTER_BCTS if rows == len(C.AFTER_BCTS) else C.AFTER


def _feature_set(features):
    """(st_feature_set value, rows, rows by name) of a `features` argument."""
    if not isinstance(features, str) or features not in C.FEATURE_SETS:
        raise ValueError(f"features must be one of {', '.join(map(repr, C.FEATURE_SETS))}, got {features!r}")
    names = C.FEATURE_NAMES[features]
    return C.FEATURE_SETS[features], len(names), names


class Afterstates:
    """TetrisBatch.afterstates()'s result: `feat` int32 [n, rows, S] (rows =
    AFTER_NFEAT, or 18 with features='bcts') and `boards` int32 [n, W, S] (or
    None), slot innermost; every feature row by its name in _lib.AFTER (with 18
    rows: _lib.AFTER_BCTS) as an [n, S] view of feat (.valid, .lines, ...)."""

    def __init__(self, feat: torch.Tensor, boards: Optional[torch.Tensor]):
        self.feat, self.boards = feat, boards

    def __getattr__(self, name):  # (only names not found otherwise)
        row = _row_names(self.feat.shape[1]).get(name) if name != "feat" else None
        if row is None:
            raise AttributeError(name)
        return self.feat[:, row]


class Reachable:
    """TetrisBatch.reachable()'s result: `steps` int32 [n, S] (the length of the
    shortest action sequence that locks the live piece in the slot, 0 where
    none does) and `first` uint8 [n, S] (the lowest-numbered action that begins
    one, 2 where none does; None with first=False), slot innermost; `mask`
    is steps > 0."""

    def __init__(self, steps: torch.Tensor, first: Optional[torch.Tensor]):
        self.steps, self.first = steps, first

    @property
    def mask(self) -> torch.Tensor:
        return self.steps > 0


def route_pack(actions) -> np.ndarray:
    """One route's actions (a sequence of 0..6, at most ROUTE_MAX of them) as
    its ROUTE_WORDS uint64 words: action i at bits 3 * (i % 21) .. + 2 of word
    i // 21, every field behind the last one 7, bit 63 clear."""
    acts = [int(a) for a in actions]
    if len(acts) > C.ROUTE_MAX or any(a < 0 or a > 6 for a in acts):
        raise ValueError(f"a route is at most {C.ROUTE_MAX} actions in 0..6")
    words = [(1 << 63) - 1] * C.ROUTE_WORDS
    for i, a in enumerate(acts):
        words[i // 21] ^= (7 - a) << (3 * (i % 21))
    return np.array(words, np.uint64)


def route_unpack(words) -> list:
    """route_pack's inverse: the actions of one route (its ROUTE_WORDS words,
    uint64 or the int64 a Routes holds) up to the first field that holds 7."""
    acts = []
    for w in np.asarray(words).astype(np.uint64).tolist():
        for j in range(21):
            a = (w >> (3 * j)) & 7
            if a == 7:
                return acts
            acts.append(a)
    return acts


class Routes:
    """TetrisBatch.routes()'s result: `route` int64 [ROUTE_WORDS, n] -- the
    library's uint64 words, whose bit 63 is 0 -- and `steps` int32 [n], the
    route's true length (0: the slot cannot be served, every field is 7).
    action(i): the i-th action of every env, uint8 [n] (7 past a route's end);
    `length`: the actions the words hold, min(steps, ROUTE_MAX)."""

    def __init__(self, route: torch.Tensor, steps: torch.Tensor):
        self.route, self.steps = route, steps

    def action(self, i: int) -> torch.Tensor:
        if not 0 <= i < C.ROUTE_MAX:
            raise IndexError(f"a route holds actions 0..{C.ROUTE_MAX - 1}")
        return ((self.route[i // 21] >> (3 * (i % 21))) & 7).to(torch.uint8)

    @property
    def length(self) -> torch.Tensor:
        return self.steps.clamp(max=C.ROUTE_MAX)


class RoutedChoice:
    """TetrisBatch.policy_routed()'s result: `slots` int32 [n] (-1: no
    reachable candidate), `routes` (a Routes) and `scores` float32 [n]."""

    def __init__(self, slots, routes, scores):
        self.slots, self.routes, self.scores = slots, routes, scores

    def __iter__(self):
        return iter((self.slots, self.routes, self.scores))


class LockSet:
    """TetrisBatch.lock_set()'s result: `rows` int32 [n, S] (bit y of word
    (e, s): the piece locks at row y of slot s; None with rows=False), `pos`
    int32 [n, cap] (the env's lock positions, ascending, -1 behind the last;
    None without a cap) and `count` int32 [n], the true count."""

    def __init__(self, rows, pos, count):
        self.rows, self.pos, self.count = rows, pos, count


class LockChoice:
    """TetrisBatch.policy_locks()'s result: `pos` int32 [n] (-1: no lock
    position), `routes` (a Routes), `scores` float32 [n], `feat` int32
    [rows, n] (the chosen position's feature rows, by name as LinearChoice's)
    and `count` int32 [n], the env's lock positions."""

    def __init__(self, pos, routes, scores, feat, count):
        self.pos, self.routes, self.scores, self.feat, self.count = pos, routes, scores, feat, count

    def __getattr__(self, name):  # (only names not found otherwise)
        feat = None if name == "feat" else self.feat
        row = None if feat is None else _row_names(feat.shape[0]).get(name)
        if row is None:
            raise AttributeError(name)
        return feat[row]


# st_policy_greedy's score as linear feature weights: 80 * lines - 12 * holes
# - 3 * height - 2000 * above (rows by their names in _lib.AFTER)
GREEDY_WEIGHTS = MappingProxyType(dict(lines=80.0, holes=-12.0, height=-3.0, above=-2000.0))
# Dellacherie's six-feature player and Thiery & Scherrer's BCTS player as weights over
# the rows of features='bcts' (_lib.AFTER_BCTS).  The published landing-height weight
# (-1 / -12.63) is halved, since the row `landing2` is twice the landing height.  The
# values were written down from memory of the published tables, not copied from the
# papers: check them against the sources before quoting results obtained with them.
DELLACHERIE_WEIGHTS = MappingProxyType(dict(landing2=-0.5, eroded=1.0, row_trans=-1.0, col_trans=-1.0, holes=-4.0,
                                            wells=-1.0))
BCTS_WEIGHTS = MappingProxyType(dict(landing2=-6.315, eroded=6.60, row_trans=-9.22, col_trans=-19.77, holes=-13.08,
                                     wells=-10.49, hole_depth=-1.61, hole_rows=-24.04))


def weight_rows(weights, features: str = "base") -> np.ndarray:
    """Host weights for policy_linear / play_linear as float32 [n_w, rows], rows =
    AFTER_NFEAT (features='bcts': 18): a mapping by the set's row names
    (_lib.AFTER / _lib.AFTER_BCTS; missing names are 0; the header's enum order
    places the values), a sequence of `rows` numbers, or a sequence of such
    mappings / sequences (one row per candidate)."""
    _, nrows, names = _feature_set(features)

    def row(w):
        if isinstance(w, Mapping):
            unknown = sorted(set(w) - set(names))
            if unknown:
                raise ValueError(f"weights: no feature row named {unknown[0]!r} (rows: {', '.join(names)})")
            v = np.zeros(nrows, np.float32)
            for name, val in w.items():
                v[names[name]] = val
            return v
        w = np.asarray(w)
        if w.shape != (nrows,):
            raise ValueError(f"weights: a row needs {nrows} values, got shape {w.shape}")
        return w
    if isinstance(weights, Mapping):
        out = row(weights)
    elif isinstance(weights, (list, tuple)) and any(isinstance(w, Mapping) for w in weights):
        out = np.stack([row(w) for w in weights])
    elif isinstance(weights, (list, tuple, np.ndarray)):
        out = np.asarray(weights)
    else:
        raise TypeError(f"weights: need a tensor, a sequence or a mapping by feature name, got {type(weights)}")
    if out.dtype.kind not in "fiu":
        raise TypeError(f"weights must be real numbers, got {out.dtype}")
    out = out.astype(np.float32)
    out = out[None] if out.ndim == 1 else out
    if out.ndim != 2 or out.shape[1] != nrows or out.shape[0] < 1:
        raise ValueError(f"weights: need [{nrows}] or [n_w, {nrows}] values, got shape {np.shape(weights)}")
    return np.ascontiguousarray(out)


class LinearChoice:
    """TetrisBatch.policy_linear()'s result: `slots` int32 [n] (-1: no valid
    slot), `actions` uint8 [n] (as step() takes them), `scores` float32 [n] and
    `feat` int32 [rows, n] (rows = AFTER_NFEAT, or 18 with features='bcts'), the
    chosen slot's feature rows with the env innermost; every row by its name in
    _lib.AFTER (with 18 rows: _lib.AFTER_BCTS) as an [n] view of feat (.lines,
    .holes, ...).  A field not asked for (`out`) is None."""

    def __init__(self, slots, actions, scores, feat):
        self.slots, self.actions, self.scores, self.feat = slots, actions, scores, feat

    def __getattr__(self, name):  # (only names not found otherwise)
        feat = None if name == "feat" else self.feat
        row = None if feat is None else _row_names(feat.shape[0]).get(name)
        if row is None:
            raise AttributeError(name)
        return feat[row]


class NTupleChoice(LinearChoice):
    """TetrisBatch.policy_ntuple()'s result: LinearChoice's `slots`, `actions`,
    `scores` and `feat` (with its rows by name), and `values` float32 [n] (V of
    the chosen slot: the network's value of its afterstate board, dead_value
    where it ends the game, 0 without a slot); with index=True `index` int32
    [T, n] (the table entries the value was read from, env innermost; -1 rows
    where no slot was chosen or the chosen slot is dead) and with
    values_all=True `values_all` float32 [n, S] (V of every candidate, 0.0
    elsewhere), else None.  A field not asked for (`out`) is None."""

    def __init__(self, slots, actions, scores, feat, values=None, index=None, values_all=None):
        super().__init__(slots, actions, scores, feat)
        self.values, self.index, self.values_all = values, index, values_all


class LookaheadChoice:
    """TetrisBatch.policy_lookahead()'s result: `slots` int32 [n] (the chosen
    first-ply slot, -1: no candidate), `slots2` int32 [n] (the best second-ply
    slot behind it, -1: none), `actions` uint8 [n] (as step() takes them) and
    `scores` float32 [n]; with table=True also `scores_all` float32 [n, S] and
    `slots2_all` int32 [n, S], the score and best second-ply slot of every
    candidate (0.0 / -1 elsewhere), else None.  A field not asked for (`out`) is
    None."""

    def __init__(self, slots, slots2, actions, scores, scores_all=None, slots2_all=None):
        self.slots, self.slots2, self.actions, self.scores = slots, slots2, actions, scores
        self.scores_all, self.slots2_all = scores_all, slots2_all


class ExpectChoice:
    """TetrisBatch.policy_expect()'s result: `slots` int32 [n] (the chosen
    first-ply slot, -1: no candidate), `actions` uint8 [n] (as step() takes
    them) and `scores` float32 [n]; with table=True also `scores_all` float32
    [n, S] (every candidate's score, 0.0 elsewhere), `tails` float32 [n, 7, S]
    (T_q(s1): the best second-ply score behind s1 for every piece q in
    SHAPE_NAMES order, 0.0 elsewhere) and `slots2_all` int32 [n, 7, S] (that
    piece's best second-ply slot, -1 where there is none), else None.  A field
    not asked for (`out`) is None."""

    def __init__(self, slots, actions, scores, scores_all=None, tails=None, slots2_all=None):
        self.slots, self.actions, self.scores = slots, actions, scores
        self.scores_all, self.tails, self.slots2_all = scores_all, tails, slots2_all


def _dead_value(dead_value) -> float:
    """policy_lookahead's / play_lookahead's dead_value as a finite float."""
    if isinstance(dead_value, bool) or not isinstance(dead_value, (int, float, np.integer, np.floating)):
        raise TypeError(f"dead_value must be a real number, got {type(dead_value)}")
    with np.errstate(over="ignore"):
        v = float(np.float32(dead_value))
    if not np.isfinite(v):
        raise ValueError(f"dead_value must be finite in float32, got {dead_value!r}")
    return v


class TetrisBatch:
    """Batched engine.  `autoreset`: 'none' (exact reference semantics; the
    caller resets done envs, like `if done: env.reset()`) or 'same_step'
    (clear() runs inside the step kernel for envs that died)."""

    def __init__(self, n_envs: int, width: int = 10, height: int = 20, lock_delay: int = 0,
                 step_reset: bool = False, reward_step: bool = False,
                 penalise_height: bool = False, penalise_height_increase: bool = False,
                 advanced_clears: bool = False, high_scoring: bool = False,
                 penalise_holes: bool = False, penalise_holes_increase: bool = False,
                 autoreset: str = "none", device=None, seeds: Optional[Sequence[int]] = None,
                 validate_actions: bool = True):
        self._L = C.load()
        if not torch.cuda.is_available():
            raise RuntimeError("TetrisBatch needs a ROCm GPU (no CPU fallback by design)")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if autoreset not in C.AUTORESET:
            raise ValueError(f"autoreset must be one of {sorted(C.AUTORESET)}")
        kw = dict(reward_step=reward_step, penalise_height=penalise_height,
                  penalise_height_increase=penalise_height_increase,
                  advanced_clears=advanced_clears, high_scoring=high_scoring,
                  penalise_holes=penalise_holes,
                  penalise_holes_increase=penalise_holes_increase, step_reset=step_reset)
        flags = 0
        for k, v in kw.items():
            if v:
                flags |= C.FLAGS[k]
        self.n = int(n_envs)
        self.width, self.height = int(width), int(height)
        self.lock_delay = int(lock_delay)
        self.flags = flags
        self.kwargs = dict(kw, lock_delay=self.lock_delay, width=self.width, height=self.height)
        self.autoreset = autoreset
        self.device = device
        # step()/rollout() reject actions outside 0..6 like the reference's
        # value_action_map[action] KeyError (tetris_env.py:245).  For a device
        # tensor that check costs one device->host sync per call;
        # validate_actions=False skips it (values >= 7 then act as idle), and
        # 'async' lets the step kernel check the actions it loads anyway (a
        # sticky flag in mapped host memory, st_set_action_flag) without a
        # sync: the KeyError comes at the next step()/rollout() after the flag
        # is seen, or from check_actions().
        if validate_actions not in (True, False, "async"):
            raise ValueError("validate_actions must be True, False or 'async'")
        self.validate_actions = validate_actions
        self._flag_h = self._flag_dev = None
        cfg = C.Config(self.width, self.height, self.lock_delay, flags, C.AUTORESET[autoreset])
        ctx = ctypes.c_void_p()
        with torch.cuda.device(device):
            C.check(self._L.st_create(ctypes.byref(ctx), ctypes.byref(cfg), device.index, self.n))
        self._ctx = ctx
        if validate_actions == "async":
            # the step kernels' own action check (st_set_action_flag) into a
            # sticky word of pinned host memory mapped for the device
            self._flag_h = torch.zeros(1, dtype=torch.int32, pin_memory=True)
            self._flag_np = self._flag_h.numpy()
            self._flag_dev = _mapped(self._flag_h)
            if self._flag_dev is None:
                raise RuntimeError("validate_actions='async' needs pinned host memory mapped for the device")
            C.check(self._L.st_set_action_flag(ctx, self._flag_dev))
        v = C.StateViews()
        C.check(self._L.st_state(ctx, ctypes.byref(v)))
        self._views = v
        self.stride = int(v.stride)
        W, n = self.width, self.n
        # Reused output buffers (valid until the next step, like a vec-env obs buffer).
        self.obs = torch.zeros((W, n), dtype=torch.int32, device=device)  # packed u32 bits
        self.obs_f32: Optional[torch.Tensor] = None
        self.reward = torch.zeros(n, dtype=torch.int32, device=device)
        self.done = torch.zeros(n, dtype=torch.bool, device=device)
        self._act = torch.zeros(n, dtype=torch.uint8, device=device)
        self._place_act: Optional[torch.Tensor] = None  # placement_actions' reused output (made on first use)
        self._route_act: Optional[torch.Tensor] = None  # route_actions' reused output (made on first use)
        self.placed: Optional[torch.Tensor] = None  # place() / step_placements(): uint8 [n] commit flags (made on first use)
        self._fork_groups: dict = {}  # fork_groups' (index, mask) device tensors by group size
        self._ntuple = None  # set_ntuple's network (the library holds its own copy of the tuples)
        self._seeded = False
        if seeds is not None:
            self.seed(seeds)

    # ------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self._L.st_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return _stream_ptr(self.device)

    def seed(self, seeds: Sequence[int]):
        """random.seed(seeds[e]) for each env (CPython MT19937 init_by_array)."""
        s = np.asarray([int(x) for x in seeds], dtype=object)
        if len(s) != self.n:
            raise ValueError(f"need {self.n} seeds, got {len(s)}")
        arr = np.empty(self.n, np.uint64)
        for i, x in enumerate(s):
            x = abs(int(x))  # random.seed uses abs() of an int seed
            if x >= 1 << 64:
                raise ValueError("seeds must fit in 64 bits")
            arr[i] = x
        with torch.cuda.device(self.device):
            C.check(self._L.st_seed(self._ctx, ctypes.c_void_p(arr.ctypes.data), self._stream()))
        self._seeded = True

    def _intake(self, x, shape, name="actions"):
        """`x` (torch tensor, DLPack producer, numpy array or anything numpy
        takes) as a torch tensor -- a device array over the same memory, no
        copy -- or a numpy array, of as many real numbers as `shape` holds."""
        x = _from_dlpack(x)
        if not isinstance(x, torch.Tensor):
            x = np.asarray(x)
        elif x.is_complex():
            raise TypeError(f"{name} must be real numbers, got {x.dtype}")
        if np.prod(x.shape) != np.prod(shape):
            raise ValueError(f"{name} must have shape {shape}, got {tuple(x.shape)}")
        return x

    def _to_dev_u8(self, x, shape, keep_bad: bool = False) -> torch.Tensor:
        """_intake's array as a contiguous uint8 tensor of `shape` on the
        engine's device (itself if it is one).  The cast wraps; `keep_bad`
        keeps the bad actions of a tensor visible to a check on the device
        as 255."""
        if isinstance(x, np.ndarray):
            return torch.as_tensor(x.astype(np.uint8).reshape(shape), device=self.device)
        if x.dtype == torch.uint8 and x.device == self.device:
            t = x
        else:
            t = x.to(device=self.device).to(torch.uint8)
            if keep_bad:  # keep bad values visible to the kernel's check: a cast
                # may wrap them into 0..6 (int16 256 -> 0, 2.5 -> 2); the sentinel is set after
                # the cast, in uint8, so no source dtype has to hold 255 (int8 cannot)
                t = t.masked_fill_(_bad_actions(x).to(self.device), 255)
        return t.reshape(shape).contiguous()

    def _action_check(self, on_dev: bool, can_gate: bool) -> str:
        """Which check the reference's KeyError for an action outside
        value_action_map (tetris_env.py:152-160, :245) comes from:
          'host'   the input is not on the engine's device: checked where it
                   lives, before anything is launched, whatever the mode;
          'sync'   validate_actions=True at an entry point that cannot gate
                   (rollouts, step_wire): on the device, one device->host sync;
          'gate'   True at step() / the vector env's step: st_gate_actions
                   (_gated_launch: the step is skipped entirely if an action
                   was bad; the host waits for the check kernel only);
          'kernel' 'async': the step kernel itself (st_set_action_flag: it sets
                   a sticky word in mapped host memory when an action is > 6,
                   polled by _raise_flagged without a sync);
          'none'   False: no check (values > 6 act as idle)."""
        if not on_dev:
            return "host"
        if self.validate_actions == "async":
            return "kernel"
        if self.validate_actions is True:
            return "gate" if can_gate else "sync"
        return "none"

    def _actions(self, x, lead=(), gate: bool = False):
        """(actions as a contiguous uint8 device tensor of shape lead + (n,),
        gated).  A uint8 cast would wrap -1 to 255 and 263 to 7, so the values
        are checked BEFORE it, by the check _action_check names; `gate` says
        that the caller can gate its launch, and `gated` that it has to
        (_gated_launch).  The checks on the device ('gate', 'kernel') see
        uint8: bad values of other dtypes reach them as 255."""
        shape = tuple(lead) + (self.n,)
        mode = self.validate_actions
        if mode == "async":
            self._raise_flagged()
        if (type(x) is torch.Tensor and x.dtype == torch.uint8 and x.device == self.device
                and x.is_contiguous() and tuple(x.shape) == shape):
            # an RL loop's own device buffer, as it is: checked in the step
            # kernel ('async'), by the gate (True), or not at all
            if mode is not True:
                return x, False
            if gate:
                return x, True
        x = self._intake(x, shape)
        check = self._action_check(isinstance(x, torch.Tensor) and x.device == self.device, gate)
        if check in ("host", "sync"):
            _raise_bad_actions(x)
        return self._to_dev_u8(x, shape, keep_bad=check in ("gate", "kernel")), check == "gate"

    def _gated_launch(self, a: torch.Tensor, s, fn, args) -> None:
        """The step launch fn(*args) on stream s behind st_gate_actions' check
        of `a` (for a step _actions returned as gated): that launch skips
        every env if an action is outside 0..6; then st_gate_wait -- the host
        waits for the check, not for the step behind it -- and the
        reference's KeyError (tetris_env.py:245): the step changed nothing.
        An ungated step is C.check(fn(*args)) at the call site: a Python call
        more per step shows in the vector env's step time."""
        C.check(self._L.st_gate_actions(self._ctx, _ptr(a), s))
        try:
            C.check(fn(*args))
        finally:  # st_gate_wait ends the gate, also when the launch raised (its answer is
            # moot then): it cannot gate a later step
            rc = self._L.st_gate_wait(self._ctx)
        if rc < 0:
            C.check(rc)
        if rc:
            raise KeyError("an action outside 0..6 (tetris_env.py:245); no env was stepped")

    def _raise_flagged(self):
        if self._flag_np[0]:
            self._flag_np[0] = 0
            raise KeyError("an action outside 0..6 reached an earlier step (validate_actions='async'; "
                           "tetris_env.py:245); it acted as idle")

    def check_actions(self):
        """validate_actions='async': wait for the work queued so far and raise
        KeyError if any checked action was outside 0..6."""
        if self.validate_actions != "async":
            return
        torch.cuda.current_stream(self.device).synchronize()
        self._raise_flagged()

    def reset(self, mask=None):
        """TetrisEngine.clear() on every env (mask None) or where mask != 0."""
        if not self._seeded:
            raise RuntimeError("seed() before reset()")
        m = None if mask is None else self._to_dev_u8(self._intake(mask, (self.n,), "mask"), (self.n,))
        with torch.cuda.device(self.device):
            C.check(self._L.st_reset(self._ctx, _ptr(m), self._stream()))

    def step(self, actions, obs: str = "packed", out=None):
        """One TetrisEngine.step on every env.  obs: 'packed' (u32 [W][n]),
        'f32' (also float32 [n][W][H], fused in the kernel) or 'none'.
        Returns (obs, reward int32 [n], done bool [n]) -- reused buffers, or
        the caller's `out` = (packed obs int32 [W][n], reward int32 [n],
        done uint8/bool [n]) device tensors (e.g. a gather buffer's views)."""
        if obs not in ("packed", "f32", "none"):
            raise ValueError("obs must be 'packed', 'f32' or 'none'")
        a, gated = self._actions(actions, gate=True)
        o_t, r_t, d_t = (self.obs, self.reward, self.done) if out is None \
            else _check_out(out, self.width, self.n, self.device)
        s = self._stream()
        # no torch.cuda.device() context: st_step selects the context's device itself
        if obs == "f32":
            o_ret = self._f32_buffer()
            fn, args = self._L.st_step_f32, (self._ctx, _ptr(a), _ptr(o_t), _ptr(o_ret), _ptr(r_t), _ptr(d_t), s)
        else:
            o_ret = o_t if obs == "packed" else None
            fn, args = self._L.st_step, (self._ctx, _ptr(a), _ptr(o_ret), _ptr(r_t), _ptr(d_t), s)
        if gated:  # validate_actions=True, device actions
            self._gated_launch(a, s, fn, args)
        else:
            C.check(fn(*args))
        return o_ret, r_t, d_t

    def _f32_buffer(self) -> torch.Tensor:
        """The float32 obs [n][W][H] that step() and step_n() reuse (made on first use)."""
        if self.obs_f32 is None:
            self.obs_f32 = torch.zeros((self.n, self.width, self.height), dtype=torch.float32, device=self.device)
        return self.obs_f32

    def _k_actions(self, actions):
        """rollout() / step_n(): a [K, n] integer tensor (or DLPack producer),
        K >= 1, through _actions -> (uint8 device tensor [K, n], K)."""
        actions = _from_dlpack(actions)
        if not isinstance(actions, torch.Tensor) or actions.dim() != 2 or actions.shape[1] != self.n \
                or actions.shape[0] < 1:
            raise ValueError(f"actions must be a [K, {self.n}] integer tensor")
        K = int(actions.shape[0])
        return self._actions(actions, lead=(K,))[0], K

    @property
    def wire_words(self) -> int:
        """uint32 rows per env of the gather format (st_wire_words)."""
        return C.check_count(self._L.st_wire_words(self.width, self.height))

    def step_wire(self, actions, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One step (as step()) writing BASELINE C5's gather format instead
        of obs / reward / done: int32 [wire_words, n], per env column x's obs
        bits at bit x*H, then the reward's 32 bits and done
        (st_step_wire; `unwire` restores step()'s outputs bit-exactly)."""
        a, _ = self._actions(actions)
        shape = (self.wire_words, self.n)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        else:
            _check_tensor(out, "out", shape, (torch.int32,), self.device)
        C.check(self._L.st_step_wire(self._ctx, _ptr(a), _ptr(out), self._stream()))
        return out

    def rollout(self, actions: torch.Tensor, obs: str = "packed", out: Optional[dict] = None):
        """K consecutive steps in one kernel launch (st_rollout).

        actions: uint8 [K, n] on the device.  Returns (obs, reward, done) with
        a leading K dimension: packed obs int32 [K, W, n] ('packed'), float32
        [K, n, W, H] ('f32') or None ('none'); reward int32 [K, n]; done bool
        [K, n].  Identical to K calls of step().  `out` may supply the output
        tensors (keys 'obs', 'obs_f32', 'reward', 'done') to reuse buffers."""
        actions, K = self._k_actions(actions)
        out = {} if out is None else out
        W, H, n, dev = self.width, self.height, self.n, self.device

        def buf(key, shape, dtype):
            t = out.get(key)
            if t is None or tuple(t.shape) != shape or t.dtype != dtype:
                t = torch.empty(shape, dtype=dtype, device=dev)
                out[key] = t
            return t
        o = buf("obs", (K, W, n), torch.int32) if obs in ("packed", "f32") else None
        f = buf("obs_f32", (K, n, W, H), torch.float32) if obs == "f32" else None
        r = buf("reward", (K, n), torch.int32)
        d = buf("done", (K, n), torch.bool)
        with torch.cuda.device(dev):
            C.check(self._L.st_rollout(self._ctx, K, _ptr(actions), _ptr(o), _ptr(f), _ptr(r),
                                       _ptr(d), self._stream()))
        return (f if obs == "f32" else o), r, d

    def step_n(self, actions: torch.Tensor, obs: str = "packed"):
        """K consecutive steps, one st_step kernel launch each, enqueued by
        ONE library call (st_step_n: the launch loop runs in C, with no
        Python between the launches).  actions: uint8 [K, n] on the device
        (checked like rollout()'s).  Identical to K calls of step(); returns
        the LAST step's (obs, reward, done) in the engine's reused buffers
        ('packed': int32 [W, n], 'f32': float32 [n, W, H], 'none': None)."""
        if obs not in ("packed", "f32", "none"):
            raise ValueError("obs: 'packed', 'f32' or 'none'")
        actions, K = self._k_actions(actions)
        f = self._f32_buffer() if obs == "f32" else None
        row = actions.stride(0)
        base = actions.data_ptr()
        ptrs = (ctypes.c_void_p * K)(*[base + t * row for t in range(K)])
        C.check(self._L.st_step_n(self._ctx, ctypes.addressof(ptrs), K,
                                  _ptr(self.obs) if obs != "none" else None, _ptr(f),
                                  _ptr(self.reward), _ptr(self.done), self._stream()))
        if obs == "f32":
            return f, self.reward, self.done
        return (self.obs if obs == "packed" else None), self.reward, self.done

    # ------------------------------------------------------------ observations
    def obs_to_f32(self, packed: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Packed obs -> float32 [n][W][H] (the reference's np.float32 board)."""
        packed = self.obs if packed is None else packed
        out = torch.empty((self.n, self.width, self.height), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            C.check(self._L.st_obs_to_f32(self._ctx, _ptr(packed), _ptr(out), self._stream()))
        return out

    def grayscale(self, packed: Optional[torch.Tensor] = None, size: int = 84, channels: int = 1,
                  as_u8: bool = False) -> torch.Tensor:
        """convert_grayscale(board, size) [+ _rgb] per env: [n][size][size][channels]."""
        packed = self.obs if packed is None else packed
        out = torch.empty((self.n, size, size, channels),
                          dtype=torch.uint8 if as_u8 else torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            C.check(self._L.st_grayscale(self._ctx, _ptr(packed), size, channels, int(as_u8),
                                         _ptr(out), self._stream()))
        return out

    # ------------------------------------------------------------ state
    def _sizes(self):
        W, sd = self.width, self.stride
        return dict(board=(W, sd), piece=(sd,), stats=(C.NSTAT, sd), mt=(sd, int(self._views.mt_pitch)))

    def _view_ptr(self, name):
        return getattr(self._views, name)

    def _stat_ptr(self, row: int, env: int = 0) -> ctypes.c_void_p:
        """Device address of counter row `row` (C.STAT) of one env: the
        counters are int32 [NSTAT][stride]."""
        return ctypes.c_void_p(self._views.stats + (row * self.stride + env) * 4)

    def _pinned(self, shape, dtype) -> "_Pinned":
        return _Pinned(shape, dtype, self.device)

    def sync_mt(self):
        """Complete the generations the lazy in-kernel MT twist left in
        progress (st_mt_sync): afterwards stats/mt hold CPython's state."""
        if not hasattr(self._L, "st_mt_sync"):  # only an ST_LIB A/B build predating it
            return
        with torch.cuda.device(self.device):
            C.check(self._L.st_mt_sync(self._ctx, self._stream()))

    def state_tensors(self, fields=("board", "piece", "stats"), sync: bool = True) -> dict:
        """Device copies of the state (full stride; slice [..., :n] for real envs).
        `sync=False` skips st_mt_sync: the MT index row then carries engine
        bits (the counters are exact either way)."""
        out = {}
        if sync and ("stats" in fields or "mt" in fields):
            self.sync_mt()
        s = self._stream()
        for f in fields:  # st_copy runs on the stream's device: no device context needed
            shape = self._sizes()[f]
            t = torch.empty(shape, dtype=torch.int32, device=self.device)
            C.check(self._L.st_copy(_ptr(t), ctypes.c_void_p(self._view_ptr(f)), t.numel() * 4, s))
            out[f] = t
        return out

    def get_state(self, fields=("board", "piece", "stats", "mt")) -> dict:
        """Host (numpy, uint32/int32) copy of the state of the real envs."""
        t = self.state_tensors(fields)
        torch.cuda.synchronize(self.device)
        out = {}
        for f, v in t.items():
            a = v.cpu().numpy()
            if f in ("board", "piece", "mt"):
                a = a.view(np.uint32)
            out[f] = a[: self.n, : C.MT_N] if f == "mt" else a[..., : self.n]
        return out

    def set_state(self, **fields):
        """Upload state arrays for the real envs (shapes as returned by
        get_state); padding envs keep their current state."""
        cur = self.state_tensors(tuple(fields))
        # `piece` aliases stats row 14: upload it after `stats`
        order = sorted(fields, key=lambda f: ("stats", "board", "mt", "piece").index(f))
        with torch.cuda.device(self.device):
            for f in order:
                v = fields[f]
                full = cur[f].cpu().numpy().view(np.uint32).copy()
                v = np.asarray(v).astype(np.int64).astype(np.uint32)
                if f == "mt":
                    full[: self.n, : C.MT_N] = v
                else:
                    full[..., : self.n] = v
                t = torch.from_numpy(full.view(np.int32)).to(self.device)
                C.check(self._L.st_copy(ctypes.c_void_p(self._view_ptr(f)), _ptr(t),
                                        t.numel() * 4, self._stream()))
            torch.cuda.synchronize(self.device)

    def save(self, path: Optional[str] = None) -> bytes:
        """Snapshot of every env's state (st_save: board, piece, counters,
        shape counts, MT19937 state); written to `path` if given."""
        nbytes = int(self._L.st_state_bytes(self._ctx))
        buf = ctypes.create_string_buffer(nbytes)
        with torch.cuda.device(self.device):
            C.check(self._L.st_save(self._ctx, ctypes.cast(buf, ctypes.c_void_p), nbytes))
        data = buf.raw
        if path is not None:
            with open(path, "wb") as f:
                f.write(data)
        return data

    def load(self, snapshot) -> None:
        """Restore a snapshot from save() (bytes or a file path) into this
        batch (same width, height and env count)."""
        if isinstance(snapshot, (str, os.PathLike)):
            with open(snapshot, "rb") as f:
                snapshot = f.read()
        data = bytes(snapshot)
        with torch.cuda.device(self.device):
            C.check(self._L.st_load(self._ctx, data, len(data)))

    # ------------------------------------------------------------ fork
    def _fork_index(self, index):
        """fork()'s index as a contiguous int32 device tensor [n]: a torch
        tensor is checked (int32 [n] on the engine's device, never converted:
        the kernel reads it through its raw pointer), anything else _intake
        takes is converted from integers."""
        if index is None:
            return None
        index = self._intake(index, (self.n,), "index")
        if isinstance(index, torch.Tensor):
            _check_tensor(index, "index", (self.n,), (torch.int32,), self.device)
            return index
        if index.dtype.kind not in "iu":
            raise TypeError(f"index must be integers, got {index.dtype}")
        if index.shape != (self.n,):
            raise ValueError(f"index must have shape ({self.n},), got {index.shape}")
        # (an index past int32 is out of every source's range: it stays so)
        return torch.as_tensor(np.clip(index.astype(np.int64), -1, 2**31 - 1).astype(np.int32), device=self.device)

    def fork(self, src: Optional["TetrisBatch"] = None, index=None, mask=None, keep_rng: bool = False):
        """Copy env states on the device (st_fork): env e of this batch takes
        the state of env index[e] of `src` (None: this batch itself) where
        mask[e] is set -- the branching a rollout player, a beam search or a
        population restart needs.  index: int32 [n] (None: e); mask: bool /
        uint8 [n] (None: every env); device tensors, or host sequences.  An
        index outside [0, src.n) leaves its env exactly as it is; so does a
        cleared mask entry.  `src` may have another env count, lock_delay,
        scoring flags and autoreset mode (configuration, not state) but the
        same board size and device.
        keep_rng=False is copy.deepcopy of the reference's TetrisEngine with
        random.getstate(): board, piece, every counter row and the MT19937
        state, so the copy then does what its source would have done.
        keep_rng=True copies the engine without the random state: the env
        keeps its own MT19937 stream (as sync_mt() shows it), so copies of
        one game draw different piece futures.
        In place (src is this batch) the result is defined iff no env written
        with another env's state is itself the source of a written env --
        fork_groups() is that pattern.  Asynchronous on the current stream, no
        host read-back, no sync_mt() needed around it.  Returns the batch."""
        idx = self._fork_index(index)
        msk = self._need(mask)
        src = self if src is None else src
        if not isinstance(src, TetrisBatch):
            raise TypeError(f"src must be a TetrisBatch, got {type(src)}")
        if src.device != self.device:
            raise ValueError(f"src is on {src.device}, this batch on {self.device}")
        flags = C.FORK_KEEP_RNG if keep_rng else 0
        with torch.cuda.device(self.device):
            C.check(self._L.st_fork(self._ctx, src._ctx, _ptr(idx), _ptr(msk), flags, self._stream()))
        return self

    def fork_groups(self, group: int, keep_rng: bool = False):
        """"R roots x B branches in one batch", in place: every env e takes the
        state of its group's root (e // group) * group; the roots themselves
        are not written.  fork() with an index and a mask cached per group
        size."""
        if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or group < 1:
            raise ValueError(f"group must be an integer >= 1, got {group!r}")
        cache = self._fork_groups
        if group not in cache:
            e = torch.arange(self.n, dtype=torch.int32, device=self.device)
            root = e - e % int(group)
            cache[group] = (root, (root != e).to(torch.uint8))
        index, mask = cache[group]
        return self.fork(None, index=index, mask=mask, keep_rng=keep_rng)

    def render_packed(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """TetrisEngine.render() (tetris_env.py:317-321): board + current piece,
        packed u32 [W][n], without stepping."""
        out = torch.empty((self.width, self.n), dtype=torch.int32, device=self.device) \
            if out is None else out
        with torch.cuda.device(self.device):
            C.check(self._L.st_render(self._ctx, _ptr(out), self._stream()))
        return out

    def info_tensors(self, stats: Optional[torch.Tensor] = None) -> dict:
        """get_info() (tetris_env.py:232-241) for every env as int32 device
        tensors, from the live state or a `stats` snapshot of it."""
        if stats is None:
            stats = self.state_tensors(("stats",), sync=False)["stats"]
        st = stats[:, : self.n]
        return dict(time=st[C.STAT["time"]], score=st[C.STAT["score"]],
                    lines_cleared=st[C.STAT["lines"]], holes=st[C.STAT["holes"]],
                    deaths=st[C.STAT["deaths"]], piece_height=st[C.STAT["piece_height"]],
                    statistics=st[C.STAT["count0"]: C.STAT["count0"] + 7],
                    ep_time=st[C.STAT["ep_time"]], ep_score=st[C.STAT["ep_score"]],
                    ep_lines=st[C.STAT["ep_lines"]], ep_holes=st[C.STAT["ep_holes"]])

    def policy_greedy(self, t: int, seed: int = 0, explore: int = 30,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Greedy placement actions for the current states (st_policy_greedy):
        a clear-heavy workload generator for benchmarks and tests; `explore`
        per mille of the actions are uniform random (splitmix64 keyed by
        seed, t and the env index)."""
        out = self._act if out is None else out
        with torch.cuda.device(self.device):
            C.check(self._L.st_policy_greedy(self._ctx, ctypes.c_uint64(seed), int(t), int(explore),
                                             _ptr(out), self._stream()))
        return out

    def gen_actions(self, t: int, seed: int, global_offset: int = 0,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Synthetic uniform actions splitmix64(seed ^ ((t<<32) ^ e)) % 7 on device."""
        out = self._act if out is None else out
        with torch.cuda.device(self.device):
            C.check(self._L.st_gen_actions(_ptr(out), self.n, int(t), ctypes.c_uint64(seed),
                                           int(global_offset), self._stream()))
        return out

    # ------------------------------------------------------------ afterstates
    @property
    def n_slots(self) -> int:
        """Placement slots per env: 4 * (width + 6) (st_after_slots)."""
        return 4 * (self.width + 6)

    def slot(self, rot: int, x: int) -> int:
        return placement_slot(self.width, rot, x)

    def slot_rot_x(self, slot: int):
        return placement_rot_x(self.width, slot)

    def afterstates(self, boards: bool = True, out=None, features: str = "base") -> Afterstates:
        """Every placement of every env's current piece, in one launch
        (st_afterstates): slot s = slot(rot, x) is the piece in rotation rot
        at anchor (x, 0), valid iff not is_occupied there (tetris_env.py:29-36),
        hard-dropped (:54-59), set (:323-327) and the lines cleared (:205-216).
        Returns an Afterstates: feat int32 [n, AFTER_NFEAT, S], rows by name
        (.valid, .y, .lines, .holes, .height, .rows, .above, .dead, .reward,
        .agg_height, .bumpiness: _lib.AFTER), and with `boards` the resulting
        column words int32 [n, W, S] (else None); all zero for an invalid
        slot.  .reward is the reward of the step that locks the piece there,
        under this batch's scoring flags.  It is the idealised placement the
        greedy policy scores: no promise that moves, rotations and gravity can
        bring the live piece there.  Reads the state, changes none of it.
        `out`: a (feat, boards) pair of device tensors to write (boards None
        without `boards`).
        features='bcts' (st_afterstates_set) gives feat int32 [n, 18, S]: the
        eleven rows, then .landing2, .eroded, .row_trans, .col_trans, .wells,
        .hole_depth, .hole_rows (_lib.AFTER_EXT; simpletetris.h, "Feature
        sets") -- the rows of Dellacherie's and the BCTS players; the boards
        are the same."""
        n, W, S = self.n, self.width, self.n_slots
        fset, nrows, _ = _feature_set(features)
        if out is None:
            feat = torch.empty((n, nrows, S), dtype=torch.int32, device=self.device)
            brd = torch.empty((n, W, S), dtype=torch.int32, device=self.device) if boards else None
        else:
            feat, brd = out
            _check_tensor(feat, "out feat", (n, nrows, S), (torch.int32,), self.device)
            if boards:
                _check_tensor(brd, "out boards", (n, W, S), (torch.int32,), self.device)
            elif brd is not None:
                raise ValueError("out boards given with boards=False")
        if features == "base":
            C.check(self._L.st_afterstates(self._ctx, _ptr(feat), _ptr(brd), self._stream()))
        else:
            C.check(self._L.st_afterstates_set(self._ctx, fset, _ptr(feat), _ptr(brd), self._stream()))
        return Afterstates(feat, brd)

    def _slots(self, slots) -> torch.Tensor:
        """Placement slots as a contiguous int32 device tensor [n]: a device
        int32 tensor as it is, another integer tensor or a host sequence
        converted."""
        if isinstance(slots, torch.Tensor):
            if slots.is_floating_point() or slots.is_complex() or slots.dtype == torch.bool:
                raise TypeError(f"slots must be integers, got {slots.dtype}")
            s = slots.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            s = torch.as_tensor(np.asarray(slots).astype(np.int32), device=self.device)
        if tuple(s.shape) != (self.n,):
            raise ValueError(f"slots must have shape ({self.n},), got {tuple(s.shape)}")
        return s

    def placement_actions(self, slots, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The action (uint8 [n], as step() takes it) that moves each env's
        live piece toward its placement slot (st_placement_actions):
        rotate_left (4) until the rotation is the slot's, then right (1) /
        left (0) toward its column, then hard drop (2) -- the greedy
        policy's rule; a slot outside [0, n_slots) (e.g. -1: no valid
        placement) hard-drops.  slots: [n] integers, a device tensor (int32
        as it is) or a host sequence."""
        s = self._slots(slots)
        if out is None:
            if self._place_act is None:
                self._place_act = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            out = self._place_act
        else:
            _check_tensor(out, "out", (self.n,), (torch.uint8,), self.device)
        C.check(self._L.st_placement_actions(self._ctx, _ptr(s), _ptr(out), self._stream()))
        return out

    # ------------------------------------------------------------ reachability
    def reachable(self, first: bool = True, out=None) -> Reachable:
        """Which placement slots each env's live piece can really be locked in
        under the reference's step (st_reachable): a slot of afterstates() is
        reachable iff it is valid and some action sequence from the piece's
        present (rot, x, y, lock counter) -- each step the action, then
        gravity, then the lock rule (tetris_env.py:243-262) -- locks the piece
        at the slot's landing.  Returns a Reachable: steps int32 [n, S], the
        shortest such sequence's length (0: unreachable), with `first` the
        lowest-numbered action uint8 [n, S] that begins one (2: unreachable),
        and .mask = steps > 0.  first=False searches the distances alone,
        which is cheaper.  Reads the state, changes none of it; lock_delay
        above REACH_MAX_LOCK is refused.  `out`: a (steps, first) pair of
        device tensors to write (first None with first=False)."""
        n, S = self.n, self.n_slots
        if out is None:
            steps = torch.empty((n, S), dtype=torch.int32, device=self.device)
            fst = torch.empty((n, S), dtype=torch.uint8, device=self.device) if first else None
        else:
            steps, fst = out
            _check_tensor(steps, "out steps", (n, S), (torch.int32,), self.device)
            if first:
                _check_tensor(fst, "out first", (n, S), (torch.uint8,), self.device)
            elif fst is not None:
                raise ValueError("out first given with first=False")
        C.check(self._L.st_reachable(self._ctx, _ptr(steps), _ptr(fst), self._stream()))
        return Reachable(steps, fst)

    def route_actions(self, slots, out: Optional[torch.Tensor] = None,
                      steps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The action (uint8 [n], as step() takes it) that begins a shortest
        way of each env's live piece into its placement slot
        (st_route_actions): reachable()'s `first` of that slot; 2 (hard drop)
        for a slot outside [0, n_slots), invalid or unreachable.  Stepping
        with it and asking again locks the piece there after exactly
        reachable().steps steps.  slots: as placement_actions takes them;
        `steps`: an int32 [n] device tensor that receives the slot's steps
        (0 likewise)."""
        s = self._slots(slots)
        if out is None:
            if self._route_act is None:
                self._route_act = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            out = self._route_act
        else:
            _check_tensor(out, "out", (self.n,), (torch.uint8,), self.device)
        if steps is not None:
            _check_tensor(steps, "steps", (self.n,), (torch.int32,), self.device)
        C.check(self._L.st_route_actions(self._ctx, _ptr(s), _ptr(out), _ptr(steps), self._stream()))
        return out

    # ------------------------------------------------------------ routes
    def _need(self, need):
        if need is None:
            return None
        if isinstance(need, torch.Tensor) and need.dtype == torch.bool:
            need = need.to(torch.uint8)
        elif not isinstance(need, torch.Tensor):
            need = torch.as_tensor(np.asarray(need).astype(bool).astype(np.uint8), device=self.device)
        _check_tensor(need, "need", (self.n,), (torch.uint8,), self.device)
        return need

    def _routes_out(self, out):
        if out is None:
            return (torch.empty((C.ROUTE_WORDS, self.n), dtype=torch.int64, device=self.device),
                    torch.empty(self.n, dtype=torch.int32, device=self.device))
        route, steps = out
        _check_tensor(route, "out route", (C.ROUTE_WORDS, self.n), (torch.int64,), self.device)
        _check_tensor(steps, "out steps", (self.n,), (torch.int32,), self.device)
        return route, steps

    def routes(self, slots, need=None, out=None) -> Routes:
        """The whole shortest way of each env's live piece into its placement
        slot (st_routes): the actions route_actions() -> step(), repeated,
        would take, planned in one launch.  Returns a Routes -- .action(i) is
        the i-th step()'s action batch, .steps the length; the last action
        locks the piece in the slot.  A slot outside [0, n_slots), invalid or
        unreachable gives steps 0 and every field 7.  need: a bool / uint8 [n]
        mask; the envs it leaves out keep what `out` (a (route int64
        [ROUTE_WORDS, n], steps int32 [n]) pair; fresh, uninitialised tensors
        without it) held.  Reads the state, changes none of it."""
        s = self._slots(slots)
        nd = self._need(need)
        route, steps = self._routes_out(out)
        C.check(self._L.st_routes(self._ctx, _ptr(s), _ptr(nd), _ptr(route), _ptr(steps), self._stream()))
        return Routes(route, steps)

    def policy_routed(self, weights, features: str = "base", need=None, out=None) -> RoutedChoice:
        """reachable(first=False) -> policy_linear(weights, features=...,
        allowed=its steps) -> routes(its slots) in one launch
        (st_policy_routed): the best slot the live piece can really reach, and
        the whole route there.  Returns a RoutedChoice (slots, routes, scores);
        no reachable candidate: slot -1, steps 0, score 0, every field 7.
        need / out: as for routes(), out a (slots int32 [n], route, steps,
        scores float32 [n]) tuple."""
        fset = _feature_set(features)[0]
        w = self._weights(weights, features)
        nd = self._need(need)
        if out is None:
            sl = torch.empty(self.n, dtype=torch.int32, device=self.device)
            sc = torch.empty(self.n, dtype=torch.float32, device=self.device)
            route, steps = self._routes_out(None)
        else:
            sl, route, steps, sc = out
            _check_tensor(sl, "out slots", (self.n,), (torch.int32,), self.device)
            _check_tensor(sc, "out scores", (self.n,), (torch.float32,), self.device)
            route, steps = self._routes_out((route, steps))
        C.check(self._L.st_policy_routed(self._ctx, fset, _ptr(w), w.shape[0], _ptr(nd), _ptr(sl), _ptr(route),
                                         _ptr(steps), _ptr(sc), self._stream()))
        return RoutedChoice(sl, Routes(route, steps), sc)

    def play_routed(self, weights, k: int, features: str = "base", returns: Optional[torch.Tensor] = None,
                    episodes: Optional[torch.Tensor] = None, pieces: Optional[torch.Tensor] = None,
                    obs: str = "packed"):
        """k primitive steps of the honest feature player, enqueued by ONE
        library call (st_play_routed): an env without a plan takes
        policy_routed()'s slot and route, every env plays its route's next
        action through the ordinary step -- every placement is one the
        reference's own step can make.  Identical to that loop by hand; plans
        do not outlive the call, and play_routed(a) then play_routed(b) equals
        play_routed(a + b).  Adds rewards to `returns` (int64 [n]), dones to
        `episodes` (int32 [n]) and the pieces whose route was played to its
        last action to `pieces` (int32 [n]) -- continued, or fresh zeros -- and
        returns (returns, episodes, pieces).  The last step's outputs are in
        .reward, .done and (obs='packed') .obs.  Stream rule as play_linear."""
        if obs not in ("packed", "none"):
            raise ValueError("obs must be 'packed' or 'none'")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"k must be an integer >= 0, got {k!r}")
        fset = _feature_set(features)[0]
        w = self._weights(weights, features)
        acc = []
        for t, name, dt in ((returns, "returns", torch.int64), (episodes, "episodes", torch.int32),
                            (pieces, "pieces", torch.int32)):
            if t is None:
                t = torch.zeros(self.n, dtype=dt, device=self.device)
            else:
                _check_tensor(t, name, (self.n,), (dt,), self.device)
            acc.append(t)
        C.check(self._L.st_play_routed(self._ctx, fset, _ptr(w), w.shape[0], int(k), _ptr(acc[0]), _ptr(acc[1]),
                                       _ptr(acc[2]), _ptr(self.obs) if obs == "packed" else None, _ptr(self.reward),
                                       _ptr(self.done), self._stream()))
        return tuple(acc)

    # ------------------------------------------------------------ lock positions
    def lock_set(self, rows: bool = True, cap: Optional[int] = None, out=None) -> LockSet:
        """Every (rot, x, y) each env's live piece can be locked at under the
        reference's step, the tucks under overhangs that are no slot's landing
        included (st_lock_set).  Returns a LockSet: `rows` int32 [n, S], bit y
        of word (e, s) set iff the piece locks collision-free at row y of slot
        s (rows=False: None); with `cap`, `pos` int32 [n, cap], the positions
        lock_pos(rot, x, y) = slot * 32 + y in ascending order, -1 behind the
        last, a longer list cut; `count` int32 [n], the true count.  Reads the
        state, changes none of it; lock_delay above REACH_MAX_LOCK is refused.
        `out`: a (rows, pos, count) triple of device tensors to write (rows /
        pos None where not asked for)."""
        n, S = self.n, self.n_slots
        if cap is not None and (isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 1):
            raise ValueError(f"cap must be an integer >= 1, got {cap!r}")
        if out is None:
            rw = torch.empty((n, S), dtype=torch.int32, device=self.device) if rows else None
            ps = torch.empty((n, int(cap)), dtype=torch.int32, device=self.device) if cap is not None else None
            cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        else:
            rw, ps, cnt = out
            if rows:
                _check_tensor(rw, "out rows", (n, S), (torch.int32,), self.device)
            elif rw is not None:
                raise ValueError("out rows given with rows=False")
            if cap is not None:
                _check_tensor(ps, "out pos", (n, int(cap)), (torch.int32,), self.device)
            elif ps is not None:
                raise ValueError("out pos given without cap")
            _check_tensor(cnt, "out count", (n,), (torch.int32,), self.device)
        C.check(self._L.st_lock_set(self._ctx, _ptr(rw), _ptr(ps), int(cap) if cap is not None else 0, _ptr(cnt),
                                    self._stream()))
        return LockSet(rw, ps, cnt)

    def _positions(self, pos, shape, name="pos") -> torch.Tensor:
        """Lock positions as a contiguous int32 device tensor of `shape` (None:
        any extent): a device int32 tensor as it is, another integer tensor or
        a host array converted."""
        if isinstance(pos, torch.Tensor):
            if pos.is_floating_point() or pos.is_complex() or pos.dtype == torch.bool:
                raise TypeError(f"{name} must be integers, got {pos.dtype}")
            q = pos.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            q = torch.as_tensor(np.ascontiguousarray(np.asarray(pos).astype(np.int32)), device=self.device)
        if len(q.shape) != len(shape) or any(w is not None and w != g for w, g in zip(shape, q.shape)):
            raise ValueError(f"{name} must have shape {shape}, got {tuple(q.shape)}")
        return q

    def afterstates_at(self, pos, boards: bool = True, features: str = "base") -> Afterstates:
        """afterstates() at given lock positions (st_afterstates_at): pos int32
        [n, cap], any order and any values.  Entry (e, i) is evaluable iff it
        decodes to a slot and a row y < height, the piece is collision-free at
        (x, y) and occupied at (x, y + 1); its rows and board are those of
        afterstates(features=...) with the piece set at (x, y) in place of the
        hard drop from row 0 (.y = y).  Every row and the board of any other
        entry, -1 included, is 0.  Returns an Afterstates with feat int32
        [n, rows, cap] and boards int32 [n, W, cap] (or None).  Reads the state,
        changes none of it."""
        fset, nrows, _ = _feature_set(features)
        q = self._positions(pos, (self.n, None))
        cap = q.shape[1]
        if cap < 1:
            raise ValueError("pos: no entries")
        feat = torch.empty((self.n, nrows, cap), dtype=torch.int32, device=self.device)
        brd = torch.empty((self.n, self.width, cap), dtype=torch.int32, device=self.device) if boards else None
        C.check(self._L.st_afterstates_at(self._ctx, fset, _ptr(q), cap, _ptr(feat), _ptr(brd), self._stream()))
        return Afterstates(feat, brd)

    def routes_at(self, pos, need=None, out=None) -> Routes:
        """routes() with a lock position per env as the target (st_routes_at):
        the shortest action sequence that locks the live piece exactly at
        lock_rot_x_y(pos[e]).  A position that is -1, does not decode or is no
        lock position gives steps 0 and every field 7.  need / out: as for
        routes()."""
        q = self._positions(pos, (self.n,))
        nd = self._need(need)
        route, steps = self._routes_out(out)
        C.check(self._L.st_routes_at(self._ctx, _ptr(q), _ptr(nd), _ptr(route), _ptr(steps), self._stream()))
        return Routes(route, steps)

    def policy_locks(self, weights, features: str = "base", need=None, out=None) -> LockChoice:
        """lock_set() -> afterstates_at(its list) -> the linear score of
        policy_linear(weights, features=...) -> routes_at(the best) in one
        launch (st_policy_locks): the best place the live piece can really be
        locked at, tucks included, ties to the lowest position, and the whole
        route there.  Returns a LockChoice (pos, routes, scores, feat, count);
        no lock position: pos -1, steps 0, score 0, zero feat column, every
        field 7.  need: as for routes(); out: a (pos int32 [n], route, steps,
        scores float32 [n], feat int32 [rows, n], count int32 [n]) tuple."""
        fset, nrows, _ = _feature_set(features)
        w = self._weights(weights, features)
        nd = self._need(need)
        if out is None:
            ps = torch.empty(self.n, dtype=torch.int32, device=self.device)
            sc = torch.empty(self.n, dtype=torch.float32, device=self.device)
            ft = torch.empty((nrows, self.n), dtype=torch.int32, device=self.device)
            cnt = torch.empty(self.n, dtype=torch.int32, device=self.device)
            route, steps = self._routes_out(None)
        else:
            ps, route, steps, sc, ft, cnt = out
            _check_tensor(ps, "out pos", (self.n,), (torch.int32,), self.device)
            _check_tensor(sc, "out scores", (self.n,), (torch.float32,), self.device)
            _check_tensor(ft, "out feat", (nrows, self.n), (torch.int32,), self.device)
            _check_tensor(cnt, "out count", (self.n,), (torch.int32,), self.device)
            route, steps = self._routes_out((route, steps))
        C.check(self._L.st_policy_locks(self._ctx, fset, _ptr(w), w.shape[0], _ptr(nd), _ptr(ps), _ptr(route),
                                        _ptr(steps), _ptr(sc), _ptr(ft), _ptr(cnt), self._stream()))
        return LockChoice(ps, Routes(route, steps), sc, ft, cnt)

    def play_locks(self, weights, k: int, features: str = "base", returns: Optional[torch.Tensor] = None,
                   episodes: Optional[torch.Tensor] = None, pieces: Optional[torch.Tensor] = None,
                   obs: str = "packed"):
        """play_routed() with policy_locks() as the planner (st_play_locks): k
        primitive steps of the feature player over every lock position, tucks
        under overhangs included, enqueued by ONE library call.  Identical to
        the loop by hand; plans do not outlive the call, and play_locks(a)
        then play_locks(b) equals play_locks(a + b).  returns / episodes /
        pieces, the result and the stream rule are play_routed's."""
        if obs not in ("packed", "none"):
            raise ValueError("obs must be 'packed' or 'none'")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"k must be an integer >= 0, got {k!r}")
        fset = _feature_set(features)[0]
        w = self._weights(weights, features)
        acc = []
        for t, name, dt in ((returns, "returns", torch.int64), (episodes, "episodes", torch.int32),
                            (pieces, "pieces", torch.int32)):
            if t is None:
                t = torch.zeros(self.n, dtype=dt, device=self.device)
            else:
                _check_tensor(t, name, (self.n,), (dt,), self.device)
            acc.append(t)
        C.check(self._L.st_play_locks(self._ctx, fset, _ptr(w), w.shape[0], int(k), _ptr(acc[0]), _ptr(acc[1]),
                                      _ptr(acc[2]), _ptr(self.obs) if obs == "packed" else None, _ptr(self.reward),
                                      _ptr(self.done), self._stream()))
        return tuple(acc)

    # ------------------------------------------------------------ placement step
    def _placed_out(self, out) -> torch.Tensor:
        if out is None:
            if self.placed is None:
                self.placed = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
            return self.placed
        _check_tensor(out, "out placed", (self.n,), (torch.uint8,), self.device)
        return out

    def place(self, slots, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Commit a placement slot per env (st_place), without stepping.  A
        valid slot -- in [0, n_slots) and, as in afterstates(), not occupied
        at (x, 0) on the env's board for its current piece -- teleports the
        env's piece there: rotation rot, anchor (x, 0) and a lock counter of
        max(lock_delay, 0), so that the next hard drop locks it whatever
        lock_delay is.  Any other slot (occupied, out of range, -1) leaves
        the piece exactly as it is.  Board, counters and MT are not touched.
        slots: [n] integers as placement_actions takes them.  Returns `placed`
        uint8 [n] (1: committed) -- a reused buffer, or the caller's `out`."""
        s = self._slots(slots)
        placed = self._placed_out(out)
        C.check(self._L.st_place(self._ctx, _ptr(s), _ptr(placed), self._stream()))
        return placed

    def step_placements(self, slots, obs: str = "packed", out=None):
        """One placement step on every env (st_step_placements): place(slots),
        then TetrisEngine.step(hard_drop) -- one decision is one piece.  Where
        the slot is valid the piece locks in this step, the reward is the
        slot's afterstates().reward and the board becomes its afterstate
        (before a death's erase or same-step reset), and the next piece is
        drawn; where it is not, the live piece hard-drops as it is.  Returns
        what step() returns -- (obs, reward, done), obs 'packed' or 'none',
        `out` as for step() -- and leaves the uint8 [n] commit flags in
        .placed.  Never raises for actions (they are the library's own)."""
        if obs not in ("packed", "none"):
            raise ValueError("obs must be 'packed' or 'none'")
        s = self._slots(slots)
        o_t, r_t, d_t = (self.obs, self.reward, self.done) if out is None \
            else _check_out(out, self.width, self.n, self.device)
        placed = self._placed_out(None)
        o_ret = o_t if obs == "packed" else None
        C.check(self._L.st_step_placements(self._ctx, _ptr(s), _ptr(placed), _ptr(o_ret), _ptr(r_t), _ptr(d_t),
                                           self._stream()))
        return o_ret, r_t, d_t

    # ------------------------------------------------------------ linear feature players
    def _weights(self, weights, features: str = "base") -> torch.Tensor:
        """policy_linear's / play_linear's weights as a float32 device tensor
        [n_w, rows] (rows = AFTER_NFEAT, features='bcts': 18): a device tensor
        [rows] or [n_w, rows] as it is (checked, never converted), anything
        else through weight_rows."""
        nrows = _feature_set(features)[1]
        if isinstance(weights, torch.Tensor):
            w = weights[None] if weights.dim() == 1 else weights
            _check_tensor(w, "weights", (None, nrows), (torch.float32,), self.device)
            if w.shape[0] < 1:
                raise ValueError("weights: no rows")
            return w
        return torch.as_tensor(weight_rows(weights, features), device=self.device)

    def policy_linear(self, weights, out=None, features: str = "base", allowed=None) -> LinearChoice:
        """Every env's best placement under linear feature weights, in one
        launch (st_policy_linear).  Env e scores every placement slot of its
        current piece -- afterstates()'s slots and feature rows -- with weight
        row e % n_w: float32 acc = acc + w[r] * feat[r] over the rows in
        _lib.AFTER order from 0, each product and sum rounded on its own; the
        valid slot with the largest score wins, ties to the lowest slot.
        weights: a float32 device tensor [AFTER_NFEAT] or [n_w, AFTER_NFEAT]
        (one row per candidate of a population), a host sequence of that
        shape, or a dict by feature name (GREEDY_WEIGHTS; missing names are 0;
        'valid' is a bias).  Returns a LinearChoice: .slots (-1 where no slot
        is valid: then action 2, score 0, feature column 0), .actions (what
        placement_actions gives for the slot), .scores, .feat [AFTER_NFEAT, n]
        and its rows by name.  Reads the state, changes none of it.
        `out`: a (slots, actions, scores, feat) tuple of device tensors to
        write; None entries are not computed (at least one must be given).
        features='bcts' (st_policy_linear_set) scores the 18 rows of
        afterstates(features='bcts') -- weights [18] / [n_w, 18] or a dict by
        _lib.AFTER_BCTS name (DELLACHERIE_WEIGHTS, BCTS_WEIGHTS), .feat [18, n].
        allowed: a slot mask, a Reachable (its .steps) or an int32 [n, S] device
        tensor: only valid slots whose entry is not 0 are candidates -- with
        reachable() the player is confined to the slots the live piece can
        really reach; where none is left: slot -1, action 2, score 0."""
        n = self.n
        fset, nrows, _ = _feature_set(features)
        w = self._weights(weights, features)
        if isinstance(allowed, Reachable):
            allowed = allowed.steps
        if allowed is not None:
            _check_tensor(allowed, "allowed", (n, self.n_slots), (torch.int32,), self.device)
        if out is None:
            out = (torch.empty(n, dtype=torch.int32, device=self.device),
                   torch.empty(n, dtype=torch.uint8, device=self.device),
                   torch.empty(n, dtype=torch.float32, device=self.device),
                   torch.empty((nrows, n), dtype=torch.int32, device=self.device))
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 4:
                raise ValueError("out: a (slots, actions, scores, feat) tuple, None for an output not wanted")
            if all(t is None for t in out):
                raise ValueError("out: at least one output tensor is needed")
            for t, name, shape, dt in zip(out, ("slots", "actions", "scores", "feat"),
                                          ((n,), (n,), (n,), (nrows, n)),
                                          (torch.int32, torch.uint8, torch.float32, torch.int32)):
                if t is not None:
                    _check_tensor(t, "out " + name, shape, (dt,), self.device)
        sl, ac, sc, ft = out
        if features == "base" and allowed is None:
            C.check(self._L.st_policy_linear(self._ctx, _ptr(w), w.shape[0], _ptr(sl), _ptr(ac), _ptr(sc), _ptr(ft),
                                             self._stream()))
        else:
            C.check(self._L.st_policy_linear_set(self._ctx, fset, _ptr(w), w.shape[0], _ptr(allowed), _ptr(sl),
                                                 _ptr(ac), _ptr(sc), _ptr(ft), self._stream()))
        return LinearChoice(sl, ac, sc, ft)

    def play_linear(self, weights, k: int, returns: Optional[torch.Tensor] = None,
                    episodes: Optional[torch.Tensor] = None, obs: str = "none", placements: bool = False,
                    features: str = "base"):
        """k steps of policy_linear(weights) -> step, enqueued by ONE library
        call (st_play_linear: no Python, no host read-back between the steps),
        identical to k rounds of policy_linear + step by hand.  Adds every
        step's reward to `returns` (int64 [n]) and every step's done to
        `episodes` (int32 [n]) -- device tensors that are continued where the
        caller left them, or fresh zeros -- and returns (returns, episodes).
        With one weight row per candidate and autoreset='same_step' that is a
        CEM / ES generation in one call and one read-back; under
        autoreset='none' a dead env keeps being stepped in the state the
        reference leaves, as the loop by hand would.  The last step's outputs
        are in .reward, .done and (obs='packed') .obs.  Not gated, never
        raises for actions (the policy's are 0..6); k = 0 does nothing.  The
        library keeps the actions and the rows it sums in one buffer per
        batch: keep a batch's play_linear calls on one stream.
        placements=True plays at placement level (st_play_linear_placements):
        k rounds of policy_linear -> step_placements(its slots), the policy's
        launch committing its own choice -- every iteration locks a piece
        (where a slot is valid) and pays exactly the afterstate reward the
        policy maximised; two launches per piece.
        features='bcts' (st_play_linear_set) plays with the 18 rows of
        policy_linear(features='bcts'), at either level."""
        if obs not in ("packed", "none"):
            raise ValueError("obs must be 'packed' or 'none'")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"k must be an integer >= 0, got {k!r}")
        fset = _feature_set(features)[0]
        w = self._weights(weights, features)
        if returns is None:
            returns = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        else:
            _check_tensor(returns, "returns", (self.n,), (torch.int64,), self.device)
        if episodes is None:
            episodes = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        else:
            _check_tensor(episodes, "episodes", (self.n,), (torch.int32,), self.device)
        tail = (_ptr(returns), _ptr(episodes), _ptr(self.obs) if obs == "packed" else None, _ptr(self.reward),
                _ptr(self.done), self._stream())
        if features == "base":
            fn = self._L.st_play_linear_placements if placements else self._L.st_play_linear
            C.check(fn(self._ctx, _ptr(w), w.shape[0], int(k), *tail))
        else:
            C.check(self._L.st_play_linear_set(self._ctx, fset, _ptr(w), w.shape[0], int(k), int(bool(placements)),
                                               *tail))
        return returns, episodes

    # ------------------------------------------------------------ next piece, two-ply player
    def next_piece(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The piece every env's next spawn takes (st_next_piece): uint8 [n],
        the id in SHAPE_NAMES order of the shape _choose_shape()
        (tetris_env.py:183-191) would return for the env now -- the piece
        behind the next lock, or behind a reset.  Changes nothing the
        reference can see: board, piece, counters and the MT19937 state as
        sync_mt() / save() give it stay the same, and so does every later
        step.  `out`: a uint8 [n] device tensor to write."""
        if out is None:
            out = torch.empty(self.n, dtype=torch.uint8, device=self.device)
        else:
            _check_tensor(out, "out", (self.n,), (torch.uint8,), self.device)
        C.check(self._L.st_next_piece(self._ctx, _ptr(out), self._stream()))
        return out

    def _lookahead_weights(self, weights, first_weights, features):
        w2 = self._weights(weights, features)
        w1 = None
        if first_weights is not None:
            w1 = self._weights(first_weights, features)
            if w1.shape != w2.shape:
                raise ValueError(f"first_weights: shape {tuple(w1.shape)} is not weights' {tuple(w2.shape)}")
        return w1, w2

    def policy_lookahead(self, weights, first_weights=None, dead_value: float = -1.0e6, features: str = "base",
                         allowed=None, table: bool = False, out=None) -> LookaheadChoice:
        """policy_linear with the next piece known, in one launch
        (st_policy_lookahead).  Every candidate slot s1 of the current piece
        (valid, and allowed where `allowed` is given: policy_linear's mask) that
        does not end the game is followed by every placement s2 of
        next_piece() on its afterstate board, with the counters the lock of s1
        leaves; score(s1) = S1 + T in float32, S1 the chain score of s1's rows
        under `first_weights` (0 if None), T the largest chain score over the
        valid s2 under `weights` (ties to the lowest s2), or `dead_value` where
        s1 is dead or leaves no valid s2.  The candidate with the largest score
        wins, ties to the lowest slot.  weights / first_weights: as
        policy_linear takes them, both of one shape; row e % n_w is env e's.
        Returns a LookaheadChoice: .slots (-1: no candidate, then slots2 -1,
        action 2, score 0), .slots2, .actions, .scores, and with table=True
        .scores_all float32 [n, S] / .slots2_all int32 [n, S] for every
        candidate (0 / -1 elsewhere).  Changes nothing the reference can see
        (next_piece's rule).  `out`: a (slots, slots2, actions, scores) tuple
        -- with table=True (slots, slots2, actions, scores, scores_all,
        slots2_all) -- of device tensors to write; None entries are not
        computed (at least one must be given)."""
        n, S = self.n, self.n_slots
        fset = _feature_set(features)[0]
        w1, w2 = self._lookahead_weights(weights, first_weights, features)
        dv = _dead_value(dead_value)
        if isinstance(allowed, Reachable):
            allowed = allowed.steps
        if allowed is not None:
            _check_tensor(allowed, "allowed", (n, S), (torch.int32,), self.device)
        names = ("slots", "slots2", "actions", "scores", "scores_all", "slots2_all")[: 6 if table else 4]
        shapes = ((n,), (n,), (n,), (n,), (n, S), (n, S))
        dtypes = (torch.int32, torch.int32, torch.uint8, torch.float32, torch.float32, torch.int32)
        if out is None:
            out = tuple(torch.empty(sh, dtype=dt, device=self.device) for _, sh, dt in zip(names, shapes, dtypes))
        else:
            if not isinstance(out, (tuple, list)) or len(out) != len(names):
                raise ValueError(f"out: a ({', '.join(names)}) tuple, None for an output not wanted")
            if all(t is None for t in out):
                raise ValueError("out: at least one output tensor is needed")
            for t, name, sh, dt in zip(out, names, shapes, dtypes):
                if t is not None:
                    _check_tensor(t, "out " + name, sh, (dt,), self.device)
        out = tuple(out) + (None,) * (6 - len(out))
        C.check(self._L.st_policy_lookahead(self._ctx, fset, _ptr(w1), _ptr(w2), w2.shape[0], dv, _ptr(allowed),
                                            *(_ptr(t) for t in out), self._stream()))
        return LookaheadChoice(*out)

    def play_lookahead(self, weights, k: int, first_weights=None, dead_value: float = -1.0e6,
                       features: str = "base", returns: Optional[torch.Tensor] = None,
                       episodes: Optional[torch.Tensor] = None, obs: str = "packed", out=None):
        """k pieces of policy_lookahead(weights, first_weights, dead_value) ->
        step_placements(its slots), enqueued by ONE library call
        (st_play_lookahead), identical to the k rounds by hand: placement-level
        play_linear with the two-ply choice.  `returns` / `episodes`, both
        autoreset modes, k = 0 and the one-stream rule are play_linear's;
        returns (returns, episodes).  The last step's outputs are in .reward,
        .done and (obs='packed') .obs, or in `out`, an (obs, reward, done)
        triple as step() takes it."""
        if obs not in ("packed", "none"):
            raise ValueError("obs must be 'packed' or 'none'")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"k must be an integer >= 0, got {k!r}")
        fset = _feature_set(features)[0]
        w1, w2 = self._lookahead_weights(weights, first_weights, features)
        dv = _dead_value(dead_value)
        if returns is None:
            returns = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        else:
            _check_tensor(returns, "returns", (self.n,), (torch.int64,), self.device)
        if episodes is None:
            episodes = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        else:
            _check_tensor(episodes, "episodes", (self.n,), (torch.int32,), self.device)
        o_t, r_t, d_t = (self.obs, self.reward, self.done) if out is None \
            else _check_out(out, self.width, self.n, self.device)
        C.check(self._L.st_play_lookahead(self._ctx, fset, _ptr(w1), _ptr(w2), w2.shape[0], dv, int(k),
                                          _ptr(returns), _ptr(episodes), _ptr(o_t) if obs == "packed" else None,
                                          _ptr(r_t), _ptr(d_t), self._stream()))
        return returns, episodes

    # ------------------------------------------------------------ next-piece odds, expectimax player
    def next_weights(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The odds of the piece every env's next spawn takes
        (st_next_weights): int32 [7, n], row i = 5 + max(counts) - counts[i]
        over the env's shape counters -- m of _choose_shape()
        (tetris_env.py:186), which picks shape i (SHAPE_NAMES order) with
        probability m[i] / m.sum(0).  Unlike next_piece() this is what an agent
        may know: the counters are info['statistics'] of every step.  Reads the
        counters only and changes nothing.  `out`: an int32 [7, n] device
        tensor to write."""
        if out is None:
            out = torch.empty((7, self.n), dtype=torch.int32, device=self.device)
        else:
            _check_tensor(out, "out", (7, self.n), (torch.int32,), self.device)
        C.check(self._L.st_next_weights(self._ctx, _ptr(out), self._stream()))
        return out

    def policy_expect(self, weights, first_weights=None, dead_value: float = -1.0e6, features: str = "base",
                      allowed=None, table: bool = False, out=None) -> ExpectChoice:
        """policy_lookahead over the odds of the next piece instead of the
        piece itself, in one launch (st_policy_expect): the two-ply player the
        reference's rules allow, since it never reads the env's random state.
        First ply, candidates, `allowed`, weights / first_weights, S1 and
        dead_value are policy_lookahead's.  For a candidate s1 and every piece
        q, T_q is the largest chain score over the valid placements of q on
        s1's afterstate (ties to the lowest), or `dead_value` where s1 is dead
        or q has no valid placement; with m = next_weights() of the env,
        score(s1) = S1 + (sum_q float32(m[q]) * T_q) / float32(sum(m)), every
        float32 operation rounded on its own, q in order 0..6.  The candidate
        with the largest score wins, ties to the lowest slot.
        Returns an ExpectChoice: .slots (-1: no candidate, then action 2, score
        0), .actions, .scores, and with table=True .scores_all float32 [n, S],
        .tails float32 [n, 7, S] and .slots2_all int32 [n, 7, S].  Changes
        nothing, the engine's private preview included.  `out`: a (slots,
        actions, scores) tuple -- with table=True (slots, actions, scores,
        scores_all, tails, slots2_all) -- of device tensors to write; None
        entries are not computed (at least one must be given)."""
        n, S = self.n, self.n_slots
        fset = _feature_set(features)[0]
        w1, w2 = self._lookahead_weights(weights, first_weights, features)
        dv = _dead_value(dead_value)
        if isinstance(allowed, Reachable):
            allowed = allowed.steps
        if allowed is not None:
            _check_tensor(allowed, "allowed", (n, S), (torch.int32,), self.device)
        names = ("slots", "actions", "scores", "scores_all", "tails", "slots2_all")[: 6 if table else 3]
        shapes = ((n,), (n,), (n,), (n, S), (n, 7, S), (n, 7, S))
        dtypes = (torch.int32, torch.uint8, torch.float32, torch.float32, torch.float32, torch.int32)
        if out is None:
            out = tuple(torch.empty(sh, dtype=dt, device=self.device) for _, sh, dt in zip(names, shapes, dtypes))
        else:
            if not isinstance(out, (tuple, list)) or len(out) != len(names):
                raise ValueError(f"out: a ({', '.join(names)}) tuple, None for an output not wanted")
            if all(t is None for t in out):
                raise ValueError("out: at least one output tensor is needed")
            for t, name, sh, dt in zip(out, names, shapes, dtypes):
                if t is not None:
                    _check_tensor(t, "out " + name, sh, (dt,), self.device)
        out = tuple(out) + (None,) * (6 - len(out))
        C.check(self._L.st_policy_expect(self._ctx, fset, _ptr(w1), _ptr(w2), w2.shape[0], dv, _ptr(allowed),
                                         *(_ptr(t) for t in out), self._stream()))
        return ExpectChoice(*out)

    def play_expect(self, weights, k: int, first_weights=None, dead_value: float = -1.0e6,
                    features: str = "base", returns: Optional[torch.Tensor] = None,
                    episodes: Optional[torch.Tensor] = None, obs: str = "packed", out=None):
        """k pieces of policy_expect(weights, first_weights, dead_value) ->
        step_placements(its slots), enqueued by ONE library call
        (st_play_expect), identical to the k rounds by hand: play_lookahead
        with the expectimax choice.  Every argument and the return value are
        play_lookahead's."""
        if obs not in ("packed", "none"):
            raise ValueError("obs must be 'packed' or 'none'")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"k must be an integer >= 0, got {k!r}")
        fset = _feature_set(features)[0]
        w1, w2 = self._lookahead_weights(weights, first_weights, features)
        dv = _dead_value(dead_value)
        if returns is None:
            returns = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        else:
            _check_tensor(returns, "returns", (self.n,), (torch.int64,), self.device)
        if episodes is None:
            episodes = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        else:
            _check_tensor(episodes, "episodes", (self.n,), (torch.int32,), self.device)
        o_t, r_t, d_t = (self.obs, self.reward, self.done) if out is None \
            else _check_out(out, self.width, self.n, self.device)
        C.check(self._L.st_play_expect(self._ctx, fset, _ptr(w1), _ptr(w2), w2.shape[0], dv, int(k),
                                       _ptr(returns), _ptr(episodes), _ptr(o_t) if obs == "packed" else None,
                                       _ptr(r_t), _ptr(d_t), self._stream()))
        return returns, episodes

    # ------------------------------------------------------------ n-tuple network
    def set_ntuple(self, net) -> None:
        """Give the batch its n-tuple network (st_ntuple_set): an
        ntuple.NTupleNet of the batch's board size, or None to remove it.  The
        library validates the tuples again and keeps a device copy of its own;
        a later call replaces it.  Synchronous."""
        if net is None:
            C.check(self._L.st_ntuple_set(self._ctx, None, 0))
            self._ntuple = None
            return
        if (net.width, net.height) != (self.width, self.height):
            raise ValueError(f"net: a {net.width}x{net.height} network on a {self.width}x{self.height} batch")
        t = np.ascontiguousarray(net.tuples, np.int32)
        C.check(self._L.st_ntuple_set(self._ctx, t.ctypes.data_as(ctypes.c_void_p), len(t)))
        assert self._L.st_ntuple_table_len(self._ctx) == net.table_len
        self._ntuple = net

    def _ntuple_table(self, table) -> torch.Tensor:
        """The host layer's check of a table: a contiguous float32 tensor on
        the batch's device with at least table_len entries."""
        net = getattr(self, "_ntuple", None)
        if net is None:
            raise RuntimeError("no n-tuple network: call set_ntuple(net) first")
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.device != self.device \
                or not table.is_contiguous():
            raise ValueError(f"table: a contiguous float32 tensor on {self.device} is needed")
        if table.numel() < net.table_len:
            raise ValueError(f"table: {table.numel()} entries, the network needs {net.table_len}")
        return table

    def ntuple_eval(self, table, boards: Optional[torch.Tensor] = None, index: bool = False, out=None):
        """The network's value of boards (st_ntuple_eval): float32 sum of the
        T table entries in tuple order.  boards: None for the batch's own
        boards (values [n]), or a contiguous int32 device tensor [W, ...] of
        packed column words (the obs layout; afterstates().boards permuted
        to [W, n, S]) -- values take the shape behind W.  With index=True
        returns (values, index), index int32 [T, ...]: the entries read.
        `out`: a (values, index) pair of device tensors to write, None for the
        one not wanted; the pair is returned."""
        table = self._ntuple_table(table)
        T = len(self._ntuple)
        if boards is None:
            rest, m = (self.n,), self.n
        else:
            if not isinstance(boards, torch.Tensor) or boards.dtype != torch.int32 or boards.device != self.device \
                    or boards.dim() < 2 or boards.shape[0] != self.width or not boards.is_contiguous():
                raise ValueError(f"boards: a contiguous int32 [{self.width}, ...] tensor on {self.device} is needed")
            rest = tuple(boards.shape[1:])
            m = int(np.prod(rest))
        if out is None:
            values = torch.empty(rest, dtype=torch.float32, device=self.device)
            idx = torch.empty((T,) + rest, dtype=torch.int32, device=self.device) if index else None
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 2 or (out[0] is None and out[1] is None):
                raise ValueError("out: a (values, index) pair, None for an output not wanted (not both)")
            values, idx = out
            if values is not None:
                _check_tensor(values, "out values", rest, (torch.float32,), self.device)
            if idx is not None:
                _check_tensor(idx, "out index", (T,) + rest, (torch.int32,), self.device)
        C.check(self._L.st_ntuple_eval(self._ctx, _ptr(table), _ptr(boards), m, _ptr(values), _ptr(idx),
                                       self._stream()))
        return (values, idx) if index or out is not None else values

    def policy_ntuple(self, table, weights=None, dead_value: float = 0.0, features: str = "base", allowed=None,
                      index: bool = False, values_all: bool = False, out=None) -> NTupleChoice:
        """policy_linear with the n-tuple network behind it, in one launch
        (st_policy_ntuple).  Every candidate slot of the current piece (valid,
        and allowed where `allowed` is given: policy_linear's mask) scores
        S1 + V in float32: S1 the chain score of its rows under `weights` (as
        policy_linear takes them; None: 0), V the network's value of its
        afterstate board (afterstates().boards) read from `table`, or
        `dead_value` where the placement ends the game.  The candidate with
        the largest score wins, ties to the lowest slot.  With the 'reward'
        weight 1 and every other 0 that is the TD afterstate rule
        argmax r + V(s').  Returns an NTupleChoice: .slots (-1: no candidate,
        then action 2, score 0, value 0), .actions, .scores, .feat, .values,
        and .index (index=True) / .values_all (values_all=True).  Reads the
        state, changes none of it.  `out`: a (slots, actions, scores, feat,
        values) tuple, with index / values_all tensors behind it where those
        are asked for; None entries are not computed (at least one is needed)."""
        n, S = self.n, self.n_slots
        table = self._ntuple_table(table)
        T = len(self._ntuple)
        fset, nrows, _ = _feature_set(features)
        w = None if weights is None else self._weights(weights, features)
        dv = _dead_value(dead_value)
        if isinstance(allowed, Reachable):
            allowed = allowed.steps
        if allowed is not None:
            _check_tensor(allowed, "allowed", (n, S), (torch.int32,), self.device)
        spec = [("slots", (n,), torch.int32), ("actions", (n,), torch.uint8), ("scores", (n,), torch.float32),
                ("feat", (nrows, n), torch.int32), ("values", (n,), torch.float32)]
        if index:
            spec.append(("index", (T, n), torch.int32))
        if values_all:
            spec.append(("values_all", (n, S), torch.float32))
        if out is None:
            out = tuple(torch.empty(sh, dtype=dt, device=self.device) for _, sh, dt in spec)
        else:
            if not isinstance(out, (tuple, list)) or len(out) != len(spec):
                raise ValueError(f"out: a ({', '.join(s[0] for s in spec)}) tuple, None for an output not wanted")
            if all(t is None for t in out):
                raise ValueError("out: at least one output tensor is needed")
            for t, (name, sh, dt) in zip(out, spec):
                if t is not None:
                    _check_tensor(t, "out " + name, sh, (dt,), self.device)
        got = dict(zip((s[0] for s in spec), out))
        C.check(self._L.st_policy_ntuple(self._ctx, fset, _ptr(w), 0 if w is None else w.shape[0], _ptr(table), dv,
                                         _ptr(allowed), _ptr(got["slots"]), _ptr(got["actions"]), _ptr(got["scores"]),
                                         _ptr(got["values"]), _ptr(got["feat"]), _ptr(got.get("index")),
                                         _ptr(got.get("values_all")), self._stream()))
        return NTupleChoice(got["slots"], got["actions"], got["scores"], got["feat"], got["values"], got.get("index"),
                            got.get("values_all"))

    def play_ntuple(self, table, k: int, weights=None, dead_value: float = 0.0, features: str = "base",
                    returns: Optional[torch.Tensor] = None, episodes: Optional[torch.Tensor] = None,
                    obs: str = "packed", out=None):
        """k pieces of policy_ntuple(table, weights, dead_value) ->
        step_placements(its slots), enqueued by ONE library call
        (st_play_ntuple), identical to the k rounds by hand: play_lookahead
        with the network's choice.  `returns` / `episodes`, both autoreset
        modes, k = 0, obs, `out` and the return value are play_lookahead's."""
        if obs not in ("packed", "none"):
            raise ValueError("obs must be 'packed' or 'none'")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0:
            raise ValueError(f"k must be an integer >= 0, got {k!r}")
        table = self._ntuple_table(table)
        fset = _feature_set(features)[0]
        w = None if weights is None else self._weights(weights, features)
        dv = _dead_value(dead_value)
        if returns is None:
            returns = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        else:
            _check_tensor(returns, "returns", (self.n,), (torch.int64,), self.device)
        if episodes is None:
            episodes = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        else:
            _check_tensor(episodes, "episodes", (self.n,), (torch.int32,), self.device)
        o_t, r_t, d_t = (self.obs, self.reward, self.done) if out is None \
            else _check_out(out, self.width, self.n, self.device)
        C.check(self._L.st_play_ntuple(self._ctx, fset, _ptr(w), 0 if w is None else w.shape[0], _ptr(table), dv,
                                       int(k), _ptr(returns), _ptr(episodes), _ptr(o_t) if obs == "packed" else None,
                                       _ptr(r_t), _ptr(d_t), self._stream()))
        return returns, episodes


def unwire(wire: torch.Tensor, width: int, height: int):
    """st_unwire: gathered wire rows int32 [words, n] (st_step_wire, one
    shard's or several shards' concatenated along n) on a GPU -> (packed obs
    int32 [width, n], reward int32 [n], done bool [n]), bit-exact with
    step()'s outputs.  Runs on the tensor's device, on torch's current stream."""
    L = C.load()
    words = C.check_count(L.st_wire_words(width, height))
    _check_tensor(wire, "wire", (words, None), (torch.int32,))
    n = wire.shape[1]
    obs = torch.empty((width, n), dtype=torch.int32, device=wire.device)
    reward = torch.empty(n, dtype=torch.int32, device=wire.device)
    done = torch.empty(n, dtype=torch.bool, device=wire.device)
    with torch.cuda.device(wire.device):
        C.check(L.st_unwire(width, height, n, _ptr(wire), _ptr(obs), _ptr(reward), _ptr(done),
                            _stream_ptr(wire.device)))
    return obs, reward, done


def unwire_shards(recv: torch.Tensor, width: int, height: int, n_global: int, out=None):
    """st_unwire_shards: a gather's receive buffer int32 [shards, words,
    n_cap] on a GPU (shard r = the contiguous block shard_range(n_global,
    shards, r), its envs at columns 0 .. count_r - 1) -> (packed obs int32
    [width, n_global], reward int32 [n_global], done bool [n_global]) in
    global env order, bit-exact with step()'s outputs, without assembling the
    shards first.  `out`: optional (obs, reward, done) tensors to write.
    Runs on the tensor's device, on torch's current stream."""
    L = C.load()
    words = C.check_count(L.st_wire_words(width, height))
    _check_tensor(recv, "recv", (None, words, None), (torch.int32,))  # [shards, words, n_cap]
    shards, _, cap = recv.shape
    if out is None:
        obs, reward, done = (torch.empty((width, n_global), dtype=torch.int32, device=recv.device),
                             torch.empty(n_global, dtype=torch.int32, device=recv.device),
                             torch.empty(n_global, dtype=torch.bool, device=recv.device))
    else:  # the kernel writes through raw pointers: every output is checked like recv
        obs, reward, done = _check_out(out, width, n_global, recv.device)
    with torch.cuda.device(recv.device):
        C.check(L.st_unwire_shards(width, height, n_global, shards, cap, _ptr(recv), _ptr(obs), _ptr(reward),
                                   _ptr(done), _stream_ptr(recv.device)))
    return obs, reward, done
