"""Gym surface of SimpleTetris-v0 on the MI355X engine.

TetrisEnv     -- the reference's single-env class (tetris_env.py:338-467;
                 its engine class is envs/tetris_engine.py, the plumbing
                 both share envs/_single.py):
                 same constructor kwargs, spaces, step/reset/render/close,
                 numpy float32 observations, the reference's reward *types*
                 (int / np.int64 / float / np.float64, R18) and info dict.
                 By default its pieces come from CPython's GLOBAL `random`
                 exactly as the reference's do (tetris_env.py:187): the global
                 MT19937 state is uploaded before and read back after every
                 call, so a program that seeds `random` gets the reference's
                 games bit-for-bit.  Its GPU work is issued on the stream
                 that was current when it was constructed, with one
                 synchronize per call.
TetrisVecEnv  -- the batched surface: N envs, torch tensors on the GPU,
                 per-env CPython MT19937 streams random.seed(seed + e).
Both run every game rule in the HIP kernels (engine.TetrisBatch); there is no
CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes
import sys
import weakref
from typing import Optional

import numpy as np
import torch

from .. import _lib as C
from .. import spaces
from ..engine import TetrisBatch
from ._single import SingleEnv


def _obs_space(obs_type, width, height, extend_dims):
    """tetris_env.py:381-392."""
    if obs_type == "ram":
        shape = (width, height, 1) if extend_dims else (width, height)
    elif obs_type == "grayscale":
        shape = (84, 84, 1) if extend_dims else (84, 84)
    elif obs_type == "rgb":
        shape = (84, 84, 3)
    else:
        return None
    return spaces.Box(0, 1, shape=shape, dtype=np.float32)


class TetrisEnv:
    metadata = {"render.modes": ["human", "rgb_array"], "render_fps": 8}  # :339

    def __init__(self, width=10, height=20, obs_type="ram", extend_dims=False,
                 render_mode="rgb_array", reward_step=False, penalise_height=False,
                 penalise_height_increase=False, advanced_clears=False, high_scoring=False,
                 penalise_holes=False, penalise_holes_increase=False, lock_delay=0,
                 step_reset=False, *, device=None, rng: str = "global", seed: Optional[int] = None):
        self.width = width
        self.height = height
        self.obs_type = obs_type
        self.extend_dims = extend_dims
        self.render_mode = render_mode
        self.window_size = 512
        # the env itself -- record, RNG mirror, live statistics, reward types:
        # shared with TetrisEngine (envs/_single.py); a step is ONE launch
        # (st_step_export) and one synchronize, plus the image launch for
        # grayscale / rgb
        self._core = SingleEnv(width, height, dict(
            lock_delay=lock_delay, step_reset=step_reset, reward_step=reward_step,
            penalise_height=penalise_height, penalise_height_increase=penalise_height_increase,
            advanced_clears=advanced_clears, high_scoring=high_scoring, penalise_holes=penalise_holes,
            penalise_holes_increase=penalise_holes_increase), device=device, rng=rng, seed=seed,
            f32=obs_type == "ram", image_channels={"grayscale": 1, "rgb": 3}.get(obs_type, 0))
        self.engine = self._core.batch  # the one-env TetrisBatch
        self.action_space = spaces.Discrete(7)           # :377
        self.observation_space = _obs_space(obs_type, width, height, extend_dims)
        self.window = None
        self.clock = None
        self._started = False

    def seed(self, seed=None):
        """Seed the piece RNG: random.seed(seed) in 'global' mode (what a user
        of the reference does), the env's private MT19937 otherwise."""
        self._core.seed(seed)
        return [seed]

    # ------------------------------------------------------------- gym API
    def _observation(self, obs, img):
        """TetrisEnv._observation (tetris_env.py:413-433) + float32 cast, from
        the read-back's float32 obs (ram) or image (grayscale / rgb)."""
        if self.obs_type == "ram":
            return obs.reshape(self.width, self.height, 1) if self.extend_dims else obs
        if self.obs_type == "grayscale":
            return img if self.extend_dims else img.reshape(84, 84)
        return img

    def step(self, action):
        """TetrisEnv.step (tetris_env.py:397-403)."""
        if not self._started:
            raise AttributeError("step() before reset(): the reference fails at tetris_env.py:244")
        core = self._core
        obs, r, d, st, img = core.step(action)
        return self._observation(obs, img), r, d, core.info(st)

    def reset(self, return_info=False):
        """TetrisEnv.reset (tetris_env.py:405-411): clear(); obs is the empty
        board (clear() returns the board before the new piece is drawn)."""
        obs, st, img = self._core.reset()
        self._started = True
        obs = self._observation(obs, img)
        return (obs, self._core.info(st)) if return_info else obs

    def render(self, mode="human"):
        """render('rgb_array'): 160x160x3 uint8 frame (tetris_env.py:458-462)."""
        if mode == "rgb_array":
            self._core.sync()  # the env's own stream first (its steps), then the current one
            packed = self.engine.render_packed()
            img = self.engine.grayscale(packed, 160, 3, as_u8=True)[0]
            return img.cpu().numpy()
        if mode == "human":
            raise NotImplementedError("render('human') needs pygame; out of scope for the GPU engine")
        raise NotImplementedError(mode)

    def close(self):
        """tetris_env.py:466-467."""
        if getattr(self, "engine", None) is not None:
            self._core.close()
            self.engine = None


class _SlotLayout:
    """The part sizes and byte offsets of a vector env's output slot,
    computed once per env (every slot of it has the same layout)."""

    def __init__(self, n, width, height, f32, final):
        nd = (n + 3) // 4  # int32 words holding done's n bytes
        wn = width * n
        # whole rows first: obs and the final obs start 16-B aligned whenever
        # n % 4 == 0 (the step kernel's 16-B store path)
        self.sizes = (wn, wn, C.NSTAT * n, n, nd) if final else (wn, C.NSTAT * n, n, nd)
        self.total = sum(self.sizes)
        offs = [0]
        for z in self.sizes[:-1]:
            offs.append(offs[-1] + 4 * z)
        self.offs = tuple(offs)
        self.n, self.width, self.height, self.f32, self.final = n, width, height, f32, final


class _Slot:
    """One set of st_step_vec outputs: with copy=False the vector env
    alternates two; with copy=True every step gets a fresh one, handed to
    the caller (the env never writes it again).  The int32 outputs are views
    of ONE allocation (obs | final obs | info rows | reward | done bytes),
    the float32 obs a second one: two caching-allocator calls per step.  The
    per-step cost of copy=True is these Python-level tensor ops, so only the
    returned obs / reward / done are viewed here; the info rows and the
    final obs are viewed when an info is read (VecInfo)."""

    def __init__(self, lay: _SlotLayout, dev):
        n = lay.n
        self.lay = lay
        flat = torch.empty(lay.total, dtype=torch.int32, device=dev)
        self.parts = parts = flat.split(lay.sizes)  # one op for every part
        self.obs = parts[0].view(lay.width, n)
        self.reward = parts[-2]
        self.done = parts[-1].view(torch.uint8)[:n].view(torch.bool)
        self.obs_f32 = torch.empty((n, lay.width, lay.height), dtype=torch.float32, device=dev) if lay.f32 else None
        base, o = flat.data_ptr(), lay.offs
        vp = ctypes.c_void_p
        self.ptrs = (vp(base), None if self.obs_f32 is None else vp(self.obs_f32.data_ptr()), vp(base + o[-2]),
                     vp(base + o[-1]), vp(base + o[1]) if lay.final else None, vp(base + o[-3]))
        self.owner = None  # weakref to the VecInfo that reads this slot
        self.stream = -1    # the stream its last step was written on (a raw handle value; None =
                            # the null stream; -1 = never written)
        self.busy = 0       # copy=True pool: times it was found held since its last step
        # the root tensor is kept: under torch.inference_mode() views do not
        # keep their base alive, and the baseline below must count only
        # long-lived owners
        self._flat = flat
        self._flat_st = flat.untyped_storage()
        self._f32_st = self.obs_f32.untyped_storage() if self.obs_f32 is not None else None
        self._flat_cd = self._flat_st._cdata
        self._idle = self._refs()  # the counts while only the slot holds its tensors

    def _refs(self):
        """Python references to the tensors step() hands out, and the owners
        of the two allocations (every view of them, the caller's included)."""
        g, use = sys.getrefcount, torch._C._storage_Use_Count
        if self.obs_f32 is None:  # (None's own count moves all the time: not counted)
            return g(self.obs), g(self.reward), g(self.done), use(self._flat_cd)
        return (g(self.obs), g(self.reward), g(self.done), g(self.obs_f32), use(self._flat_cd),
                use(self._f32_st._cdata))

    def idle(self) -> bool:
        """Nothing outside the slot still holds its outputs (no returned
        tensor, view of one, info or info tensor): a copy=True env may write
        the next step into it without touching anything the caller kept."""
        return self._refs() == self._idle

    def info_rows(self):
        return self.parts[-3].view(C.NSTAT, self.lay.n)

    def final_obs(self):
        return self.parts[1].view(self.lay.width, self.lay.n) if self.lay.final else None


class _SlotPool:
    """copy=True's output slots, oldest first.  take() reuses one of the two
    oldest if nothing outside the pool holds it (_Slot.idle) -- callers
    release in order, so a loop that keeps the last d steps' outputs settles
    at d + 1 slots and then allocates nothing -- else builds a new one (the
    oldest is dropped at `cap`).  A slot found held at the front more often
    than the pool is long is kept for good: the pool forgets it (it is freed
    when the caller drops it), so a few kept-forever steps do not block the
    reuse behind them."""

    def __init__(self, cap: int):
        self.q: collections.deque = collections.deque()
        self.cap = cap

    def __len__(self):
        return len(self.q)

    def clear(self):
        self.q.clear()

    def take(self, new):
        """(slot, reused): a released slot, or new() when none is."""
        q = self.q
        if q:  # the common case: the oldest slot was released -- it goes to the back
            z = q[0]
            if z.idle():
                q.rotate(-1)
                z.busy = 0
                return z, True
        return self._take_slow(new)

    def _take_slow(self, new):
        q = self.q
        slot = None
        for i in range(min(2, len(q))):
            z = q[i]
            if z.idle():
                del q[i]
                slot = z
                break
            z.busy += 1
        reused = slot is not None
        if slot is None:
            slot = new()
            if len(q) >= self.cap:
                q.popleft()  # still the caller's: it is freed when they drop it
        while q and q[0].busy > max(8, len(q)) and not q[0].idle():
            q.popleft()
        slot.busy = 0
        q.append(slot)
        return slot, reused


class VecInfo:
    """get_info() (tetris_env.py:232-241) of one TetrisVecEnv step for all N
    envs, as int32 GPU tensors built on first access: time, score,
    lines_cleared, holes, deaths, piece_height, current_piece (shape id, the
    index into SHAPE_NAMES), statistics [7, N]; ep_time / ep_score /
    ep_lines / ep_holes (the finished episode's counters where the env was
    reset in this step, else 0); and, with the gym reset convention,
    final_observation (the terminal obs of the envs reset in this step, in
    the env's obs format; zeros elsewhere) and _final_observation (bool [N],
    which envs those are).

    The step kernel writes the counters into the slot this info reads, so
    building it costs nothing per step.  With copy=True (the default) the
    slot is the caller's; with copy=False the env reuses a slot two steps
    later and copies it into this object first if this info is still alive
    then (a counter tensor taken out of the info and kept past that is a
    view of the slot: clone it to keep it)."""

    def __init__(self, env: "TetrisVecEnv", slot: _Slot):
        self._env = env
        self._slot = slot  # the info rows / final obs are viewed on first access
        self._info = self._final = None
        self._done = slot.done
        self._cache = None

    def _views(self):
        if self._slot is not None:
            self._info, self._final = self._slot.info_rows(), self._slot.final_obs()
            self._slot = None

    def _detach(self):
        """Own copies of the slot's tensors (the env is about to reuse it;
        stream-ordered before the step that overwrites it).  A dict already
        built from the slot is rebuilt from the copies on the next access
        (its counter tensors were views into the slot)."""
        self._views()
        self._info = self._info.clone()
        self._done = self._done.clone()
        if self._final is not None:
            self._final = self._final.clone()
        self._cache = None

    def _load(self):
        if self._cache is None:
            self._views()
            env = self._env
            d = env.engine.info_tensors(self._info)
            d["current_piece"] = self._info[C.STAT["piece"]] & 7
            if self._final is not None:
                fin = torch.where(self._done.unsqueeze(0), self._final, torch.zeros_like(self._final))
                d["final_observation"] = env._obs(fin, None)
                d["_final_observation"] = self._done.clone()
            self._cache = d
        return self._cache

    def __getitem__(self, k):
        return self._load()[k]

    def get(self, k, default=None):
        return self._load().get(k, default)

    def keys(self):
        return self._load().keys()

    def items(self):
        return self._load().items()

    def __contains__(self, k):
        return k in self._load()

    def __iter__(self):
        return iter(self._load())


class TetrisVecEnv:
    """N SimpleTetris-v0 envs stepped together on one GPU.

    step(actions) -> (obs, reward int32 [N], done bool [N], info)
      obs: float32 [N, W, H] ('ram', '(...,1)' with extend_dims), or
           [N, 84, 84(, 1|3)] for 'grayscale' / 'rgb', or the packed uint32
           [W, N] words with obs_format='packed'.
    With autoreset=True (default) envs that died are reset inside the same
    kernel (TetrisEngine.clear).  autoreset_obs='reset' (default; gym's
    vector-env convention): the returned obs of such an env is
    its RESET obs -- the empty board clear() returns (tetris_env.py:306-315,
    :405-411) -- and its terminal observation (what the reference's step
    returned) is in info['final_observation'] (materialised on first access,
    valid where info['_final_observation']); 'terminal': the returned obs is
    the terminal observation itself (no final_observation key).
    info['ep_score'] / ['ep_lines'] / ['ep_time'] / ['ep_holes'] hold the
    finished episode's counters.  One st_step_vec launch per step writes the
    obs, reward, done, the terminal obs and the info counters.  copy=True
    (default; gym's SyncVectorEnv convention, and the reference's step
    returns a fresh np.copy of the board, tetris_env.py:302): the kernel
    writes them into tensors of their own, which the env never touches
    again while the caller keeps any of them -- obs / reward / done / info,
    a view of one, an info tensor (a slot of a recent step is reused once
    none of that is referenced any more, when torch's allocator would hand
    the memory out again: `slots_reused` counts those steps; the pool
    follows how many steps' outputs the caller keeps).  Outputs read on
    another stream: call record_stream(stream) once, as Tensor.record_stream
    for torch's allocator -- a reused slot is then written only after the
    work queued on that stream.  copy=False: they live in one of two output slots
    that alternate, so they are overwritten two steps later (an info object
    kept longer takes a copy; the obs / reward / done tensors do not; a step
    that raised -- a rejected action batch -- wrote nothing and does not count) -- the
    fast path, for loops that consume each step's outputs right away.
    reset(return_info=True) returns (obs, info) like the reference's
    reset (:405-411): the post-reset counters (time 0, score 0, the new
    current_piece, the persisting deaths and statistics).
    Actions outside 0..6 raise KeyError like the reference's.  By default
    (`validate_actions='async'`) the step kernel checks the actions it loads
    anyway and sets a sticky flag in mapped host memory: no extra launch and
    no sync; the flagged step has already been applied with the bad action
    acting as idle, and the KeyError comes at the next step() after the flag
    is seen or from check_actions().  `validate_actions=True` is the
    reference's immediate KeyError, before any state changes: actions on the
    GPU are checked by a small kernel the step launch is gated on
    (st_gate_actions: the step changes nothing if an action is bad), and the
    host waits for that check only, with the step already queued behind it;
    `False` does not check (out-of-range values act as idle).  Host (numpy /
    list) actions are always checked up front.
    """

    def __init__(self, num_envs: int, width=10, height=20, obs_type="ram", extend_dims=False,
                 reward_step=False, penalise_height=False, penalise_height_increase=False,
                 advanced_clears=False, high_scoring=False, penalise_holes=False,
                 penalise_holes_increase=False, lock_delay=0, step_reset=False, *,
                 device=None, seed: int = 0, global_offset: int = 0, autoreset: bool = True,
                 autoreset_obs: str = "reset", obs_format: str = "f32", validate_actions="async",
                 copy: bool = True):
        if obs_format not in ("f32", "packed"):
            raise ValueError("obs_format must be 'f32' or 'packed'")
        if autoreset_obs not in ("reset", "terminal"):
            raise ValueError("autoreset_obs must be 'reset' (gym's convention) or 'terminal'")
        self.num_envs = int(num_envs)
        self.width, self.height = width, height
        self.obs_type, self.extend_dims, self.obs_format = obs_type, extend_dims, obs_format
        self.autoreset, self.autoreset_obs = bool(autoreset), autoreset_obs
        self.engine = TetrisBatch(self.num_envs, width=width, height=height,
                                  lock_delay=lock_delay, step_reset=step_reset,
                                  reward_step=reward_step, penalise_height=penalise_height,
                                  penalise_height_increase=penalise_height_increase,
                                  advanced_clears=advanced_clears, high_scoring=high_scoring,
                                  penalise_holes=penalise_holes,
                                  penalise_holes_increase=penalise_holes_increase,
                                  autoreset="same_step" if autoreset else "none", device=device,
                                  validate_actions=validate_actions)
        self.engine.seed([seed + global_offset + e for e in range(self.num_envs)])
        self.single_action_space = spaces.Discrete(7)
        self.single_observation_space = _obs_space(obs_type, width, height, extend_dims)
        self.device = self.engine.device
        self._want_f32 = obs_format == "f32" and obs_type == "ram"
        fin = self.autoreset and autoreset_obs == "reset"
        self.copy = bool(copy)
        self._fin = fin
        self._lay = _SlotLayout(self.num_envs, width, height, self._want_f32, fin)
        self._slots = [] if self.copy else [_Slot(self._lay, self.device) for _ in range(2)]
        # copy=True: the slots of recent steps, oldest first, reused once the
        # caller holds nothing of them (_Slot.idle).  The pool grows to the
        # caller's holding depth (a loop that keeps each step's outputs for d
        # steps settles at d + 1 slots, and every step then reuses the oldest:
        # one idle() test per step), up to _SLOT_BYTES of slots
        slot_bytes = 4 * self._lay.total + (4 * self.num_envs * width * height if self._want_f32 else 0)
        self._pool = _SlotPool(max(4, min(64, self._SLOT_BYTES // max(slot_bytes, 1))))
        self.slots_reused = 0
        self._consumers: list = []  # record_stream: streams that read the outputs
        self._k = 0
        self._step_vec = self.engine._L.st_step_vec
        self._stream_wait = self.engine._L.st_stream_wait

    _SLOT_BYTES = 1 << 30  # copy=True: most memory the slot pool keeps for reuse

    def _new_slot(self):
        return _Slot(self._lay, self.device)

    def record_stream(self, stream) -> None:
        """Declare that the outputs of this env's steps are read on `stream`
        (a torch.cuda.Stream or a raw hipStream_t handle) -- the vector env's
        counterpart of Tensor.record_stream, which torch's caching allocator
        honours and this env's output slots do as well: before a step writes
        into a slot again (a copy=True slot the caller released, or
        copy=False's alternating slots), the env's stream waits, on the
        device, for the work queued on every registered stream by then.  A
        consumer on the env's own stream needs nothing (stream order)."""
        h = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
        if all(c.value != h for c in self._consumers):
            self._consumers.append(ctypes.c_void_p(h))

    def _order_reuse(self, s: ctypes.c_void_p, prev) -> None:
        """A slot is written on stream s again: s waits for the registered
        consumer streams and for the stream that last wrote it (if another)."""
        waits = [c for c in self._consumers if c.value != s.value]
        if prev != -1 and prev != s.value:
            waits.append(ctypes.c_void_p(prev))
        if waits:
            with torch.cuda.device(self.device):
                for c in waits:
                    C.check(self._stream_wait(s, c))

    def _obs(self, packed, f32):
        if self.obs_format == "packed":
            return packed
        if self.obs_type == "ram":
            o = f32 if f32 is not None else self.engine.obs_to_f32(packed)
            return o.unsqueeze(-1) if self.extend_dims else o
        ch = 1 if self.obs_type == "grayscale" else 3
        g = self.engine.grayscale(packed, 84, ch)
        return g if (self.obs_type == "rgb" or self.extend_dims) else g.squeeze(-1)

    def reset(self, return_info: bool = False):
        """TetrisEnv.reset (tetris_env.py:405-411) for every env: clear()
        (:306-315), whose observation is the empty board; with return_info
        also get_info() after the reset (:232-241) as a dict of [N] tensors
        (ep_* 0: no episode finished in a reset)."""
        self.engine.reset()
        zeros = torch.zeros((self.width, self.num_envs), dtype=torch.int32, device=self.device)
        if self.obs_format == "packed":
            obs = zeros
        else:
            obs = self._obs(zeros, torch.zeros((self.num_envs, self.width, self.height),
                                               device=self.device) if self.obs_type == "ram" else None)
        if not return_info:
            return obs
        st = self.engine.state_tensors(("stats",), sync=False)["stats"][:, :self.num_envs].clone()
        for k in ("ep_time", "ep_score", "ep_lines", "ep_holes"):
            st[C.STAT[k]] = 0
        info = self.engine.info_tensors(st)
        info["current_piece"] = st[C.STAT["piece"]] & 7
        return obs, info

    def step(self, actions):
        eng = self.engine
        a, gated = eng._actions(actions, gate=True)
        s = eng._stream()
        # the slot this step writes (chosen inline: a helper call per step shows in the step time)
        k0 = self._k
        if self.copy:  # this step's outputs, the caller's from now on
            slot, reused = self._pool.take(self._new_slot)
            if reused:
                self.slots_reused += 1
                if self._consumers or slot.stream != s.value:  # (a reused slot was written before)
                    self._order_reuse(s, slot.stream)
        else:
            slot = self._slots[self._k]
            self._k ^= 1
            held = slot.owner() if slot.owner is not None else None
            if held is not None:  # an info from two steps ago is still alive: it keeps a copy
                held._detach()
            if self._consumers or (slot.stream != -1 and slot.stream != s.value):
                self._order_reuse(s, slot.stream)
        prev = slot.stream
        slot.stream = s.value
        po, pf, pr, pd, pfin, pinfo = slot.ptrs
        args = (eng._ctx, ctypes.c_void_p(a.data_ptr()), po, pf, pr, pd, pfin, pinfo, s)
        try:
            if gated:  # validate_actions=True, device actions: KeyError if the step was skipped
                eng._gated_launch(a, s, self._step_vec, args)
            else:
                C.check(self._step_vec(*args))
        except BaseException:
            # a step that raised wrote nothing: copy=False's alternation stays
            # where it was, so the next step takes this slot again and the last
            # successful step's outputs keep their two steps
            self._k, slot.stream = k0, prev
            raise
        info = VecInfo(self, slot)
        if not self.copy:
            slot.owner = weakref.ref(info)
        return self._obs(slot.obs, slot.obs_f32), slot.reward, slot.done, info

    def check_actions(self):
        """validate_actions='async': raise KeyError if an action outside 0..6
        reached any step so far (waits for the queued work)."""
        self.engine.check_actions()

    def afterstates(self, boards: bool = True, out=None, features="base"):
        """TetrisBatch.afterstates of the engine, on its stream: every
        placement of every env's current piece (features and boards), for an
        afterstate agent's afterstates -> score -> argmax ->
        placement_actions -> step loop.  features='bcts': the 18 rows."""
        return self.engine.afterstates(boards=boards, out=out, features=features)

    def placement_actions(self, slots, out=None):
        """TetrisBatch.placement_actions of the engine, on its stream: the
        uint8 actions step() takes, toward the chosen placement slots."""
        return self.engine.placement_actions(slots, out=out)

    def policy_linear(self, weights, out=None, features="base", allowed=None):
        """TetrisBatch.policy_linear of the engine, on its stream: every env's
        best placement under linear feature weights (slot, action, score and
        feature row) in one launch.  features='bcts': over the 18 rows;
        allowed: a slot mask (a Reachable, or int32 [n, S])."""
        return self.engine.policy_linear(weights, out=out, features=features, allowed=allowed)

    def play_linear(self, weights, k, returns=None, episodes=None, obs="none", placements=False, features="base"):
        """TetrisBatch.play_linear of the engine: k steps of policy_linear ->
        step in one library call, straight on the engine (no info, no
        final_observation: with autoreset a finished env simply plays on);
        returns the (returns, episodes) accumulators.  placements=True: at
        placement level (policy_linear -> step_placements).  features='bcts':
        with the 18 rows."""
        return self.engine.play_linear(weights, k, returns=returns, episodes=episodes, obs=obs,
                                       placements=placements, features=features)

    def place(self, slots, out=None):
        """TetrisBatch.place of the engine, on its stream: commit a placement
        slot per env (the piece is teleported there), without stepping."""
        return self.engine.place(slots, out=out)

    def step_placements(self, slots, obs="packed", out=None):
        """TetrisBatch.step_placements of the engine: place(slots), then the
        hard drop that locks the piece, straight on the engine (no info, no
        final_observation); returns its (obs, reward, done)."""
        return self.engine.step_placements(slots, obs=obs, out=out)

    def close(self):
        self._pool.clear()
        self.engine.close()
