"""SingleEnv: one env of the HIP engine behind the reference's single-env
classes -- what TetrisEnv (the Gym surface) and TetrisEngine (the engine
class) share.

It owns the one-env TetrisBatch, the read-back record in pinned host memory
(st_export_env's layout: obs words | reward | done | counters | CPython's MT
words in 'global' mode | the float32 obs), the mirror of CPython's global
`random` (the MT19937 state is uploaded before a call when the program used
`random` since the last one, and taken back after a call that drew pieces),
the env's one live shape-count dict (counts written into it weight the next
draw) and the reference's reward types.  A step is ONE launch
(st_step_export: the step and the record) and one synchronize; reset and
render are their launch plus st_export_env.  All GPU work is issued on the
stream that was current at construction.
"""
from __future__ import annotations

import ctypes
import random
from typing import Optional

import numpy as np
import torch

from .. import _lib as C
from ..engine import SHAPE_NAMES, TetrisBatch, scalar_action

# counter rows of the export record (st_stat)
TIME, SCORE, LINES, HOLES, DEATHS, HEIGHT, C0, PIECE, MT_INDEX = (
    C.STAT[k] for k in ("time", "score", "lines", "holes", "deaths", "piece_height", "count0", "piece",
                        "mt_index"))


def _stream_sync(sp: ctypes.c_void_p):
    """A synchronize of stream `sp` through libsimpletetris (st_stream_sync:
    the runtime its kernels use; torch's stream synchronize costs ~3 us more
    per call)."""
    fn = C.load().st_stream_sync

    def sync():
        C.check(fn(sp))
    return sync


class SingleEnv:
    """`f32`: the record carries the float32 obs (TetrisEnv 'ram',
    TetrisEngine); `image_channels` 1 / 3: every read-back also renders the
    84x84 grayscale / rgb image of the obs (a second launch)."""

    def __init__(self, width, height, engine_kwargs, *, device=None, rng: str = "global",
                 seed: Optional[int] = None, f32: bool = True, image_channels: int = 0):
        if rng not in ("global", "private"):
            raise ValueError("rng must be 'global' (CPython's random, like the reference) or 'private'")
        self.width, self.height = width, height
        self.batch = TetrisBatch(1, width=width, height=height, autoreset="none", device=device,
                                 validate_actions=False,  # step() checks the action itself
                                 **engine_kwargs)
        self.rng_mode = rng
        self.batch.seed([0 if seed is None else seed])
        if rng == "global" and seed is not None:
            random.seed(seed)
        self.scoring = {k: bool(engine_kwargs.get(k)) for k in
                        ("advanced_clears", "penalise_height", "penalise_height_increase")}
        self.stats = None          # the last read-back's counter rows (Python ints [NSTAT])
        # ONE shape-count dict for the env's lifetime, updated in place, like
        # the reference's live shape_counts (tetris_env.py:181, :199, :240):
        # a held reference sees later spawns, and counts written into it
        # weight the next draws (:183-191)
        self.shape_counts = dict.fromkeys(SHAPE_NAMES, 0)
        self._shape_vals = (0,) * 7  # what the env last wrote into it
        self._rng_sync_state = None
        b = self.batch
        dev, L = b.device, b._L
        self._L, self._ctx = L, b._ctx
        # per-step plumbing without per-call allocations: one device tensor per
        # action value, the step's outputs, and ONE read-back record plus the
        # image for grayscale / rgb, written into pinned host buffers and
        # waited for once
        self._acts = [torch.full((1,), a, dtype=torch.uint8, device=dev) for a in range(7)]
        self.p_acts = [ctypes.c_void_p(t.data_ptr()) for t in self._acts]
        self.parts = (C.EXPORT_MT if rng == "global" else 0) | (C.EXPORT_OBS_F32 if f32 else 0)
        self._f32 = f32
        self._f32_at = width + 2 + C.NSTAT + C.MT_N  # the record's float32 obs
        # the export and image kernels write straight into the pinned buffers
        # when the runtime maps them for the device (else: device buffer + copy)
        self.rec = b._pinned(int(L.st_export_words(width, height)), torch.int32)
        self._h_rec = self.rec.host.numpy()
        self._zeros = torch.zeros((width, 1), dtype=torch.int32, device=dev)
        self._scratch = None       # render()'s packed obs
        self._ch = image_channels
        self.img = b._pinned((1, 84, 84, image_channels), torch.float32) if image_channels else None
        self._h_mt = np.zeros(C.MT_N, np.uint32)
        self._h_idx = np.zeros(1, np.int32)
        # per-step constants: output pointers, the stream current at
        # construction, a direct hipStreamSynchronize
        self.po, self.pr, self.pd = (ctypes.c_void_p(t.data_ptr()) for t in (b.obs, b.reward, b.done))
        self.pz = ctypes.c_void_p(self._zeros.data_ptr())
        self.sp = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.sync = _stream_sync(self.sp)
        self._step_export = L.st_step_export

    # ------------------------------------------------------------- RNG mirror
    def seed(self, seed=None):
        """random.seed(seed) in 'global' mode (what a user of the reference
        does), the env's private MT19937 otherwise."""
        if self.rng_mode == "global":
            random.seed(seed)
        else:
            self.batch.seed([0 if seed is None else seed])

    def push_rng(self):
        if self.rng_mode != "global":
            return
        state = random.getstate()
        if self._rng_sync_state is not None and state == self._rng_sync_state:
            return
        internal = state[1]
        self._h_mt[:] = np.asarray(internal[:C.MT_N], dtype=np.uint32)
        self._h_idx[0] = internal[C.MT_N]
        b, L, s = self.batch, self._L, self.sp
        C.check(L.st_copy(ctypes.c_void_p(b._view_ptr("mt")), ctypes.c_void_p(self._h_mt.ctypes.data),
                          C.MT_N * 4, s))
        C.check(L.st_copy(b._stat_ptr(MT_INDEX), ctypes.c_void_p(self._h_idx.ctypes.data), 4, s))
        self._rng_sync_state = state  # the device now mirrors CPython's state

    def push_counts(self):
        """Counts the caller wrote into the shape-count dict since the last
        call take effect like writes into the reference's shape_counts: the
        next draw (:183-191) sees them, and spawns count on from them (:199).
        The device drops its preview (st_mt_sync: the piece drawn one spawn
        ahead with the old counts) and takes the new counts."""
        d = self.shape_counts
        if len(d) == 7 and all(type(d.get(k)) is int for k in SHAPE_NAMES):
            vals = tuple(d[k] for k in SHAPE_NAMES)
            if vals == self._shape_vals:
                return
        else:
            vals = None
        if vals is None or not all(-(1 << 31) <= v < (1 << 31) for v in vals):
            raise ValueError("the shape counts (info['statistics'], shape_counts) may only hold int32 "
                             f"counts for the keys {SHAPE_NAMES} (got {dict(d)!r})")
        L, s = self._L, self.sp
        C.check(L.st_mt_sync(self._ctx, s))
        cnt = np.asarray(vals, dtype=np.int32)
        for i in range(7):
            C.check(L.st_copy(self.batch._stat_ptr(C0 + i), ctypes.c_void_p(cnt.ctypes.data + 4 * i), 4, s))
        self.sync()  # (cnt is pageable host memory)
        self._shape_vals = vals
        if self.stats is not None:
            self.stats[C0:C0 + 7] = list(vals)  # typed_reward compares with these

    def refresh_counts(self, st):
        """The live dict takes the counter rows' shape counts (in place)."""
        vals = tuple(st[C0:C0 + 7])
        if vals != self._shape_vals:
            d = self.shape_counts
            for k, v in zip(SHAPE_NAMES, vals):
                d[k] = v
            self._shape_vals = vals
        return self.shape_counts

    # ------------------------------------------------------------- read-back
    def export(self, obs_ptr, rew_ptr, done_ptr):
        """st_export_env of the env's record on the stream (reset, render)."""
        C.check(self._L.st_export_env(self._ctx, 0, obs_ptr, rew_ptr, done_ptr, self.parts, self.rec.dst, self.sp))

    def land(self, img_src, prev_idx=None, rng: bool = True):
        """The one wait of a call, behind the launch that wrote the record:
        the image of the packed obs at `img_src` for image observations, the
        copies to the pinned buffers where the device cannot write them
        itself, then ONE synchronize.  In 'global' mode CPython's random takes
        the env's MT state if this call drew pieces (`rng`; not for a render).
        Returns (float32 obs [W, H] or None, reward, done, counters [NSTAT]
        as Python ints, image or None)."""
        L, s = self._L, self.sp
        rec, img = self.rec, self.img
        if rec.staged:
            rec.land(s)
        if img is not None:
            C.check(L.st_grayscale(self._ctx, img_src, 84, self._ch, 0, img.dst, s))
            if img.staged:
                img.land(s)
        self.sync()
        rec = self._h_rec
        W = self.width
        obs = None
        if self._f32:  # decoded on the device; a fresh array per call, like np.array(state)
            a = self._f32_at
            obs = rec[a:a + W * self.height].view(np.float32).reshape(W, self.height).copy()
        st = rec[W + 2: W + 2 + C.NSTAT].tolist()  # Python ints (the reference's counters are ints)
        if rng and self.rng_mode == "global":
            idx = st[MT_INDEX]
            # the cached state is CPython's current one (push_rng checked it
            # before the step); only a step that drew changes it
            if prev_idx is None or idx != prev_idx or self._rng_sync_state is None:
                mt = rec[W + 2 + C.NSTAT:W + 2 + C.NSTAT + C.MT_N].view(np.uint32)
                old = self._rng_sync_state if self._rng_sync_state is not None else random.getstate()
                new = (old[0], tuple(mt.tolist()) + (idx,), old[2])
                random.setstate(new)
                self._rng_sync_state = new
        if img is not None:
            img = img.host.numpy()[0].copy()
        return obs, int(rec[W]), bool(rec[W + 1]), st, img

    # ------------------------------------------------------------- the calls
    def step(self, action):
        """TetrisEngine.step (tetris_env.py:243-304): one st_step_export and
        one synchronize (plus the image launch for image observations).
        -> (float32 obs or None, typed reward, done, counters, image or None)."""
        action = scalar_action(action)  # value_action_map[action]'s KeyError, tetris_env.py:245
        self.push_counts()
        prev = self.stats
        self.push_rng()
        po = self.po
        C.check(self._step_export(self._ctx, self.p_acts[action], 0, self.parts, self.rec.dst, po, self.pr,
                                  self.pd, self.sp))
        obs, r, d, st, img = self.land(po, prev[MT_INDEX])
        self.stats = st
        return obs, self.typed_reward(r, d, prev, st), d, st, img

    def reset(self):
        """TetrisEngine.clear (tetris_env.py:306-315); the obs is the empty
        board.  -> (float32 obs or None, counters, image or None)."""
        self.push_counts()
        self.push_rng()
        C.check(self._L.st_reset(self._ctx, None, self.sp))
        self.export(self.pz, None, None)
        obs, _, _, st, img = self.land(self.pz)
        self.stats = st
        return obs, st, img

    def render(self):
        """TetrisEngine.render (tetris_env.py:317-321): the board with the
        piece overlaid as float32 [W, H], no step, no RNG traffic."""
        if self._scratch is None:
            self._scratch = torch.zeros_like(self._zeros)
        p = ctypes.c_void_p(self._scratch.data_ptr())
        C.check(self._L.st_render(self._ctx, p, self.sp))
        self.export(p, None, None)
        return self.land(p, rng=False)[0]

    def board(self):
        """The env's board words [W] (uint32: bit y of word x = board[x, y])."""
        b = self.batch
        rows = np.zeros((self.width, b.stride), np.uint32)  # the [W][stride] board rows; env 0 is column 0
        C.check(self._L.st_copy(ctypes.c_void_p(rows.ctypes.data), ctypes.c_void_p(b._view_ptr("board")),
                                rows.nbytes, self.sp))
        self.sync()
        return rows[:, 0].copy()

    def typed_reward(self, r: int, done: bool, prev, st):
        """Reproduce the Python type the reference's reward ends up with (R18)."""
        if done:
            return int(r)
        if st[C0:C0 + 7] == prev[C0:C0 + 7]:  # no new piece: the step did not lock
            return int(r)
        if self.scoring["advanced_clears"]:
            if self.scoring["penalise_height"] or (
                    self.scoring["penalise_height_increase"] and st[HEIGHT] > prev[HEIGHT]):
                return np.float64(r)
            return float(r)
        return np.int64(r)

    def info(self, st):
        """TetrisEngine.get_info (tetris_env.py:232-241) from counter rows;
        'statistics' is the live shape-count dict, refreshed in place."""
        return {"time": st[TIME],
                "current_piece": SHAPE_NAMES[st[PIECE] & 7],
                "score": st[SCORE],
                "lines_cleared": st[LINES],
                "holes": st[HOLES],
                "deaths": st[DEATHS],
                "statistics": self.refresh_counts(st)}

    def close(self):
        if self.batch is not None:
            self.batch.close()
            self.batch = None
