"""TetrisEngine: the reference's engine class (tetris_env.py:125-335) on the
HIP engine -- step(action) -> (state, reward, done), clear(), render(),
get_info() and the counters as attributes, for code that drives the engine
directly (search, planners).  Every rule runs in the step kernel; a step is
one st_step_export launch and one synchronize (envs/_single.py).

Deviations from the reference class: `anchor` always holds
ints; clear()'s return value does not alias `board`; value_action_map,
action_value_map and valid_action_count() are not provided.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from ..engine import SHAPE_NAMES
from . import _single as S

# tetris_env.py:10-19, shape_names order T, J, L, Z, S, I, O
_BASE_CELLS = (
    ((0, 0), (-1, 0), (1, 0), (0, -1)),
    ((0, 0), (-1, 0), (0, -1), (0, -2)),
    ((0, 0), (1, 0), (0, -1), (0, -2)),
    ((0, 0), (-1, 0), (0, -1), (1, -1)),
    ((0, 0), (-1, -1), (0, -1), (1, 0)),
    ((0, 0), (0, -1), (0, -2), (0, -3)),
    ((0, 0), (0, -1), (-1, 0), (-1, -1)),
)


def _cell_table():
    """CELLS[id][rot]: the four (i, j) cells of piece `id` after `rot`
    applications of rotated(cclk=False), (i, j) -> (j, -i)
    (tetris_env.py:22-26), in the reference's cell order -- the piece word's
    (id, rot) as the reference's `shape` (the kernels' piece table is built
    the same way: base cells, then the rotation rule)."""
    tab = []
    for base in _BASE_CELLS:
        cells, rots = list(base), []
        for _ in range(4):
            rots.append(tuple(cells))
            cells = [(j, -i) for i, j in cells]
        tab.append(tuple(rots))
    return tuple(tab)


CELLS = _cell_table()


class TetrisEngine:
    def __init__(self, width, height, lock_delay=0, step_reset=False, reward_step=False,
                 penalise_height=False, penalise_height_increase=False, advanced_clears=False,
                 high_scoring=False, penalise_holes=False, penalise_holes_increase=False, *,
                 device=None, rng: str = "global", seed: Optional[int] = None):
        self.width = width
        self.height = height
        self._core = S.SingleEnv(width, height, dict(
            lock_delay=lock_delay, step_reset=step_reset, reward_step=reward_step,
            penalise_height=penalise_height, penalise_height_increase=penalise_height_increase,
            advanced_clears=advanced_clears, high_scoring=high_scoring, penalise_holes=penalise_holes,
            penalise_holes_increase=penalise_holes_increase), device=device, rng=rng, seed=seed, f32=True)
        self.nb_actions = 7  # len(value_action_map), tetris_env.py:162
        self.shape_counts = self._core.shape_counts  # the live dict (:181)
        # the reference's initial values (:165-176) until the first clear()
        self.time = -1
        self.score = -1
        self.holes = 0
        self.lines_cleared = 0
        self.piece_height = 0
        self.anchor = None
        self.shape = None
        self.shape_name = None
        self.n_deaths = 0
        self._lock_delay = 0

    def seed(self, seed=None):
        """random.seed(seed) in 'global' mode, the engine's private MT19937 otherwise."""
        self._core.seed(seed)
        return [seed]

    def _take(self, st):
        """The attributes from a read-back's counter rows."""
        self.time = st[S.TIME]
        self.score = st[S.SCORE]
        self.lines_cleared = st[S.LINES]
        self.holes = st[S.HOLES]
        self.piece_height = st[S.HEIGHT]
        self.n_deaths = st[S.DEATHS]
        pw = st[S.PIECE] & 0xFFFFFFFF  # id | rot << 3 | anchor_x << 5 | anchor_y << 11 | lock << 17
        sid = pw & 7
        self.shape_name = SHAPE_NAMES[sid]
        self.shape = list(CELLS[sid][(pw >> 3) & 3])
        self.anchor = ((pw >> 5) & 63, (pw >> 11) & 63)
        self._lock_delay = pw >> 17
        self._core.refresh_counts(st)

    def step(self, action):
        """tetris_env.py:243-304 -> (state float64 [width, height], reward in
        the reference's Python type, done)."""
        if self.anchor is None:  # the reference subscripts anchor = None (:244)
            raise TypeError("'NoneType' object is not subscriptable: step() before clear() (tetris_env.py:244)")
        obs, r, d, st, _ = self._core.step(action)
        self._take(st)
        return obs.astype(np.float64), r, d

    def clear(self):
        """tetris_env.py:306-315: the counters but n_deaths and shape_counts
        zeroed, a new piece, the empty board returned."""
        obs, st, _ = self._core.reset()
        self._take(st)
        return obs.astype(np.float64)

    def render(self):
        """tetris_env.py:317-321: the board with the piece overlaid; no step."""
        if self.anchor is None:  # _set_piece iterates shape = None (:324)
            raise TypeError("'NoneType' object is not iterable: render() before clear() (tetris_env.py:324)")
        return self._core.render().astype(np.float64)

    @property
    def board(self):
        """The board without the piece, float64 [width, height], read from the device on demand."""
        w = self._core.board()
        return ((w[:, None] >> np.arange(self.height, dtype=np.uint32)) & 1).astype(np.float64)

    def get_info(self):
        """tetris_env.py:232-241; 'statistics' is the live shape_counts."""
        return {"time": self.time,
                "current_piece": self.shape_name,
                "score": self.score,
                "lines_cleared": self.lines_cleared,
                "holes": self.holes,
                "deaths": self.n_deaths,
                "statistics": self.shape_counts}

    def __repr__(self):
        """tetris_env.py:329-335."""
        rows = self.render().T
        s = "o" + "-" * self.width + "o\n"
        s += "\n".join("|" + "".join("X" if j else " " for j in i) + "|" for i in rows)
        s += "\no" + "-" * self.width + "o"
        return s

    def close(self):
        if getattr(self, "_core", None) is not None:
            self._core.close()
            self._core = None
