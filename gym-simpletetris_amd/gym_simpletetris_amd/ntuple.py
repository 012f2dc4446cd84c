"""N-tuple networks for the batched engine (include/simpletetris.h, "N-tuple
network"): the network's description, which TetrisBatch.set_ntuple uploads,
and the TD(0) table update on policy_ntuple's outputs.

A network is T tuples (x, y, w, h, flip, base): a w x h window of the board
with its top-left cell at column x, row y (row 0 is the top); the window's bit
pattern, column by column (mirrored under flip), is an index into the table at
`base`.  The value of a board is the float32 sum of the T table entries, in
tuple order.  This module needs no GPU; the evaluation is the library's
(TetrisBatch.ntuple_eval, .policy_ntuple, .play_ntuple)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as C


class NTupleNet:
    """T tuples on a width x height board, validated by the header's rules
    (ValueError).  `.tuples` int32 [T, 6] (read-only), `.table_len` (the
    number of float32 entries a table needs), `.new_table(device)`."""

    def __init__(self, width: int, height: int, tuples):
        self.width, self.height = int(width), int(height)
        raw = np.asarray(tuples)
        if raw.ndim != 2 or raw.shape[1] != 6 or raw.dtype.kind not in "iu":
            raise ValueError(f"tuples: need integers of shape [T, 6] (x, y, w, h, flip, base), got {raw.dtype} "
                             f"{raw.shape}")
        t = raw.astype(np.int64)
        if not 1 <= len(t) <= C.NTUPLE_MAX_TUPLES:
            raise ValueError(f"tuples: T = {len(t)} outside [1, {C.NTUPLE_MAX_TUPLES}]")
        table_len = 0
        for i, (x, y, w, h, flip, base) in enumerate(t.tolist()):
            bad = ("w or h < 1" if w < 1 or h < 1 else
                   f"more than {C.NTUPLE_MAX_BITS} cells" if w * h > C.NTUPLE_MAX_BITS else
                   "columns off the board" if x < 0 or x + w > self.width else
                   "rows off the board" if y < 0 or y + h > self.height else
                   "flip not 0 or 1" if flip not in (0, 1) else
                   "negative base" if base < 0 else
                   "table_len above 2^31 - 1" if base + (1 << (w * h)) > 2 ** 31 - 1 else None)
            if bad:
                raise ValueError(f"tuple {i} (x {x}, y {y}, w {w}, h {h}, flip {flip}, base {base}) on a "
                                 f"{self.width}x{self.height} board: {bad}")
            table_len = max(table_len, base + (1 << (w * h)))
        self.tuples = np.ascontiguousarray(t, np.int32)
        self.tuples.setflags(write=False)
        self.table_len = int(table_len)

    def __len__(self):
        return len(self.tuples)

    @classmethod
    def systematic(cls, width: int, height: int, w: int, h: int, share: bool = False, mirror: bool = False):
        """Every position of a w x h window, in column-major order of (x, y)
        (x outermost), one table of 2^(w h) entries per position -- or one
        shared table with share=True.  With mirror=True every tuple is
        followed by its mirror image (width - x - w, y, w, h, flip 1) on the
        same base, so a board and its mirror image have one value."""
        if w < 1 or h < 1 or w > width or h > height:
            raise ValueError(f"a {w}x{h} window does not fit a {width}x{height} board")
        size, rows, k = 1 << (w * h), [], 0
        for x in range(width - w + 1):
            for y in range(height - h + 1):
                base = 0 if share else k * size
                rows.append((x, y, w, h, 0, base))
                if mirror:
                    rows.append((width - x - w, y, w, h, 1, base))
                k += 1
        return cls(width, height, rows)

    def new_table(self, device, fill: float = 0.0) -> torch.Tensor:
        """A float32 [table_len] tensor on `device`, every entry `fill`."""
        return torch.full((self.table_len,), float(fill), dtype=torch.float32, device=device)


def td_update(table: torch.Tensor, index: torch.Tensor, delta: torch.Tensor, alpha: float) -> torch.Tensor:
    """The TD(0) afterstate step on policy_ntuple's outputs, on the tensors'
    device: table[index[t, e]] += alpha * delta[e] for every tuple t and every
    env e with index[0, e] >= 0 (an env without a chosen slot, or whose chosen
    slot ends the game, has -1 rows: no entry was read for it, none is
    updated).  table float32 [>= table_len], index int32/int64 [T, n], delta
    float32 [n]; one index_add_ (entries several tuples share are added to
    once per tuple).  Returns table."""
    if table.dim() != 1 or table.dtype != torch.float32:
        raise ValueError("table: a float32 vector is needed")
    if index.dim() != 2 or index.dtype not in (torch.int32, torch.int64):
        raise ValueError("index: an int32 / int64 [T, n] tensor is needed")
    if delta.shape != index.shape[1:] or delta.dtype != torch.float32:
        raise ValueError(f"delta: a float32 [{index.shape[1]}] tensor is needed")
    if not (table.device == index.device == delta.device):
        raise ValueError("table, index and delta must be on one device")
    live = index[0] >= 0
    src = torch.where(live, delta * float(alpha), torch.zeros_like(delta))
    idx = torch.where(live[None], index, torch.zeros_like(index)).to(torch.int64)
    table.index_add_(0, idx.reshape(-1), src[None].expand(index.shape).reshape(-1))
    return table
