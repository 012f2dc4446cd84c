"""st_fork (simpletetris.h, "Fork") in the oracle's terms, shared by
test_cpu_fork.py, test_gpu_fork.py and test_gpu_search.py.  A plain module
imported by name, like lookahead_ref.py; it runs no engine code and needs no GPU.

The oracle's Env is a plain struct: the deep copy is a byte copy of it,
ST_FORK_KEEP_RNG a byte copy of everything but its `rng` field.  The `cfg` field
is configuration, which st_fork does not copy either: the target keeps its own.
"""
import ctypes

import numpy as np

from oracle import oracle as O

_SIZE = ctypes.sizeof(O.Env)
_CFG = (O.Env.cfg.offset, O.Env.cfg.offset + ctypes.sizeof(O.Config))
_RNG = (O.Env.rng.offset, O.Env.rng.offset + ctypes.sizeof(O.MT))


def _raw(ob):
    return np.frombuffer(ob.envs, dtype=np.uint8).reshape(ob.n, _SIZE)


def written(n_dst, n_src, index=None, mask=None):
    """(written bool [n_dst], source int64 [n_dst]): st_fork's rule -- masked in
    and the index inside [0, n_src)."""
    idx = np.arange(n_dst, dtype=np.int64) if index is None else np.asarray(index, np.int64)
    m = np.ones(n_dst, bool) if mask is None else np.asarray(mask) != 0
    assert idx.shape == m.shape == (n_dst,)
    return m & (idx >= 0) & (idx < n_src), idx


def fork(dst, src, index=None, mask=None, keep_rng=False):
    """st_fork(dst, src, index, mask, ST_FORK_KEEP_RNG if keep_rng else 0) on
    two OracleBatches (dst may be src): every written env's bytes are its
    source's, except `cfg` and, with keep_rng, `rng`.  Returns `written`."""
    assert (dst.cfg.width, dst.cfg.height) == (src.cfg.width, src.cfg.height)
    wr, idx = written(dst.n, src.n, index, mask)
    before = _raw(src).copy()  # (in place: every source is read as it was)
    out = _raw(dst)
    for e in np.flatnonzero(wr):
        keep = [out[e, a:b].copy() for a, b in ((_CFG,) + ((_RNG,) if keep_rng else ()))]
        out[e] = before[idx[e]]
        for (a, b), v in zip((_CFG,) + ((_RNG,) if keep_rng else ()), keep):
            out[e, a:b] = v
    return wr
