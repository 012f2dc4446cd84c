"""The oracle harness shared by the GPU tests: one copy of the bit helpers,
the step-by-step oracle recorder and its cache, the threaded full-size oracle,
the checks of engine outputs against oracle rows, and the loop that drives one
step surface through them.  A plain module imported by name, like replay.py.

The oracle's state views (field / boards / packed_state) are OracleBatch
methods, oracle/oracle.py.  Every check takes numpy arrays or torch tensors on
any device; tests/test_harness.py proves that each one fails when it should.
"""
import os
import socket
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as O
from oracle.oracle import pack_cols  # noqa: F401  (the one copy; tests import it from here)

# BASELINE C4's scoring flags
C4 = dict(advanced_clears=True, penalise_holes_increase=True, penalise_height_increase=True)
SEED_BASE, ASEED = 1000, 0x5EED  # bench.py's env seeds (SEED_BASE + e) and action stream


def engine():
    import gym_simpletetris_amd as G
    return G


def batch_and_oracle(n, seeds, autoreset="same_step", **kw):
    """A TetrisBatch and an OracleBatch of the same seeds and settings, both reset."""
    b = engine().TetrisBatch(n, autoreset=autoreset, seeds=seeds, **kw)
    ob = O.OracleBatch(n, list(seeds), **kw)
    b.reset()
    ob.reset()
    return b, ob


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class Foreign:
    """A non-torch DLPack producer over a torch tensor's memory."""

    def __init__(self, t):
        self.t = t

    def __dlpack__(self, stream=None, **kw):
        return self.t.__dlpack__() if stream is None else self.t.__dlpack__(stream=stream)

    def __dlpack_device__(self):
        return self.t.__dlpack_device__()


# ------------------------------------------------------------------ bit helpers
def _np(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


def words(obs):
    """Packed obs [W, n] in the engine's layout -> [n, W] u32, the oracle's."""
    return _np(obs).view(np.uint32).T


def unpack_f32(words, H):
    """Column words [..., W] -> float32 cells [..., W, H]."""
    w = np.asarray(words).astype(np.uint32, copy=False)
    return ((w[..., None] >> np.arange(H, dtype=np.uint32)) & 1).astype(np.float32)


def mt_twist(words):
    """One MT19937 refill of every row of words [n, 624] (CPython's
    genrand_uint32 at index 624)."""
    w = np.array(words, dtype=np.uint32)
    for k in range(624):
        y = (w[:, k] & np.uint32(0x80000000)) | (w[:, (k + 1) % 624] & np.uint32(0x7FFFFFFF))
        w[:, k] = w[:, (k + 397) % 624] ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), np.uint32(0x9908B0DF),
                                                                       np.uint32(0))
    return w


def untemper(y):
    """Inverse of MT19937 tempering (so crafted state words produce chosen outputs)."""
    def undo_r(y, s):
        x = y
        for _ in range(32 // s + 1):
            x = y ^ (x >> s)
        return x & 0xFFFFFFFF

    def undo_l(y, s, m):
        x = y
        for _ in range(32 // s + 1):
            x = y ^ ((x << s) & m)
        return x & 0xFFFFFFFF
    y = undo_r(y, 18)
    y = undo_l(y, 15, 0xEFC60000)
    y = undo_l(y, 7, 0x9D2C5680)
    return undo_r(y, 11)


# ------------------------------------------------------------------ the replay adapter
class HipAdapter:
    """TetrisBatch(autoreset='none') behind the replay interface (replay.py).
    sync=False reads board, piece and counter rows without st_mt_sync (they
    are exact without it), so every env keeps the preview the step kernels
    drew one spawn ahead and a reset consumes it; sync=True (get_state) gives
    every preview back after every step, and a reset draws its piece afresh."""

    def __init__(self, n, seeds, kw, sync=True):
        self.b = engine().TetrisBatch(n, autoreset="none", seeds=seeds, **kw)
        self.n, self.sync = n, sync

    def _dev(self, a):
        import torch
        return torch.as_tensor(np.asarray(a, np.uint8), device=self.b.device)

    def _read(self):
        if self.sync:
            return self.b.get_state(("board", "piece", "stats"))
        st = {k: v.cpu().numpy()[..., :self.n] for k, v in
              self.b.state_tensors(("board", "piece", "stats"), sync=False).items()}
        return dict(st, board=st["board"].view(np.uint32), piece=st["piece"].view(np.uint32))

    def reset(self, mask):
        self.b.reset(None if bool(np.all(mask)) else self._dev(mask))

    def set_state(self, i, init):
        st = self.b.get_state(("board", "piece", "stats"))
        st["board"][:, i] = init["board"]
        st["piece"][i] = init["piece"]
        s = st["stats"]
        s[0, i], s[1, i], s[2, i], s[3, i] = init["time"], init["score"], init["lines"], init["holes"]
        s[4, i], s[5, i] = init["height"], init["deaths"]
        s[6:13, i] = init["counts"]
        self.b.set_state(**st)

    def step(self, actions):
        obs, rew, done = self.b.step(self._dev(actions), obs="packed")
        st = self._read()
        s = st["stats"]
        return dict(reward=rew.cpu().numpy(), done=done.cpu().numpy().astype(np.uint8),
                    time=s[0], score=s[1], lines=s[2], holes=s[3], height=s[4], deaths=s[5],
                    counts=s[6:13].T, piece=st["piece"],
                    obs=words(obs), board=st["board"].T)

    def state(self):
        st = self._read()
        return dict(piece=st["piece"], time=st["stats"][0], counts=st["stats"][6:13].T, board=st["board"].T)

    def render(self):
        return words(self.b.render_packed())


# ------------------------------------------------------------------ action streams
def wall_pattern(W, steps, n):
    """actions [steps, n]: env i repeats W // 2 + 1 moves towards one wall
    (enough to reach it from the spawn column), 0..3 rotations and a hard
    drop; i selects the wall, the rotation count, which run comes first, the
    rotation's sense and the phase."""
    i = np.arange(n)
    k = i % 16
    side = (k & 1).astype(np.uint8)  # 0: left, 1: right
    nrot = (k >> 1) & 3
    rot_first = ((k >> 3) & 1).astype(bool)
    rot_act = np.where((i >> 4) & 1, 5, 4).astype(np.uint8)
    moves = W // 2 + 1
    period = moves + nrot + 1
    phase = (i >> 5) % period
    acts = np.empty((steps, n), np.uint8)
    for t in range(steps):
        u = (t + phase) % period
        first = np.where(rot_first, nrot, moves)
        in_first = u < first
        in_second = ~in_first & (u < moves + nrot)
        rot_now = np.where(rot_first, in_first, in_second)
        mov_now = np.where(rot_first, in_second, in_first)
        acts[t] = np.where(rot_now, rot_act, np.where(mov_now, side, 2))
    return acts


# ------------------------------------------------------------------ oracle runs
def record(ob, acts, before=None, after=None):
    """The oracle one step at a time: acts, obs, reward, done, stats of every
    step, and `locked` -- the envs whose piece locked in it (their shape counts
    moved, or they died).  before(t) runs ahead of step t; after(t, locked,
    what before(t) returned) behind it."""
    T, n = acts.shape[0], ob.n
    out = dict(acts=acts, obs=np.empty((T, n, ob.cfg.width), np.uint32), reward=np.empty((T, n), np.int32),
               done=np.empty((T, n), np.uint8), stats=np.empty((T, n, 8), np.int32), locked=np.empty((T, n), bool))
    for t in range(T):
        pre = before(t) if before else None
        spawned = ob.field("counts", (7,)).sum(axis=1)
        r = ob.rollout(acts[t:t + 1])
        for k in ("obs", "reward", "done", "stats"):
            out[k][t] = r[k][0]
        out["locked"][t] = (ob.field("counts", (7,)).sum(axis=1) != spawned) | (r["done"][0] != 0)
        if after:
            after(t, out["locked"][t], pre)
    return out


_REFS = {}


def _freeze(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    elif isinstance(v, (dict, list, tuple)):
        for x in (v.values() if isinstance(v, dict) else v):
            _freeze(x)


def cached_ref(key, make):
    """make() once per key, shared by the tests read-only."""
    if key not in _REFS:
        _REFS[key] = make()
        _freeze(_REFS[key])
    return _REFS[key]


def _threads():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(16, n))


class ParallelOracle:
    """n oracle envs split into contiguous slices, one host thread each
    (ctypes releases the GIL); global env index e keeps seed seed_base + e
    and the splitmix64 action stream of e."""

    def __init__(self, n, kw, parts=None, seed_base=SEED_BASE, aseed=ASEED, board=(10, 20)):
        bounds = np.linspace(0, n, (parts or _threads()) + 1).astype(int)
        self.sl = [(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
        self.aseed = aseed
        self.obs = [O.OracleBatch(b - a, [seed_base + a + e for e in range(b - a)],
                                  width=board[0], height=board[1], **kw) for a, b in self.sl]
        for ob in self.obs:
            ob.reset()
        self.pool = ThreadPoolExecutor(len(self.sl))

    def rollout(self, t0, T, obs=True, stats=False):
        def one(i):
            a, b = self.sl[i]
            acts = O.splitmix64_actions(self.aseed, t0, T, b - a, offset=a)
            return self.obs[i].rollout(acts, want_obs=obs, want_stats=stats)
        rs = list(self.pool.map(one, range(len(self.sl))))
        keys = ("reward", "done") + (("obs",) if obs else ()) + (("stats",) if stats else ())
        return {k: np.concatenate([r[k] for r in rs], axis=1) for k in keys}

    def final_state(self):
        """Structured view of every env (Env struct fields) in global order."""
        return np.concatenate([np.ctypeslib.as_array(ob.envs) for ob in self.obs])

    def packed_state(self):
        """OracleBatch.packed_state of all slices in global order, with the
        MT19937 words [n, 624] and index [n]."""
        parts = [ob.packed_state() for ob in self.obs]
        rng = self.final_state()["rng"]
        return dict({k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0]},
                    mt=rng["mt"].astype(np.uint32), mt_index=rng["index"])

    def close(self):
        self.pool.shutdown()


# ------------------------------------------------------------------ checks
def check_f32(obs_f32, robs, H, t):
    assert np.array_equal(_np(obs_f32), unpack_f32(robs, H)), ("f32 obs", t)


def check_step(ref, t, obs, rew, done, robs=None, sel=None, at=None, H=None):
    """Reward, done and packed obs of one step equal the oracle's row t (of
    its envs sel; robs: another expected obs [n, W], e.g. the reset
    convention's; H: obs is float32 cells [n, W, H]).  Failures name the
    field and the step (at, where row t of a chunked ref is not the step's
    number)."""
    at = t if at is None else at
    row = (lambda a: a) if sel is None else (lambda a: a[sel])
    assert np.array_equal(_np(rew), row(ref["reward"][t])), ("reward", at)
    assert np.array_equal(_np(done).astype(np.uint8), row(ref["done"][t])), ("done", at)
    robs = row(ref["obs"][t]) if robs is None else robs
    if H is None:
        assert np.array_equal(words(obs), robs), ("obs", at)
    else:
        check_f32(obs, robs, H, at)


def check_steps(ref, obs, rew, done, t0=0, sel=None, H=None):
    """check_step over the leading axis of a rollout's outputs: its step k is
    the oracle's row t0 + k."""
    obs, rew, done = _np(obs), _np(rew), _np(done)
    assert len(obs) == len(rew) == len(done) > 0
    for k in range(len(rew)):
        check_step(ref, t0 + k, obs[k], rew[k], done[k], sel=sel, H=H)


def check_info(info, stats_row, done, t):
    """The vector env's info against the oracle's stats row [n, 8] (time,
    score, lines, holes, deaths, piece id, height, lock -- before the reset):
    clear()'s zeros and the ep_* rows where done, the live counters elsewhere."""
    st, done = stats_row, np.asarray(done, bool)
    zero = np.zeros_like(st[:, 0])
    want = {"time": np.where(done, zero, st[:, 0]), "score": np.where(done, zero, st[:, 1]),
            "lines_cleared": np.where(done, zero, st[:, 2]), "holes": np.where(done, zero, st[:, 3]),
            "deaths": st[:, 4], "piece_height": np.where(done, zero, st[:, 6]),
            "ep_time": np.where(done, st[:, 0], zero), "ep_score": np.where(done, st[:, 1], zero),
            "ep_lines": np.where(done, st[:, 2], zero), "ep_holes": np.where(done, st[:, 3], zero)}
    for k, v in want.items():
        assert np.array_equal(_np(info[k]), v), (k, t)
    assert np.array_equal(_np(info["current_piece"])[~done], st[~done, 5]), ("current_piece", t)


def check_final_observation(info, robs, done, t, H=None):
    """info['final_observation'] is the oracle's terminal obs where done and
    zero elsewhere, flagged by info['_final_observation'] (H: float32 cells)."""
    done = np.asarray(done, bool)
    fin, got = np.where(done[:, None], robs, 0), info["final_observation"]
    if H is None:
        assert np.array_equal(words(got), fin), ("final_observation", t)
    else:
        check_f32(got, fin, H, ("final_observation", t))
    assert np.array_equal(_np(info["_final_observation"]), done), ("_final_observation", t)


def engine_state(b, fields=("board", "piece", "stats", "mt")):
    """A copy of a batch's (or a vector env's engine's) state."""
    return {k: v.copy() for k, v in getattr(b, "engine", b).get_state(fields).items()}


def raw_state(b):
    """The state as it lies in device memory, padding envs and both MT
    generation buffers included, read without st_mt_sync: the read changes
    nothing (previews and generations in progress stay as they are)."""
    t = getattr(b, "engine", b).state_tensors(("board", "piece", "stats", "mt"), sync=False)
    return {k: v.cpu().numpy() for k, v in t.items()}


def assert_same_state(a, b, what="", fields=("board", "piece", "stats", "mt")):
    """Two states field by field; a and b are snapshots (dicts of arrays or
    tensors) or engines, read through engine_state(fields)."""
    a, b = (x if isinstance(x, dict) else engine_state(x, fields) for x in (a, b))
    assert len(a) > 0 and sorted(a) == sorted(b), (sorted(a), sorted(b), what)
    for k in a:
        assert np.array_equal(_np(a[k]), _np(b[k])), (k, what)


def check_engine_state(b, exp, what="final"):
    """Board, piece word and counter rows 0..12 against packed_state()."""
    st = getattr(b, "engine", b).get_state(("board", "piece", "stats"))
    assert np.array_equal(st["board"], exp["board"]), (what, "board")
    assert np.array_equal(st["piece"], exp["piece"]), (what, "piece")
    assert np.array_equal(st["stats"][:13], exp["stats"]), (what, "counters")


def set_mt_state(ob, mt, index):
    """MT19937 words [n, 624] and index [n] into every env of an oracle batch."""
    rng = np.ctypeslib.as_array(ob.envs)["rng"]
    rng["mt"][:], rng["index"][:] = mt, index


def check_mt_state(b, ob, what=""):
    """The engine's MT19937 words and index of every env (st_mt_sync:
    CPython's exact state) against the oracle batch's."""
    st = getattr(b, "engine", b).get_state(("mt", "stats"))
    rng = np.ctypeslib.as_array(ob.envs)["rng"]
    assert np.array_equal(st["stats"][13], rng["index"]), ("MT index", what)
    assert np.array_equal(st["mt"], rng["mt"]), ("MT words", what)


def check_bench_dump(path, n_global, steps):
    """bench.py's C5 region (ST_BENCH_DUMP): rank 0's assembled outputs of the
    last timed step -- gathered from every rank -- against the oracle stepping
    all n_global envs through the same `steps` action rows (seeds 1000 + e,
    the bench's splitmix64 actions keyed by the global index)."""
    z = np.load(path)
    assert int(z["n_global"]) == n_global and int(z["step"]) == steps - 1
    orc = ParallelOracle(n_global, {})
    try:
        if steps > 1:
            orc.rollout(0, steps - 1, obs=False)
        ref = orc.rollout(steps - 1, 1)
    finally:
        orc.close()
    check_step(ref, 0, z["obs"], z["reward"], z["done"], at=steps - 1)
    return z


# ------------------------------------------------------------------ the surface loop
def drive_surface(target, ref, surface, acts, on_step=None):
    """One step surface over every row of acts, each step checked against
    ref: st_step ("step": host actions, its own ungated instantiation;
    "gated": a device tensor, which TetrisBatch.step gates), st_step_f32
    ("f32"), st_step_wire + st_unwire ("wire") on a TetrisBatch, or
    st_step_vec with final_obs and info on a TetrisVecEnv ("vec").  acts
    [T, n] is passed as it is -- a numpy array or a device tensor selects
    another kernel instantiation, so the caller chooses.  on_step(t) runs
    after step t's checks."""
    assert surface in ("step", "gated", "f32", "wire", "vec"), surface
    assert surface != "gated" or not isinstance(acts, np.ndarray)
    from gym_simpletetris_amd.engine import unwire
    b = getattr(target, "engine", target)
    W, H = b.width, b.height
    for t in range(len(acts)):
        done = ref["done"][t].astype(bool)
        robs = ref["obs"][t]
        if surface == "vec":
            obs, rew, dn, info = target.step(acts[t])
            check_final_observation(info, robs, done, t)
            check_info(info, ref["stats"][t], done, t)
            robs = np.where(done[:, None], 0, robs)  # the reset convention
        elif surface == "wire":
            obs, rew, dn = unwire(b.step_wire(acts[t]), W, H)
        elif surface == "f32":
            f32, rew, dn = b.step(acts[t], obs="f32")
            check_f32(f32, robs, H, t)
            obs = b.obs
        else:
            obs, rew, dn = b.step(acts[t], obs="packed")
        check_step(ref, t, obs, rew, dn, robs)
        if on_step:
            on_step(t)
