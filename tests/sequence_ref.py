"""Random call sequences across MT19937 generation ends, in the oracle's terms:
the op generator, the model and the interpreter shared by
test_cpu_call_sequences.py (the model alone: conditions on the inputs) and
test_gpu_call_sequences.py (the engine beside it).  A plain module imported by
name, like fork_ref.py; it runs no engine code and needs no GPU.

The engine keeps per-env state the reference cannot see (two generation
buffers and the bit that selects one, the successor's build progress, a
preview drawn one spawn ahead), and every kernel reads and leaves it.  Here one
context takes a seeded random sequence of every such call, its envs starting
just short of a generation end, and the oracle takes the same sequence.

An op is a plain tuple (kind, args...).  Three groups:
  state-changing  the oracle steps or resets too; stepping ops consume rows of
                  one drop-heavy action stream (t0 = the first row);
  form-changing   the reference cannot see them: the model does nothing, or
                  moves its Env structs the way the engine moves its states;
  read-only       the state stays as it is, bit for bit.
`checkpoint` compares the whole MT19937 state (which syncs the engine's form).
The interpreter run() appends one more checkpoint behind the list, so that a
list made with a smaller n_ops is a prefix of a longer one.
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import fork_ref as FK
import placement_ref as P
from harness import C4
from oracle import oracle as O

MT_N, MT_WIN = 624, 16       # words of a generation; the draw window (kMtWin)
REACH_MAX_LOCK = 3           # ST_REACH_MAX_LOCK
EXTREME = dict(advanced_clears=True, penalise_height=True, penalise_holes_increase=True)  # test_gpu_gate_grid's
N_PLACED = 100               # envs that take random placement slots, as in test_gpu_prologue_draw's _handoffs
SEED0, SPARE_SEEDS, ALT_SEEDS = 770000, 50000, 90000
MI355X_CUS = 256             # the CPU test sizes 10x20_two_wave as the GPU test does on an MI355X

ONE_STEP = ("step", "gated", "f32", "wire", "vec", "step_export")
MULTI_STEP = ("step_n", "rollout")
STEPPING = ONE_STEP + MULTI_STEP + ("placements",)
STATE_KINDS = STEPPING + ("reset_mask",)
FORM_KINDS = ("sync_mt", "save_load", "handover_load", "get_set_state", "fork_self", "fork_self_keep_rng",
              "fork_handover", "fork_alt")
REACH_KINDS = ("reachable_route", "routes")
READ_KINDS = ("next_piece", "next_weights", "render", "afterstates_set", "policy_linear_set", "policy_expect",
              "export_env", "policy_lookahead") + REACH_KINDS
DRAWING_READS = ("next_piece", "policy_lookahead")  # may draw a preview: row 13 and the MT rows may move

# the bag one round of ops is drawn from, without replacement: every kind at
# least once a round, the stepping kinds more often
_BAG = {k: 5 for k in ONE_STEP}
_BAG.update(step_n=4, rollout=6, placements=4, reset_mask=2, checkpoint=3)
_BAG.update({k: 1 for k in FORM_KINDS[:-1] + READ_KINDS})

# id -> board, env count (None: two_wave_n), constructor kwargs, autoreset, op
# seeds, ops per sequence, the start index of lanes 0..3 of every wave, the
# range lanes 4..63 are spread over, and the largest placements run.  The
# start indices, seeds and op counts were tuned on the oracle alone until
# test_cpu_call_sequences.py's conditions held; see its docstring.
CONFIGS = {
    "10x20_c3": dict(board=(10, 20), n=70, kw={}, autoreset="same_step", seeds=(1, 2, 3), n_ops=132,
                     low=(600, 585, 565, 545), spread=(590, 624), place_k=3),
    "10x20_c4_none": dict(board=(10, 20), n=130, kw=C4, autoreset="none", seeds=(1, 2, 3), n_ops=160,
                          low=(610, 600, 590, 580), spread=(595, 624), place_k=3),
    "7x9_lock2": dict(board=(7, 9), n=70, autoreset="same_step", seeds=(1, 2, 3), n_ops=150,
                      kw=dict(lock_delay=2, step_reset=True, penalise_height=True, penalise_holes=True,
                              reward_step=True), low=(610, 600, 590, 580), spread=(600, 624), place_k=6,
                      bag=dict(placements=12)),
    "8x4_extreme": dict(board=(8, 4), n=70, kw=EXTREME, autoreset="same_step", seeds=(1, 2, 3), n_ops=132,
                        low=(600, 585, 565, 545), spread=(590, 624), place_k=3),
    "10x20_lock5": dict(board=(10, 20), n=70, kw=dict(lock_delay=5), autoreset="same_step", seeds=(1, 2, 3),
                        n_ops=150, low=(612, 606, 600, 594), spread=(604, 624), place_k=6,
                        bag=dict(placements=12, fork_alt=1), alt=dict(lock_delay=9)),
    "6x9_lockneg": dict(board=(6, 9), n=70, kw=dict(lock_delay=-2, penalise_holes_increase=True),
                        autoreset="same_step", seeds=(1, 2, 3), n_ops=132, low=(600, 585, 565, 545),
                        spread=(590, 624), place_k=3),
    "10x20_two_wave": dict(board=(10, 20), n=None, kw=C4, autoreset="same_step", seeds=(1,), n_ops=20,
                           low=(606, 606, 606, 606), spread=(606, 624), place_k=1, t_cap=40,
                           only=("step", "gated", "vec", "step_n", "rollout", "placements", "sync_mt",
                                 "fork_self_keep_rng", "next_piece", "render")),
}


def two_wave_n(cus):
    """The smallest n at which st_rollout launches k_rollout2 (test_handoffs_two_wave_rollout's)."""
    return 64 * 4 * cus + 1


def n_envs(cid, cus=MI355X_CUS):
    return CONFIGS[cid]["n"] or two_wave_n(cus)


def kinds(cid):
    """The op kinds of a config, by group: (state-changing, form-changing, read-only)."""
    bag = bag_of(cid)
    return tuple(tuple(k for k in grp if k in bag) for grp in (STATE_KINDS, FORM_KINDS, READ_KINDS))


def bag_of(cid):
    cfg = CONFIGS[cid]
    bag = dict(_BAG, **cfg.get("bag", {}))
    if cfg["autoreset"] == "none":  # the oracle's rollout resets on done: one-step ops only
        del bag["step_n"]
    if "only" in cfg:
        bag = {k: 1 for k in cfg["only"]}
    return bag


def drop_heavy(T, n, seed):
    """actions [T, n]: about half hard drops, the rest uniform over the seven
    actions, row by row (so a shorter stream is a prefix of a longer one)."""
    rng = np.random.default_rng(seed)
    out = np.empty((T, n), np.uint8)
    for t in range(T):
        out[t] = np.where(rng.random(n) < 0.5, 2, rng.integers(0, 7, n))
    return out


def start_indices(cid, n):
    """The CPython MT index of every env before op 0.  Lanes 0..3 of each wave
    start further back: the chunk builder serves the lowest incomplete lane
    first and needs 10 chunks per env, so their successor is complete before
    they cross.  The other lanes are spread up to 624 and cross from the first
    op on, against a successor that is not: the wave finishes it (mt_finish)."""
    cfg = CONFIGS[cid]
    lane = np.arange(n) % 64
    lo, hi = cfg["spread"]
    idx = lo + (np.maximum(lane, 4) - 4) * (hi - lo) // 59
    return np.where(lane < 4, np.array(cfg["low"])[np.minimum(lane, 3)], idx).astype(np.int32)


def make_ops(cid, seed, n_ops=None):
    """The op list of (config, seed): deterministic, printable, and a prefix
    of the list made with a larger n_ops."""
    cfg = CONFIGS[cid]
    n_ops = cfg["n_ops"] if n_ops is None else n_ops
    n = n_envs(cid)
    none = cfg["autoreset"] == "none"
    rng = np.random.default_rng(1000 * seed + sorted(CONFIGS).index(cid))
    names = sorted(bag_of(cid).items())
    ops, bag, t = [], [], 0

    def sub():
        return int(rng.integers(1 << 30))
    while len(ops) < n_ops:
        if not bag:
            bag = [k for k, c in names for _ in range(c)]
            rng.shuffle(bag)
            if not ops and "reset_mask" in bag:  # op 0: a masked reset while the last lanes stand at 624
                bag.remove("reset_mask")
                bag.append("reset_mask")
        kind = bag.pop()
        if kind in ("step", "gated", "f32", "wire", "vec"):
            op, k = (kind, t), 1
        elif kind == "step_n":
            k = int(rng.integers(2, 5))
            op = (kind, t, k)
        elif kind == "rollout":
            k = 1 if none else int(rng.integers(1, 10))
            op = (kind, t, k)
        elif kind == "step_export":
            op, k = (kind, t, int(rng.integers(n)), int(rng.integers(4))), 1
        elif kind == "placements":
            op, k = (kind, int(rng.integers(1, cfg["place_k"] + 1)), sub()), 0
        elif kind == "export_env":
            op, k = (kind, int(rng.integers(n)), int(rng.integers(4))), 0
        elif kind in ("reset_mask", "fork_self", "fork_self_keep_rng", "fork_handover", "fork_alt") + REACH_KINDS:
            op, k = (kind, sub()), 0
        else:
            op, k = (kind,), 0
        ops.append(op)
        t += k
        assert t <= cfg.get("t_cap", 512)
    return ops


def render_ref(ob):
    """TetrisEngine.render() (tetris_env.py:317-321) of every env as column
    words [n, W]: the board with the live piece set, clipped like _set_piece."""
    W, H = ob.cfg.width, ob.cfg.height
    env = np.ctypeslib.as_array(ob.envs)
    cells = ob.boards()[:, :W, :H].copy()
    e = np.arange(ob.n)
    for c in range(4):
        x, y = env["ax"] + env["shape"][:, c, 0], env["ay"] + env["shape"][:, c, 1]
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        cells[e[ok], x[ok], y[ok]] = 1
    return O.pack_cols(cells)


def next_weights_ref(ob):
    """st_next_weights [7, n]: 5 + max(counts) - counts[i] (tetris_env.py:186)."""
    c = ob.field("counts", (7,))
    return (5 + c.max(axis=1, keepdims=True) - c).T.astype(np.int32)


def next_pieces(ob):
    """lookahead_ref.next_pieces (st_next_piece: the shape the oracle's own
    clear() spawns on a byte copy of the env) with one copy of the whole Env
    array instead of one per env: 10x20_two_wave has 65,537 of them."""
    cp = type(ob.envs).from_buffer_copy(ob.envs)
    clear = O.lib().or_env_clear
    for i in range(ob.n):
        clear(ctypes.byref(cp[i]))
    return np.ctypeslib.as_array(cp)["shape_id"].astype(np.uint8)


def rollout_rows(ob, acts, lo=0, want_stats=True):
    """OracleBatch.rollout of the envs from `lo` on (acts [T, n - lo]); a large
    batch in contiguous slices, one host thread each, as harness.ParallelOracle
    does (ctypes releases the GIL)."""
    acts = np.ascontiguousarray(acts, np.uint8)
    T, n = acts.shape
    assert n == ob.n - lo
    out = dict(reward=np.zeros((T, n), np.int32), done=np.zeros((T, n), np.uint8),
               obs=np.zeros((T, n, ob.cfg.width), np.uint32),
               stats=np.zeros((T, n, 8), np.int32) if want_stats else None)
    parts = min(16, len(os.sched_getaffinity(0))) if n >= 4096 and hasattr(os, "sched_getaffinity") else 1
    bounds = np.linspace(0, n, parts + 1).astype(int)
    base, size = ctypes.addressof(ob.envs), ctypes.sizeof(O.Env)

    def one(k):
        a, b = int(bounds[k]), int(bounds[k + 1])
        part = {f: np.ascontiguousarray(v[:, a:b]) for f, v in out.items() if v is not None}
        O.lib().or_batch_rollout(base + (lo + a) * size, b - a, T, np.ascontiguousarray(acts[:, a:b]).ctypes.data,
                                 part["reward"].ctypes.data, part["done"].ctypes.data, part["obs"].ctypes.data,
                                 part["stats"].ctypes.data if want_stats else None)
        for f, v in part.items():
            out[f][:, a:b] = v
    if parts == 1:
        one(0)
    else:
        with ThreadPoolExecutor(parts) as pool:
            list(pool.map(one, range(parts)))
    return out


def _mask(sub, n, p=0.5):
    return np.random.default_rng(sub).random(n) < p


def fork_handover_args(sub, n):
    """(index, mask) of the permuting fork into the spare context: indices
    from -1 to n (both out of range: the env is left as it is), half masked."""
    rng = np.random.default_rng(sub)
    return rng.integers(-1, n + 1, n).astype(np.int32), rng.random(n) < 0.5


def fork_alt_args(sub, n):
    rng = np.random.default_rng(sub)
    return rng.integers(0, n, n).astype(np.int32), rng.random(n) < 0.3


def slots_of(sub, k, m, S):
    """Placement slots [k, m] in [-2, S + 2): valid, invalid and out of range."""
    return np.random.default_rng(sub).integers(-2, S + 2, (k, m))


ALT_ACTS = (2, 6, 6, 6, 6, 6, 6)  # a hard drop, then idling: the pieces rest with lock counters of 7


class Model:
    """The oracle side of one (config, seed): the context under test (`ob`),
    the spare one the hand-over ops move to (`sp`) and, where the config has
    one, the fork source with another lock_delay (`alt`); and the record the
    input conditions are read from."""

    def __init__(self, cid, seed, cus=MI355X_CUS):
        cfg = CONFIGS[cid]
        self.cid, self.seed, self.cfg = cid, seed, cfg
        self.n = n = n_envs(cid, cus)
        W, H = cfg["board"]
        self.kw = dict(cfg["kw"], width=W, height=H)
        self.seed_base = SEED0 + 1000 * seed
        self.ob = O.OracleBatch(n, [self.seed_base + e for e in range(n)], **self.kw)
        self.ob.reset()
        self.sp = None  # (only where an op moves to it)
        if {"handover_load", "fork_handover"} & set(bag_of(cid)):
            self.sp = O.OracleBatch(n, [self.seed_base + SPARE_SEEDS + e for e in range(n)], **self.kw)
            self.sp.reset()
        self.start = start_indices(cid, n)
        self.index()[:] = self.start
        self.alt = None
        if "alt" in cfg:
            self.alt_kw = dict(self.kw, **cfg["alt"])
            self.alt = O.OracleBatch(n, [self.seed_base + ALT_SEEDS + e for e in range(n)], **self.alt_kw)
            self.alt.reset()
            self.alt.rollout(np.repeat(np.array(ALT_ACTS, np.uint8)[:, None], n, axis=1))
        self.acts = drop_heavy(cfg.get("t_cap", 512), n, 7000 + seed)
        self.m = min(n, N_PLACED)
        self.S = 4 * (W + 6)
        self.none = cfg["autoreset"] == "none"
        # the record
        self.crossed = np.zeros(n, bool)
        self.log = []                  # per op: kind, envs that crossed in it, whether one was near the end
        self.deaths = self.dead_resets = self.env_steps = self.lock_pairs = 0
        self._locked = None

    def index(self, ob=None):
        return np.ctypeslib.as_array((ob or self.ob).envs)["rng"]["index"]

    def near_end(self):
        return bool((self.index() >= MT_N - MT_WIN).any())

    def _count(self, done, spawned):
        locked = (self.ob.field("counts", (7,)).sum(axis=1) != spawned) | (done != 0)
        if self._locked is not None:
            self.lock_pairs += int((locked & self._locked).sum())
            self.env_steps += self.n
        self._locked = locked
        self.deaths += int((done != 0).sum())

    def steps(self, t0, k):
        """k steps of the action stream from row t0, one oracle step at a time."""
        rows = []
        for t in range(t0, t0 + k):
            spawned = self.ob.field("counts", (7,)).sum(axis=1)
            r = rollout_rows(self.ob, self.acts[t:t + 1])
            self._count(r["done"][0], spawned)
            rows.append(r)
        return {f: np.concatenate([r[f] for r in rows]) for f in ("obs", "reward", "done", "stats")}

    def place(self, slots):
        """One placement step: slots [m] for the first m envs, slot -1 (the
        hard drop from where the piece is) for the rest."""
        ob, m, n = self.ob, self.m, self.n
        spawned = ob.field("counts", (7,)).sum(axis=1)
        rows = [P.ref_place_step(ob, i, slots[i], "same_step") for i in range(m)]  # (the oracle resets on done)
        ref = dict(obs=np.stack([r[0] for r in rows])[None], reward=np.array([r[1] for r in rows], np.int32)[None],
                   done=np.array([r[2] for r in rows], np.uint8)[None])
        if n > m:
            r2 = rollout_rows(ob, np.full((1, n - m), 2, np.uint8), lo=m, want_stats=False)
            ref = {f: np.concatenate([ref[f], r2[f]], axis=1) for f in ref}
        self._count(ref["done"][0], spawned)
        ref["placed"] = np.array([r[3] for r in rows], np.uint8)
        return ref

    def reset(self, mask):
        for i in np.flatnonzero(mask):
            self.ob.reset(int(i))
        if self._locked is not None:
            self._locked = self._locked & ~mask

    def swap(self):
        self.ob, self.sp = self.sp, self.ob
        self._locked = None

    def copy_all(self, dst, src):
        ctypes.memmove(dst.envs, src.envs, ctypes.sizeof(src.envs))


def run(ops, m, eng=None, note=None):
    """The ops on the model m and, beside it, on the engine adapter eng (None:
    the model alone).  eng's methods take what the model expects and assert it;
    note(k, op) runs before op k."""
    ops = list(ops) + [("checkpoint",)]
    for k, op in enumerate(ops):
        kind = op[0]
        if note:
            note(k, op)
        if eng:
            eng.begin(k, op)
        idx0, near = m.index().copy(), m.near_end()
        crossed = np.zeros(m.n, bool)

        def after_step(ref, j=0):
            nonlocal idx0
            idx1 = m.index()
            crossed[:] |= idx1 < idx0
            idx0 = idx1.copy()
            if m.none:  # the masked reset behind every step, as test_autoreset_off_masked_reset does
                dead = ref["done"][j] != 0
                if dead.any():
                    m.dead_resets += 1
                    if eng:
                        eng.reset(dead)
        if kind in ONE_STEP or kind in MULTI_STEP:
            t0, n_steps = op[1], (op[2] if kind in MULTI_STEP else 1)
            assert n_steps == 1 or not m.none
            ref = m.steps(t0, n_steps)
            if eng:
                eng.step(op, m.acts[t0:t0 + n_steps], ref)
            after_step(ref, n_steps - 1)
        elif kind == "placements":
            for row in slots_of(op[2], op[1], m.m, m.S):
                ref = m.place(row)
                if eng:
                    eng.placements(row, ref)
                after_step(ref)
        elif kind == "reset_mask":
            mask = _mask(op[1], m.n)
            m.reset(mask)
            crossed |= m.index() < idx0
            if eng:
                eng.reset(mask)
        elif kind in ("sync_mt", "save_load", "get_set_state"):
            if eng:
                eng.form(op)
        elif kind in ("fork_self", "fork_self_keep_rng"):
            mask = _mask(op[1], m.n, 0.5)  # the identity index: nothing the reference can see
            if eng:
                eng.form(op, mask=mask)
        elif kind == "handover_load":
            m.copy_all(m.sp, m.ob)
            if eng:
                eng.form(op)
            m.swap()
        elif kind == "fork_handover":
            index, mask = fork_handover_args(op[1], m.n)
            m.copy_all(m.sp, m.ob)  # the full identity fork first: every env of the spare is the context's
            FK.fork(m.sp, m.ob, index, mask)
            if eng:
                eng.form(op, index=index, mask=mask)
            m.swap()
        elif kind == "fork_alt":
            index, mask = fork_alt_args(op[1], m.n)
            FK.fork(m.ob, m.alt, index, mask, keep_rng=True)
            m._locked = None
            if eng:
                eng.form(op, index=index, mask=mask)
        elif kind in READ_KINDS:
            if eng:
                eng.read(op, m)
        elif kind == "checkpoint":
            if eng:
                eng.checkpoint(m)
        else:
            raise ValueError(kind)
        m.crossed |= crossed
        m.log.append(dict(kind=kind, crossed=crossed, near=near))
        if eng:
            eng.end(k, op, m)
    return m
