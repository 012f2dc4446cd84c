"""Random call sequences across MT19937 generation ends against the C oracle.

The step kernels keep per-env state the reference cannot see, packed into the
upper bits of the MT index word and the second half of each MT row: two
generation buffers and the bit that selects the live one, the successor's
build progress, a preview piece drawn one spawn ahead with the words its draw
consumed.  Every kernel that spawns, draws, syncs, saves, forks or resets reads
and leaves that word, whatever kernel wrote it last.  The other modules test
each transition from a fresh seed or a host-written state; here one context
takes a seeded random sequence of all of them (sequence_ref.make_ops), with
its envs starting just short of a generation end, so that each kernel meets
the half-built successors and the previews the others left behind.

After every op: the op's outputs against the model, and board, piece word and
counter rows 0..12 against the oracle, read without st_mt_sync so that the
check itself gives no preview back and restarts no successor.  A read-only op
leaves the raw state (padding envs, both MT buffers, the MT index word)
bit-equal; st_next_piece and st_policy_lookahead, which may draw a preview,
leave everything but the MT rows and the MT index word bit-equal and the saved
state byte-equal.  At a checkpoint the whole MT19937 state is the oracle's.
test_cpu_call_sequences.py holds the conditions the sequences meet.

A failure names (config, seed, op number, op, field) and prints the ops up to
it; run_sequence(cid, seed, upto=k) replays a prefix.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import sequence_ref as SR
from harness import (check_final_observation, check_info, check_mt_state, check_step, check_steps, engine, raw_state)

pytestmark = pytest.mark.gpu

CASES = [(cid, seed) for cid in SR.CONFIGS for seed in SR.CONFIGS[cid]["seeds"]]
EDGE = 256  # 10x20_two_wave: the per-op state check reads the first and the last EDGE envs


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _eq(a, b, *what):
    assert np.array_equal(a, b), what


class Eng:
    """The engine side of sequence_ref.run: the context under test (a
    TetrisVecEnv's engine), the spare the hand-over ops move to, a scratch
    context for saves that must not touch the one under test and, where the
    config has one, the fork source with another lock_delay."""

    def __init__(self, m):
        G = engine()
        from gym_simpletetris_amd import _lib as C
        self.C, self.m, self.cfg = C, m, m.cfg
        n, kw = m.n, m.kw
        self.W, self.H = kw["width"], kw["height"]
        same = not m.none
        self.venvs = [G.TetrisVecEnv(n, seed=base, obs_format="packed", autoreset=same, validate_actions=True, **kw)
                      for base in (m.seed_base, m.seed_base + SR.SPARE_SEEDS)[:1 if m.sp is None else 2]]
        auto = m.cfg["autoreset"]
        self.scratch = G.TetrisBatch(n, autoreset=auto, seeds=range(n), **kw)
        self.alt = None
        self.k = self.op = None
        self.complete = self.incomplete = 0
        try:
            for v in self.venvs:
                v.reset()
            self.scratch.reset()
            if m.alt is not None:
                self.alt = G.TetrisBatch(n, autoreset=auto, seeds=[m.seed_base + SR.ALT_SEEDS + e for e in range(n)],
                                         **m.alt_kw)
                self.alt.reset()
                for a in SR.ALT_ACTS:
                    self.alt.step(np.full(n, a, np.uint8))
            # the start indices, as test_gpu_next_piece.py::test_generation_boundary writes them
            st = self.b.get_state(("stats", "mt"))
            st["stats"][13] = m.start
            self.b.set_state(stats=st["stats"], mt=st["mt"])
            check_mt_state(self.b, m.ob, "start")
            self.rec = torch.empty(self.b._L.st_export_words(self.W, self.H), dtype=torch.int32, device=self.b.device)
        except BaseException:
            self.close()
            raise

    @property
    def b(self):
        return self.venvs[0].engine

    def close(self):
        for v in self.venvs:
            v.close()
        for b in (self.scratch, self.alt):
            if b is not None:
                b.close()

    def _dev(self, a):
        return torch.as_tensor(np.ascontiguousarray(a), device=self.b.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.b.device).cuda_stream)

    def _row13(self):
        return self.b.state_tensors(("stats",), sync=False)["stats"][13, :self.m.n].cpu().numpy().view(np.uint32)

    # ------------------------------------------------------------ the interpreter's calls
    def begin(self, k, op):
        self.k, self.op = k, op
        if op[0] in SR.STEPPING:
            self.p0 = (self._row13() >> 10) & 0x3FF  # the successor's progress, for the coverage print alone

    def step(self, op, acts, ref):
        b, kind, W, H = self.b, op[0], self.W, self.H
        if kind == "step":      # host actions: the ungated kernel
            check_step(ref, 0, *b.step(acts[0]), at=kind)
        elif kind == "gated":   # a device tensor: st_gate_actions in front
            check_step(ref, 0, *b.step(self._dev(acts[0])), at=kind)
        elif kind == "f32":
            check_step(ref, 0, *b.step(self._dev(acts[0]), obs="f32"), H=H, at=kind)
        elif kind == "wire":
            from gym_simpletetris_amd.engine import unwire
            check_step(ref, 0, *unwire(b.step_wire(self._dev(acts[0])), W, H), at=kind)
        elif kind == "vec":
            obs, rew, dn, info = self.venvs[0].step(self._dev(acts[0]))
            done, robs = ref["done"][0].astype(bool), ref["obs"][0]
            if not self.m.none:  # (without auto-reset the vector env has no final observation and the
                # info of a dead env is the reference's own: the obs, reward and done rows are checked)
                check_final_observation(info, robs, done, kind)
                check_info(info, ref["stats"][0], done, kind)
                robs = np.where(done[:, None], 0, robs)  # the reset convention
            check_step(ref, 0, obs, rew, dn, robs, at=kind)
        elif kind == "step_export":
            self.C.check(b._L.st_step_export(b._ctx, _P(self._dev(acts[0])), op[2], op[3], _P(self.rec), _P(b.obs),
                                             _P(b.reward), _P(b.done), self._stream()))
            check_step(ref, 0, b.obs, b.reward, b.done, at=kind)
        elif kind == "step_n":  # the last step's outputs
            check_step(ref, len(acts) - 1, *b.step_n(self._dev(acts)), at=kind)
        elif kind == "rollout":
            check_steps(ref, *b.rollout(self._dev(acts)))
        else:
            raise ValueError(kind)

    def placements(self, row, ref):
        slots = np.full(self.m.n, -1, np.int64)
        slots[:self.m.m] = row
        check_step(ref, 0, *self.b.step_placements(slots), at="placements")
        _eq(self.b.placed.cpu().numpy()[:self.m.m], ref["placed"], "placed")

    def reset(self, mask):
        self.b.reset(self._dev(mask.astype(np.uint8)))

    def form(self, op, index=None, mask=None):
        b, kind, spare = self.b, op[0], self.venvs[-1].engine
        if kind == "sync_mt":
            b.sync_mt()
        elif kind == "save_load":
            b.load(b.save())
        elif kind == "get_set_state":  # CPython's form through the host: the progress restarts at 0
            st = b.get_state(("stats", "mt"))
            b.set_state(stats=st["stats"], mt=st["mt"])
        elif kind in ("fork_self", "fork_self_keep_rng"):
            b.fork(None, None, mask, keep_rng=kind == "fork_self_keep_rng")
        elif kind == "handover_load":
            spare.load(b.save())
            self.venvs.reverse()
        elif kind == "fork_handover":
            spare.fork(b)
            spare.fork(b, index=index, mask=mask)
            self.venvs.reverse()
        elif kind == "fork_alt":
            b.fork(self.alt, index=index, mask=mask, keep_rng=True)
        else:
            raise ValueError(kind)

    def _saved(self):
        """save() of a deep copy: the save's own sync stays off the context under test."""
        self.scratch.fork(self.b)
        return self.scratch.save()

    def read(self, op, m):
        from gym_simpletetris_amd.engine import BCTS_WEIGHTS
        b, kind, C = self.b, op[0], self.C
        drawing = kind in SR.DRAWING_READS
        refused = kind in SR.REACH_KINDS and max(b.lock_delay, 0) > SR.REACH_MAX_LOCK
        snap = self._saved() if drawing else None
        raw0 = raw_state(b)
        if kind == "next_piece":
            _eq(b.next_piece().cpu().numpy(), SR.next_pieces(m.ob), "next_piece")
        elif kind == "next_weights":
            _eq(b.next_weights().cpu().numpy(), SR.next_weights_ref(m.ob), "next_weights")
        elif kind == "render":
            _eq(b.render_packed().cpu().numpy().view(np.uint32).T, SR.render_ref(m.ob), "render")
        elif kind == "afterstates_set":
            b.afterstates(features="bcts")
        elif kind == "policy_linear_set":
            b.policy_linear(BCTS_WEIGHTS, features="bcts")
        elif kind == "policy_expect":
            b.policy_expect(BCTS_WEIGHTS, features="bcts")
        elif kind == "policy_lookahead":
            b.policy_lookahead(BCTS_WEIGHTS, features="bcts")
        elif kind == "export_env":
            C.check(b._L.st_export_env(b._ctx, op[1], _P(b.obs), _P(b.reward), _P(b.done), op[2], _P(self.rec),
                                       self._stream()))
        elif kind in SR.REACH_KINDS:
            slots = np.random.default_rng(op[1]).integers(-2, m.S + 2, m.n)
            calls = [lambda: b.routes(slots)] if kind == "routes" \
                else [lambda: b.reachable(), lambda: b.route_actions(slots)]
            for call in calls:
                if refused:  # ST_EINVAL and no state change
                    with pytest.raises(C.StError) as err:
                        call()
                    assert err.value.code == C.ST_EINVAL, ("ST_EINVAL", err.value.code)
                else:
                    call()
        else:
            raise ValueError(kind)
        torch.cuda.synchronize(b.device)
        raw1 = raw_state(b)
        for f in raw0:
            if drawing and f == "mt":
                continue
            rows = [r for r in range(raw0[f].shape[0]) if not (drawing and f == "stats" and r == 13)] \
                if f == "stats" else slice(None)
            _eq(raw0[f][rows], raw1[f][rows], "raw " + f, "changed by a read-only call")
        if drawing:
            assert self._saved() == snap, ("save()", "changed by the call")

    def checkpoint(self, m):
        check_mt_state(self.b, m.ob, "checkpoint")

    def end(self, k, op, m):
        n = m.n
        st = {f: v.cpu().numpy()[..., :n] for f, v in
              self.b.state_tensors(("board", "piece", "stats"), sync=False).items()}
        exp = m.ob.packed_state()
        sel = slice(None) if n <= 2 * EDGE else np.r_[0:EDGE, n - EDGE:n]
        _eq(st["board"].view(np.uint32)[:, sel], exp["board"][:, sel], "board", "after the op")
        _eq(st["piece"].view(np.uint32)[sel], exp["piece"][sel], "piece", "after the op")
        _eq(st["stats"][:13][:, sel], exp["stats"][:, sel], "counters", "after the op")
        if op[0] in SR.STEPPING:
            crossed = m.log[-1]["crossed"]
            self.complete += int((crossed & (self.p0 == SR.MT_N)).sum())
            self.incomplete += int((crossed & (self.p0 < SR.MT_N)).sum())


def run_sequence(cid, seed, upto=None):
    """The sequence of (config, seed), or its first `upto` ops, on the engine
    and the model; returns (crossings that found the successor complete,
    crossings that found it incomplete), read from the engine's own word and
    so printed, never asserted."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ops = SR.make_ops(cid, seed)[:upto]
    m = SR.Model(cid, seed, cus)
    eng = Eng(m)
    try:
        SR.run(ops, m, eng)
    except AssertionError as e:
        print(f"{cid} seed {seed}: the ops up to the failing one")
        for k, op in enumerate((ops + [("checkpoint",)])[:eng.k + 1]):
            print(f"  {k}: {op}")
        raise AssertionError(f"config {cid}, seed {seed}, op {eng.k} {eng.op}: {e.args}") from e
    finally:
        eng.close()
    return eng.complete, eng.incomplete


@pytest.mark.parametrize("cid,seed", CASES)
def test_call_sequence(cid, seed):
    t0 = time.perf_counter()
    complete, incomplete = run_sequence(cid, seed)
    print(f"call sequence {cid} seed {seed}: crossings with the successor complete {complete}, "
          f"incomplete {incomplete}; {time.perf_counter() - t0:.1f} s")
