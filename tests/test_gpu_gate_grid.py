"""The action gate (validate_actions=True) above one block, and every gated
step kernel.  k_gate_actions reduces n actions to one answer over up to 64
blocks of B = 4,096 actions per pass (S = 64 B per grid pass); the gated
k_step instantiations leave at their early return when the answer is "bad".
tests/test_gpu_streams_gate.py stops at n = 2,048: one block.  All of this
is integer work: every comparison is bit-exact.

What each test is the only cover for:

* test_gate_answer_every_grid_shape -- k_gate_actions with 2, 4 and 64
  blocks and with a second grid-stride pass, at the C ABI: the cross-block
  counter words[1] and its reset by the last block, the epoch tag words[2]
  written by one block and read by another, the last block's publication of
  words[0] and the host word, the scalar tail behind the 16-byte loads, and
  the all-scalar path of a misaligned action pointer (a slice at byte
  offset 1 or 15).  A clean call follows every bad one, so a counter that
  was not reset or a tag that leaked shows as a wrong or missing answer.
* test_gate_multiblock_rejects_and_stays_in_lockstep -- the same grid behind
  TetrisBatch.step and TetrisVecEnv.step (both copy modes) at n = S + B + 5:
  a rejected step changes no env whichever block saw the bad byte, the
  device-side 255 sentinel of a non-uint8 tensor at this size, and the clean
  steps in between equal an unvalidated twin's.
* test_gated_step_kernels_vs_oracle -- the gated k_step instantiations with
  a rejected launch in the run (the early return behind barrier B0):
  <10,20,F32?,false,false,true> (scoring flags) and the runtime-size
  <0,0,F32?,false,false,true>, with null vector outputs (TetrisBatch.step)
  and with final_obs / info (TetrisVecEnv), at n = 200 (a last workgroup of 8
  real envs: the index clamp and the masked stores), against the C oracle.
* test_gate_covers_only_first_of_step_n -- st_step_n with an armed gate:
  only the first of the k launches carries the gate.
* test_copy_false_rejection_keeps_two_step_lifetime -- TetrisVecEnv's
  copy=False alternation across rejected steps (the outputs of the last
  successful step live for two successful steps), and the copy=True pool
  across a run of rejections.
"""
import ctypes

import numpy as np
import pytest
import torch

from harness import (C4, assert_same_state, check_final_observation, check_info, check_step,
                     engine as _engine, engine_state)
from oracle import oracle as O

pytestmark = pytest.mark.gpu

B = 4096     # actions per block and pass: 256 threads x 16
S = 64 * B   # actions per grid pass: at most 64 blocks
NBIG = S + B + 5
vp = ctypes.c_void_p


def _positions(n):
    """Indices that land in the first block, on a block edge, in a middle
    block, on the last action, and -- where n reaches them -- on the last lane
    of the grid's first pass and in the second pass of blocks 0 and 1."""
    pos = [0, B - 1, B, 31 * B + 123, n - 1]
    if n >= S:
        pos.append(S - 1)
    if n > S:
        pos += [S, S + B]
    return sorted({p for p in pos if 0 <= p < n})


@pytest.mark.parametrize("n", [B + 1, 3 * B + 1, S, S + 1, NBIG])
def test_gate_answer_every_grid_shape(n):
    """st_gate_actions + st_gate_wait (no step) on one context per n: the
    answer equals (bytes > 6).any() of the very bytes passed, for one byte of
    6 / 7 / 255 at every position of _positions(n), with the action pointer
    16-byte aligned and (n = B + 1 and S + B + 5) at byte offsets 1 and 15;
    every other call is clean and must answer 0.  n = S + B + 5 adds 24
    random cases of 0..3 bad bytes."""
    G = _engine()
    eng = G.TetrisBatch(n, seeds=range(n), validate_actions=False)
    eng.reset()  # (only owns a context of n envs: no step is launched)
    L, ctx = eng._L, eng._ctx
    s = vp(torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(n + 16, dtype=torch.uint8, device=eng.device)

    def ask(view):
        """(the gate's answer, the answer the bytes passed call for)"""
        assert L.st_gate_actions(ctx, vp(view.data_ptr()), s) == 0
        got = L.st_gate_wait(ctx)
        a = view.cpu().numpy()
        return got, int((a > 6).any())

    offs = (0, 1, 15) if n in (B + 1, NBIG) else (0,)
    fill = (torch.arange(n, device=eng.device) % 7).to(torch.uint8)
    for off in offs:
        view = buf[off:off + n]
        assert view.data_ptr() % 16 == off
        view.copy_(fill)
        for pos in _positions(n):
            for val in (6, 7, 255):
                assert ask(view) == (0, 0), ("clean", n, off, pos, val)
                view[pos] = val
                got, want = ask(view)
                assert want == int(val > 6)
                assert got == want, (n, off, pos, val)
                view[pos] = pos % 7
        assert ask(view) == (0, 0), ("clean", n, off)
    if n == NBIG:
        rng = np.random.default_rng(0)
        cases = []
        for _ in range(24):
            k = int(rng.integers(0, 4))
            cases.append((rng.integers(0, n, size=k), rng.integers(7, 256, size=k)))
        # the draw keeps its point whatever the seed: clean cases among the
        # bad ones, and bad bytes that different blocks find in the same call
        assert sum(len(p) == 0 for p, _ in cases) >= 4
        assert sum(len({int(x) % S // B for x in p}) >= 2 for p, _ in cases) >= 4
        for i, (pos, vals) in enumerate(cases):
            view = buf[offs[i % 3]:offs[i % 3] + n]
            view.copy_(fill)
            assert ask(view) == (0, 0), ("clean before fuzz case", i)
            for p_, v_ in zip(pos, vals):
                view[int(p_)] = int(v_)
            got, want = ask(view)
            assert want == int(len(pos) > 0)
            assert got == want, ("fuzz case", i, pos, vals)
    eng.close()


def _bad_batches(good, n):
    """Rejected batches in turn: one bad byte in the first block, a middle
    block, the last block, the second pass and the scalar tail; then an int64
    tensor holding -1 (the 255 sentinel is set on the device)."""
    out = []
    for pos, val in ((0, 7), (31 * B + 123, 9), (S - 1, 255), (S, 200), (n - 1, 7)):
        x = good.clone()
        x[pos] = val
        out.append(x)
    x = good.to(torch.int64)
    x[S + B + 2] = -1
    out.append(x)
    return out


@pytest.mark.parametrize("kind", ["engine", "vec-copy", "vec-nocopy"])
def test_gate_multiblock_rejects_and_stays_in_lockstep(kind):
    """n = S + B + 5 (64 blocks, two passes, a 5-byte scalar tail): clean and
    rejected calls alternate.  A rejected call raises KeyError and leaves
    board, piece and stats as they were (compared on the device); every clean
    call equals an unvalidated twin's; at the end the whole state, MT words
    included, equals the twin's."""
    G = _engine()
    n = NBIG
    if kind == "engine":
        a = G.TetrisBatch(n, seeds=range(n), autoreset="same_step", validate_actions=True)
        b = G.TetrisBatch(n, seeds=range(n), autoreset="same_step", validate_actions=False)
        ea, eb, calls = a, b, 12
    else:
        copy = kind == "vec-copy"
        a = G.TetrisVecEnv(n, seed=21, obs_format="packed", validate_actions=True, copy=copy)
        b = G.TetrisVecEnv(n, seed=21, obs_format="packed", validate_actions=False, copy=copy)
        ea, eb, calls = a.engine, b.engine, 8
    a.reset()
    b.reset()
    bads = None
    fields = ("board", "piece", "stats")
    for c in range(calls):
        good = eb.gen_actions(c, 3).clone()
        if c % 2 == 0:
            ra, rb = a.step(good), b.step(good)
            for x, y in zip(ra[:3], rb[:3]):
                assert torch.equal(x, y), c
            if kind != "engine":
                for k in ("time", "score", "final_observation"):
                    assert torch.equal(ra[3][k], rb[3][k]), (k, c)
            del ra, rb
            continue
        if bads is None:
            bads = _bad_batches(good, n)
        bad = bads[c // 2]
        before = ea.state_tensors(fields)  # (st_mt_sync first)
        # the twin syncs where `a` does: st_mt_sync restarts the build of the
        # next MT generation, and the last comparison takes the raw MT tensor,
        # the engine's half-built successor buffers included
        eb.sync_mt()
        with pytest.raises(KeyError):
            a.step(bad)
        after = ea.state_tensors(fields)
        for k in fields:
            assert torch.equal(before[k], after[k]), (k, c)
        del before, after
    fields = ("board", "piece", "stats", "mt")
    sa, sb = ea.state_tensors(fields), eb.state_tensors(fields)
    for k in fields:
        assert torch.equal(sa[k], sb[k]), k
    del sa, sb
    a.close()
    b.close()


ODD = dict(width=9, height=15, lock_delay=2, step_reset=True, penalise_height=True, penalise_holes=True,
           reward_step=True)
EXTREME = dict(advanced_clears=True, penalise_height=True, penalise_holes_increase=True)


@pytest.mark.parametrize("api,kw,obs", [
    ("batch", dict(width=10, height=20, **C4), "packed"),
    ("batch", dict(width=10, height=20, **C4), "f32"),
    ("batch", ODD, "packed"),
    ("batch", ODD, "f32"),
    ("batch", dict(width=4, height=4, **EXTREME), "packed"),
    ("batch", dict(width=32, height=28, **EXTREME), "packed"),
    ("vec", dict(width=10, height=20, **C4), "f32"),
    ("vec", ODD, "packed"),
], ids=["10x20-c4-packed", "10x20-c4-f32", "9x15-packed", "9x15-f32", "4x4-packed", "32x28-packed",
        "vec-10x20-c4-f32", "vec-9x15-packed"])
def test_gated_step_kernels_vs_oracle(api, kw, obs):
    """150 gated steps of n = 200 envs (device uint8 actions, same-step
    auto-reset) against the C oracle: reward, done and obs of every step
    (float32 obs: equal to the conversion of the packed obs as well); a batch
    with one action 9 ahead of steps 40 and 110 raises KeyError, changes
    neither board, piece, stats nor MT state, and the oracle -- which never saw
    it -- still agrees on every later step.  'vec': TetrisVecEnv, the same
    kernels with final_obs and info, in gym's reset convention."""
    G = _engine()
    n, T, base, aseed = 200, 150, 7, 99
    w, h = kw["width"], kw["height"]
    seeds = [base + e for e in range(n)]
    ob = O.OracleBatch(n, seeds, **kw)
    ob.reset()
    acts = O.splitmix64_actions(aseed, 0, T, n)
    ref = ob.rollout(acts)
    if api == "batch":
        env = eng = G.TetrisBatch(n, autoreset="same_step", seeds=seeds, validate_actions=True, **kw)
    else:
        env = G.TetrisVecEnv(n, seed=base, obs_format=obs, validate_actions=True, **kw)
        eng = env.engine
    env.reset()
    dev = eng.device
    for t in range(T):
        a = eng.gen_actions(t, aseed)
        assert a.dtype == torch.uint8 and np.array_equal(a.cpu().numpy(), acts[t])
        if t in (40, 110):
            bad = a.clone()
            bad[n - 1 if t == 40 else 64] = 9  # the last, partly filled workgroup; a full one
            before = engine_state(eng)
            with pytest.raises(KeyError):
                env.step(bad, obs=obs) if api == "batch" else env.step(bad)
            assert_same_state(before, eng, t)
        done = ref["done"][t].astype(bool)
        robs = ref["obs"][t]  # [n][W]: the terminal obs where done
        if api == "batch":
            o, r, d = env.step(a, obs=obs)
            if obs == "f32":
                assert torch.equal(o, eng.obs_to_f32(eng.obs)), ("f32 obs", t)
            check_step(ref, t, eng.obs if obs == "f32" else o, r, d)
        else:
            o, r, d, info = env.step(a)
            f32 = h if obs == "f32" else None
            check_step(ref, t, o, r, d, np.where(done[:, None], 0, robs), H=f32)  # the reset convention
            check_final_observation(info, robs, done, t, H=f32)
            check_info(info, ref["stats"][t], done, t)
    if w * h == 16:
        assert ref["done"].sum() > n  # a 4x4 board: resets and spawns into a full board all along
    env.close()


def test_gate_covers_only_first_of_step_n():
    """C ABI: st_gate_actions, then st_step_n with k = 3, then st_gate_wait.
    A gate that saw a bad batch skips the first launch only (the twin takes
    two plain steps); a clean gate skips nothing (three steps); an ungated
    st_step afterwards is an ordinary step."""
    G = _engine()
    n = 256
    a = G.TetrisBatch(n, seeds=range(n), autoreset="same_step", validate_actions=False)
    b = G.TetrisBatch(n, seeds=range(n), autoreset="same_step", validate_actions=False)
    a.reset()
    b.reset()
    L, ctx = a._L, a._ctx
    s = vp(torch.cuda.current_stream().cuda_stream)
    o = torch.empty((10, n), dtype=torch.int32, device=a.device)
    r = torch.empty(n, dtype=torch.int32, device=a.device)
    d = torch.empty(n, dtype=torch.uint8, device=a.device)

    def step_n(acts):
        ptrs = (vp * len(acts))(*[x.data_ptr() for x in acts])
        assert L.st_step_n(ctx, ctypes.addressof(ptrs), len(acts), vp(o.data_ptr()), None, vp(r.data_ptr()),
                           vp(d.data_ptr()), s) == 0

    def same_as_twin(out, what):
        ob, rb, db = out
        torch.cuda.synchronize()
        assert torch.equal(o, ob) and torch.equal(r, rb) and torch.equal(d.bool(), db.bool()), what
        assert_same_state(a, b, what)

    acts = [b.gen_actions(t, 5).clone() for t in range(7)]
    bad = acts[0].clone()
    bad[n - 1] = 7
    assert L.st_gate_actions(ctx, vp(bad.data_ptr()), s) == 0
    step_n(acts[0:3])
    assert L.st_gate_wait(ctx) == 1
    b.step(acts[1])
    same_as_twin(b.step(acts[2]), "bad gate: two of three steps")
    assert L.st_gate_actions(ctx, vp(acts[3].data_ptr()), s) == 0
    step_n(acts[3:6])
    assert L.st_gate_wait(ctx) == 0
    b.step(acts[3])
    b.step(acts[4])
    same_as_twin(b.step(acts[5]), "clean gate: three steps")
    assert L.st_step(ctx, vp(acts[6].data_ptr()), vp(o.data_ptr()), vp(r.data_ptr()), vp(d.data_ptr()), s) == 0
    same_as_twin(b.step(acts[6]), "ungated step after both")
    a.close()
    b.close()


def test_copy_false_rejection_keeps_two_step_lifetime():
    """copy=False: the outputs of a step are overwritten two successful steps
    later.  Outputs kept (not cloned) across one rejected step, and across
    two in a row, still hold their step after the next successful step, and
    the step after that writes the same memory; the env stays in lockstep with
    an unvalidated twin.  copy=True: ten rejections in a row, then ten clean
    steps with nothing held, keep the pool at two slots at the most and reuse
    one every step."""
    G = _engine()
    n = 512
    for rejections in (1, 2):
        v = G.TetrisVecEnv(n, seed=9, obs_format="packed", copy=False, validate_actions=True)
        u = G.TetrisVecEnv(n, seed=9, obs_format="packed", copy=False, validate_actions=False)
        v.reset()
        u.reset()

        def both(t):
            acts = u.engine.gen_actions(t, 4).clone()
            rv, ru = v.step(acts), u.step(acts)
            for x, y in zip(rv[:3], ru[:3]):
                assert torch.equal(x, y), t
            for k in ("time", "score", "final_observation"):
                assert torch.equal(rv[3][k], ru[3][k]), (k, t)
            return rv

        for t in range(3):
            both(t)
        obs, rew, done, info = both(3)
        score = info["score"]  # a view of the slot's info rows
        want = [x.clone() for x in (obs, rew, done, score, info["time"])]
        bad = u.engine.gen_actions(50, 4).clone()
        bad[n // 2] = 7
        for _ in range(rejections):
            with pytest.raises(KeyError):
                v.step(bad)
        nxt = both(4)
        torch.cuda.synchronize()
        for got, w_ in zip((obs, rew, done, score, info["time"]), want):
            assert torch.equal(got, w_), rejections
        assert nxt[0].data_ptr() != obs.data_ptr()
        del nxt
        third = both(5)  # two successful steps later: the slot of step 3 again
        assert third[0].data_ptr() == obs.data_ptr() and third[1].data_ptr() == rew.data_ptr()
        both(6)
        del third, obs, rew, done, info, score
        v.close()
        u.close()
    v = G.TetrisVecEnv(n, seed=9, obs_format="packed", validate_actions=True)
    v.reset()
    bad = v.engine.gen_actions(50, 4).clone()
    bad[0] = 255
    for _ in range(10):
        with pytest.raises(KeyError):
            v.step(bad)
    assert len(v._pool) <= 2
    seen = [v.slots_reused]
    for t in range(10):
        v.step(v.engine.gen_actions(t, 4))
        seen.append(v.slots_reused)
    assert len(v._pool) <= 2
    assert all(y > x for x, y in zip(seen, seen[1:])), seen
    v.close()
