"""Which action check runs, and what a bad action does: validate_actions
(True / 'async' / False) x where the actions live x entry point.

Every batch has one entry outside value_action_map (tetris_env.py:152-160,
:245) at env 5 (row 1 of a [K, n] batch); each kind's all-good batch is the
control.  The engine under test runs beside a validate_actions=False twin
that is fed, as plain uint8 device tensors, only what the engine is expected
to have applied; outputs are compared bit for bit after every call and the
whole state at the end, so a rejected call that stepped anything shows up.

  input not on the engine's device (list, numpy, CPU tensor):
      KeyError from this call in every mode, nothing launched
      (rollout / step_n take tensors only: a list or numpy array is their
      ValueError, as before);
  device input, True:    KeyError from this call, no env stepped (step and
      the vector env's step through the action gate, the others by a sync);
  device input, 'async': the call returns, the bad env idles (action 6); the
      KeyError comes from check_actions() or from the next call, once;
  device input, False:   no error; the value acts as its uint8 cast does
      (9 and -1 -> 255 idle; 256 -> 0 and 2.5 -> 2 wrap into range).
"""
import numpy as np
import pytest
import torch

from harness import Foreign, assert_same_state, engine as _engine

pytestmark = pytest.mark.gpu

N, W, H, K = 70, 10, 20, 3  # one full wave and a ragged one
BAD_ENV, BAD_ROW = 5, 1
IDLE = 6


def _dev(dtype):
    return lambda a, dev: torch.as_tensor(a, device=dev).to(dtype)


# kind: (numpy dtype the batch is built in, the bad value, builder, on the
# device, what the bad value is after a plain uint8 cast (validate_actions=False))
KINDS = {
    "list": (np.int64, 9, lambda a, dev: a.tolist(), False, None),
    "numpy_int64": (np.int64, -1, lambda a, dev: a, False, None),
    "numpy_float32": (np.float32, 2.5, lambda a, dev: a, False, None),
    "cpu_int64": (np.int64, 263, lambda a, dev: torch.from_numpy(a), False, None),
    "dev_uint8": (np.uint8, 9, _dev(torch.uint8), True, IDLE),
    "dev_int64": (np.int64, 256, _dev(torch.int64), True, 0),
    "dev_int8": (np.int8, -1, _dev(torch.int8), True, IDLE),
    "dev_float32": (np.float32, 2.5, _dev(torch.float32), True, 2),
    "dlpack_uint8": (np.uint8, 9, lambda a, dev: Foreign(torch.as_tensor(a, device=dev)), True, IDLE),
}

ENTRIES = ("step", "step_wire", "rollout", "step_n", "vec_copy", "vec_nocopy")
TENSOR_ONLY = ("rollout", "step_n")   # a list / numpy batch is their ValueError
GATED = ("step", "vec_copy", "vec_nocopy")


def _make(entry, mode):
    G = _engine()
    if entry.startswith("vec"):
        e = G.TetrisVecEnv(N, width=W, height=H, seed=11, validate_actions=mode, copy=entry == "vec_copy")
        e.reset()
        return e
    e = G.TetrisBatch(N, width=W, height=H, seeds=range(11, 11 + N), autoreset="same_step", validate_actions=mode)
    e.reset()
    return e


def _call(entry, e, acts):
    """The entry point's outputs as a tuple of tensors."""
    if entry.startswith("vec"):
        obs, rew, done, info = e.step(acts)
        return obs, rew, done, info["time"], info["score"]
    out = getattr(e, entry)(acts)
    return (out,) if entry == "step_wire" else tuple(out)


def _same(entry, e, twin, acts, applied, what):
    got = _call(entry, e, acts)
    want = _call(entry, twin, torch.as_tensor(applied, device=twin.device))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (what, i)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("mode", [True, "async", False], ids=["True", "async", "False"])
def test_action_check_matrix(mode, entry):
    e, twin = _make(entry, mode), _make(entry, False)
    dev = twin.device
    rng = np.random.default_rng(2024)
    shape = (K, N) if entry in TENSOR_ONLY else (N,)
    at = (BAD_ROW, BAD_ENV) if entry in TENSOR_ONLY else (BAD_ENV,)
    checker = e.check_actions

    def fresh():
        return rng.integers(0, 7, size=shape).astype(np.uint8)

    for kind, (dt, bad_value, build, on_dev, cast) in KINDS.items():
        if entry in TENSOR_ONLY and kind in ("list", "numpy_int64", "numpy_float32"):
            bad = fresh().astype(dt)
            bad[at] = bad_value
            for a in (fresh().astype(dt), bad):  # good or bad: not a tensor either way
                with pytest.raises(ValueError):
                    _call(entry, e, build(a, dev))
            good = fresh()
            _same(entry, e, twin, torch.as_tensor(good, device=dev), good, (kind, "after"))
            continue
        # the control: an all-good batch of this kind (float 2.0 counts as 2)
        good = fresh()
        _same(entry, e, twin, build(good.astype(dt), dev), good, (kind, "control"))
        rounds = ("check_actions", "next_call") if (mode == "async" and on_dev) else ("once",)
        for via in rounds:
            good = fresh()
            bad = good.astype(dt)
            bad[at] = bad_value
            src = build(bad, dev)
            if not on_dev or mode is True:
                # refused by this call, before anything is launched (host
                # input; True by a sync) or with the step skipped (the gate)
                with pytest.raises(KeyError):
                    _call(entry, e, src)
            elif mode == "async":
                applied = good.copy()
                applied[at] = IDLE
                _same(entry, e, twin, src, applied, (kind, via, "bad applied as idle"))
                if via == "check_actions":
                    with pytest.raises(KeyError):
                        checker()
                else:  # the next call raises instead, and launches nothing
                    with pytest.raises(KeyError):
                        _call(entry, e, torch.as_tensor(fresh(), device=dev))
                checker()  # the flag is clear again
            else:
                applied = good.copy()
                applied[at] = cast
                _same(entry, e, twin, src, applied, (kind, "unchecked: acts as its uint8 cast"))
                checker()
            # the next good step equals the twin's: a refused call stepped nothing
            good = fresh()
            _same(entry, e, twin, torch.as_tensor(good, device=dev), good, (kind, via, "after"))
    assert_same_state(e, twin)
    e.close()
    twin.close()


@pytest.mark.parametrize("mode", [True, "async", False], ids=["True", "async", "False"])
def test_action_errors_that_are_not_key_errors(mode):
    """A complex tensor and a numpy string array are TypeErrors, a wrong
    element count a ValueError, in every mode and from host and device alike;
    none of them steps anything."""
    e, twin = _make("step", mode), _make("step", False)
    dev = e.device
    with pytest.raises(TypeError):
        e.step(torch.zeros(N, dtype=torch.complex64, device=dev))
    with pytest.raises(TypeError):
        e.step(torch.zeros(N, dtype=torch.complex64))
    with pytest.raises(TypeError):
        e.step(np.array(["1"] * N))
    for wrong in (np.zeros(N + 1, np.int64), [0] * (N - 1), torch.zeros(N + 1, dtype=torch.int64, device=dev),
                  torch.zeros(N - 1, dtype=torch.uint8, device=dev), torch.zeros((2, N), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            e.step(wrong)
        with pytest.raises(ValueError):
            e.step_wire(wrong)
    with pytest.raises(ValueError):
        e.rollout(torch.zeros((K, N + 1), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError):
        e.step_n(torch.zeros((0, N), dtype=torch.uint8, device=dev))
    good = np.arange(N) % 7
    _same("step", e, twin, torch.as_tensor(good, device=dev), good.astype(np.uint8), "after")
    assert_same_state(e, twin)
    e.close()
    twin.close()
