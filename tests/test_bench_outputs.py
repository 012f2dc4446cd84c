"""bench.py's plain run and --dump-outputs.

One plain `bench.py --gpus 1 --obs f32 --dump-outputs DIR` run (2,051 envs: not
a multiple of the 64-env workgroup; 3 warm-up + 12 timed steps) is shared by
the GPU tests: its result line holds the headline and none of the --full legs,
and the dumped arrays -- the output buffers after the last timed step -- equal
the oracle's step 14 of the same seeds and action stream, so two builds run
with the same arguments can be compared array for array.  The sampling of an
output above the byte budget is checked on the host.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from harness import ParallelOracle, check_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, WU, K, W, H = 2051, 3, 12, 10, 20


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench") / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", str(WU), "--n-envs", str(N), "--obs", "f32", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


@pytest.mark.gpu
def test_plain_run_measures_the_headline_only(plain_run):
    d, _ = plain_run
    assert d["steps"] == K and d["warmup"] == WU and d["full"] is False
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["ms_per_step"] > 0
    # value and ms_per_step are the same K timed steps
    assert d["value"] == pytest.approx(N * 1e3 / d["ms_per_step"], rel=1e-9)
    for leg in ("variants", "cpu_baseline", "debug", "step_no_gather"):
        assert leg not in d
    assert "steady" not in d["roofline"]


@pytest.mark.gpu
def test_dumped_outputs_equal_the_oracle(plain_run):
    _, out = plain_run
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["done", "obs", "obs_f32", "reward"]
    assert got["obs_f32"].dtype == np.float32
    assert all(got[k].dtype == np.float64 for k in ("obs", "reward", "done"))
    assert sum(a.nbytes for a in got.values()) <= 64 * 1000 * 1000
    orc = ParallelOracle(N, {})
    try:
        orc.rollout(0, WU + K - 1, obs=False)
        ref = orc.rollout(WU + K - 1, 1)
    finally:
        orc.close()
    assert np.array_equal(got["reward"], ref["reward"][0].astype(np.float64))
    assert np.array_equal(got["done"], ref["done"][0].astype(np.float64))
    assert got["obs"].shape == (W, N)
    assert np.array_equal(got["obs"].T, ref["obs"][0].astype(np.float64))
    check_f32(got["obs_f32"], ref["obs"][0], H, WU + K - 1)  # [n][W][H]


def test_dump_outputs_samples_above_the_budget(tmp_path, monkeypatch):
    """An output above the byte budget is written as one fixed sample of envs
    (the same columns of every array, ascending, indices in env_index.npy),
    identical from call to call."""
    import bench
    n = 1000
    obs = torch.arange(W * n, dtype=torch.int32).reshape(W, n)
    rew = torch.arange(n, dtype=torch.int32) - 5
    done = (torch.arange(n) % 3 == 0)
    f32 = torch.arange(n * W * H, dtype=torch.float32).reshape(n, W, H)
    arrs = {"obs": (obs, 1), "reward": (rew, 0), "done": (done, 0), "obs_f32": (f32, 0)}
    per_env = W * 8 + 8 + 8 + W * H * 4
    monkeypatch.setattr(bench, "DUMP_BUDGET", 300 * (per_env + 8))
    shapes = bench.dump_outputs(str(tmp_path / "a"), arrs)
    bench.dump_outputs(str(tmp_path / "b"), arrs)
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == ["done", "env_index", "obs", "obs_f32", "reward"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(x.nbytes for x in a.values()) <= 300 * (per_env + 8)
    idx = a["env_index"].astype(np.int64)
    assert len(idx) == 300 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert shapes["obs"] == [W, 300] and shapes["obs_f32"] == [300, W, H]
    assert np.array_equal(a["obs"], obs.numpy()[:, idx].astype(np.float64))
    assert np.array_equal(a["reward"], rew.numpy()[idx].astype(np.float64))
    assert np.array_equal(a["done"], done.numpy()[idx].astype(np.float64))
    assert np.array_equal(a["obs_f32"], f32.numpy()[idx])
    # under the budget: every env, no index file
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64 * 1000 * 1000)
    assert "env_index" not in bench.dump_outputs(str(tmp_path / "c"), arrs)
    assert np.array_equal(np.load(tmp_path / "c" / "obs.npy"), obs.numpy().astype(np.float64))
