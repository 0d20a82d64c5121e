"""bench.py on the GPU at a small batch: a plain run is lean, --dump-outputs writes the last timed step's outputs, the
same arguments give the same arrays, and --full (whose self-check replays sampled envs on the C oracle) leaves
them unchanged."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--envs", "2048", "--max-steps", "60"]


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + ARGS + list(args), env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1, lines                       # stdout carries exactly the result line
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_full_and_dump(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    plain = _bench("--dump-outputs", a)
    full = _bench("--dump-outputs", b, "--full", "--no-cpu-baseline")
    for line in (plain, full):
        assert line["steps"] == 7 and line["warmup"] == 2
        assert line["unit"] == "agent-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["ms_per_step"] > 0 and line["value"] > 0
        # value = agent-steps of the 7 timed steps over their wall time
        units = line["config"]["live_agents_per_env_step"] * 7 * 2048
        assert abs(line["value"] - units / (7 * line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    # a plain run leaves out what takes runs of its own
    assert "check" not in plain and plain["cpu_baseline"] is None and plain["roofline"]["measured_peak"] is None
    assert full["check"]["ok"] and full["check"]["steps"] == 60 + 2 + 7
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"envs.npy", "view_g0.npy", "view_g1.npy", "feature_g0.npy", "feature_g1.npy", "actions.npy", "rewards.npy",
            "mean_action.npy", "ids_g0.npy", "pos_g0.npy", "hp_g0.npy", "agent_steps.npy", "stats.npy",
            "episode_return.npy", "group_num.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64), n
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), n
        total += x.nbytes
    assert total <= 64 << 20
    k = len(np.load(os.path.join(a, "envs.npy")))
    assert np.load(os.path.join(a, "view_g0.npy")).shape == (k, 128, 13 * 13 * 7)
    assert np.load(os.path.join(a, "actions.npy")).shape == (k, 2, 128)
    steps = np.load(os.path.join(a, "agent_steps.npy"))
    assert steps.shape == (2048, 1) and steps.min() > 0
