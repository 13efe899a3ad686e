"""bench.py's side legs: the cfg4 rollout leg runs green at a small size with
the MLP policy in the loop and the deferred bootstrap, and a failing leg keeps the headline line
but is named in `legs_failed` and makes bench.py exit non-zero."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--envs", "4096", "--rollout-envs", "2048", "--rollout-steps", "32", "--policy-steps", "16",
         "--burn-in", "8", "--no-cpu-baseline"]


@pytest.mark.gpu
def test_rollout_leg_small(gpu, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *SMALL])
    args = bench.parse()
    r = bench.rollout_bench(args, gpu, 0, 1)
    assert "error" not in r
    assert r["rollout_env_steps_per_s"] > 0 and r["rollout_fused_steps_env_steps_per_s"] > 0
    pol = r["policy_in_the_loop"]
    assert pol["steps"] == 16 and np.isfinite(pol["env_steps_per_s"]) and pol["env_steps_per_s"] > 0
    assert "deferred" in pol["policy"]
    assert np.isfinite(pol["bootstrap_per_step"]["env_steps_per_s"])
    assert 0 < r["gae_kernel_ms"] and r["gather_s"] is None


def _bench(extra, timeout=900):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2", *SMALL, *extra],
                       capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    return p, (json.loads(lines[-1]) if lines else None)


@pytest.mark.gpu
def test_plain_run_has_the_headline_only_and_dumps_its_last_step(gpu, tmp_path):
    """Without --full the line carries the headline and none of the side legs (--fail-leg finds no
    leg to fail); --dump-outputs writes the StepOut of the last timed step, the same from run to run."""
    dumps = []
    for name in ("a", "b"):
        p, d = _bench(["--fail-leg", "rollout", "--dump-outputs", str(tmp_path / name)])
        assert p.returncode == 0, p.stderr[-3000:]
        assert d["full"] is False and d["steps"] == 5 and d["warmup"] == 2
        assert d["value"] > 0 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(4096 / (d["ms_per_step"] * 1e-3), rel=1e-2)
        assert d["legs_failed"] == []
        for k in ("features", "telemetry", "sampler", "rollout", "sb3_compat", "cfg2", "persistent_random_policy",
                  "cfg1_hip", "layouts", "cpu_baseline"):
            assert k not in d, k
        dumps.append({f: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))})
    a, b = dumps
    assert sorted(a) == [f + ".npy" for f in ("ep_len", "ep_return", "obs", "rew", "terminal_obs", "terminated",
                                              "truncated")]
    assert a["obs.npy"].shape == a["terminal_obs.npy"].shape == (4096, 4, 15) and a["obs.npy"].dtype == np.float32
    assert a["ep_return.npy"].dtype == np.float64 and a["rew.npy"].shape == (4096,)
    assert np.isfinite(a["obs.npy"]).all() and np.any(a["obs.npy"] != 0) and np.any(a["rew.npy"] != 0)
    for f in a:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)


@pytest.mark.gpu
def test_forced_leg_failure_exits_nonzero(gpu):
    p, d = _bench(["--full", "--fail-leg", "rollout"])  # --full: the side legs run only there
    assert p.returncode == 1, p.stderr[-3000:]
    assert d is not None, "the headline line must still be printed"
    assert d["legs_failed"] == ["rollout"]
    assert "forced failure" in d["rollout"]["error"]
    assert d["value"] > 0 and d["n_gpus"] == 1
