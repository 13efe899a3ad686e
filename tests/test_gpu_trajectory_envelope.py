"""Trajectory parity at every step: each step-kernel instance against the fp64 oracle over steps
1 .. 120 of random-action flight, held to the oracle's own fp32-storage divergence and the
observation's number format -- no fixed tolerance (tests/fp32_envelope.py: dense, check):

    p99_hip[t, c] <= 3 * E[t, c] + F[t, c]      for every step t and frame component c,

p99 over the lanes still running on both sides; E the p99 of the oracle against itself with its
fp32-stored state rounded every step or every frame, or moved by one fp32 ulp (four seeds, and the
quaternion at every frame); F four fp32 spacings of the component's largest value.
tests/test_fp32_envelope_cpu.py shows on the CPU what this bound rejects (a 1e-5 error of dt and
a dropped J2 term at step 1, a 1e-4 elevator gain by step 4) and that the oracle alone passes it
(held-out seeds at most 0.94 of the bound, on the edge lanes).

1 024 lanes, the same actions on both sides (the oracle's sample_actions stream, recorded by the
oracle run), goals and ICs of tests/fp32_envelope.py's workloads. One case per step-kernel
instance, each asserting the instance it launched. The flight-envelope edge lanes of
tests/test_gpu_envelope.py are held per group over 30 steps, with exact done flags. The fused
and persistent rollout kernels are held bit-identical to these step kernels elsewhere
(test_fused_rollout_step_equals_sample_step_add, test_persistent_rollout_matches_fused_steps).
With $F16_TRAJ_ENVELOPE_JSON set, every case's ratios are written there
(profiles/trajectory_envelope.json)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fp32_envelope as fe  # noqa: E402
from parity_tools import FRAME_NAMES  # noqa: E402

_CASES = {}


@pytest.fixture(scope="module")
def torch_mod(gpu):
    import torch
    yield torch
    path = os.environ.get("F16_TRAJ_ENVELOPE_JSON")
    if path and _CASES:
        with open(path, "w") as f:
            json.dump({"test": "tests/test_gpu_trajectory_envelope.py", "factor": fe.FACTOR,
                       "floor": "%g fp32 spacings of the component's largest reference value (angles: at 2 pi)"
                                % fe.FLOOR_ULPS,
                       "bound": "p99_hip[t, c] <= factor * E[t, c] + F[t, c] at every step; ratio = p99_hip / bound",
                       "cases": _CASES}, f, indent=1)


def _hip_trajectory(torch, d, want_kernel, stack_k=4, **env_kw):
    """(frames (steps, n, 12) float64, done (steps, n) bool) of F16Envs on the workload of d."""
    from f16_jsb_amd.env import F16Envs
    w = d.workload
    su = fe.setup(w)
    g = F16Envs(w.n, stack_k=stack_k, **dict(su["env_kw"], **env_kw))
    try:
        g.reset(goals=torch.as_tensor(su["goals"]), ic=su["ic"])
        acts = torch.as_tensor(np.array(d.actions), device=g.device)  # (a writable copy)
        frames = torch.zeros((w.steps, w.n, 12), dtype=torch.float32, device=g.device)
        done = torch.zeros((w.steps, w.n), dtype=torch.uint8, device=g.device)
        for t in range(w.steps):
            out = g.step(acts[t])
            frames[t] = out.obs[:, -1, :12]
            done[t] = out.terminated | out.truncated
        assert g.step_kernel_name == want_kernel, g.step_kernel_name
        return frames.cpu().numpy().astype(np.float64), done.cpu().numpy() != 0
    finally:
        g.close()


def _record(name, kernel, d, rep):
    per_group = {}
    for g, (gname, idx) in enumerate(d.groups):
        r = np.nan_to_num(rep.ratio[g])
        t_of = r.argmax(axis=0)
        rows = {}
        for t in fe.RECORD_STEPS:
            if t <= d.workload.steps and rep.lanes[g, t - 1]:
                rows[str(t)] = {"lanes": int(rep.lanes[g, t - 1]), "hip": rep.p99[g, t - 1].tolist(),
                                "E": d.E[g, t - 1].tolist(), "F": d.F[g, t - 1].tolist()}
        per_group[gname] = {"lanes_at_start": len(idx), "lanes_at_end": int(rep.lanes[g, -1]),
                            "worst_ratio": {nm: float(r[t_of[c], c]) for c, nm in enumerate(FRAME_NAMES[:12])},
                            "worst_step": {nm: int(t_of[c]) + 1 for c, nm in enumerate(FRAME_NAMES[:12])},
                            "raw": rows}
    _CASES[name] = {"kernel": kernel, "workload": d.workload._asdict(), "components": FRAME_NAMES[:12],
                    "worst": dict(zip(("ratio", "group", "step", "component", "lane"), rep.worst)),
                    "groups": per_group}


def _case(torch, name, w, want_kernel, exact_done=False, **env_kw):
    d = fe.dense(w)
    frames, done = _hip_trajectory(torch, d, want_kernel, **env_kw)
    if exact_done:  # a lane's flags count up to and including its first done
        before = np.vstack([np.ones((1, w.n), bool), fe.running(d.done)[:-1]])
        bad = np.argwhere(before & (done != d.done))
        assert not len(bad), "%s: done flags differ first at (step %d, lane %d)" % (name, bad[0][0] + 1, bad[0][1])
    rep = fe.check(d, frames, done)
    _record(name, want_kernel, d, rep)
    print("%s (%s): worst ratio %.3g at (group %s, t %d, %s, lane %d); %d lanes at the end" % (
        (name, want_kernel) + rep.worst + (int(rep.lanes[:, -1].sum()),)))
    assert rep.lanes[:, 0].min() > 0 and rep.lanes[:, -1].sum() >= w.n // 2, rep.lanes[:, -1]
    fe.assert_within(d, frames, done, "%s (%s)" % (name, want_kernel))


@pytest.mark.parametrize("down_sample", [4, 2, 1])
def test_contiguous(torch_mod, down_sample):
    _case(torch_mod, "contiguous_ds%d" % down_sample, fe.Workload(down_sample=down_sample), "f16_step_kernel")


@pytest.mark.parametrize("order", ["position", "env"])
def test_window(torch_mod, order):
    """The bench layout (position-major frame histories) and the env-major order."""
    _case(torch_mod, "window_%s_major" % order, fe.Workload(), "f16_step_win_nt_kernel<0, 1, false>",
          obs_layout="window", window_order=order)


def test_k10_global_tables(torch_mod):
    _case(torch_mod, "k10", fe.Workload(), "f16_step_gt_kernel<0, false>", stack_k=10)


def test_two_waves_per_simd(torch_mod, monkeypatch):
    """The 256-register build, forced at this size as tests/test_gpu_window.py does."""
    monkeypatch.setenv("F16ENV_OCC", "2")
    _case(torch_mod, "occ2", fe.Workload(), "f16_step_var_kernel<0, 2, false>")


def test_cfg5_window(torch_mod):
    _case(torch_mod, "cfg5_window", fe.Workload(cfg5=True), "f16_step_win_nt_kernel<3, 1, false>", obs_layout="window")


def test_cfg5_two_waves_per_simd(torch_mod, monkeypatch):
    monkeypatch.setenv("F16ENV_OCC", "2")
    _case(torch_mod, "cfg5_occ2", fe.Workload(cfg5=True), "f16_step_var_kernel<3, 2, false>")


def test_steady_wind_without_gusts(torch_mod):
    """Wind through the reset IC's wind columns on both sides: the wind kernels, no gust draw."""
    _case(torch_mod, "steady_wind", fe.Workload(wind=True), "f16_step_var_kernel<2, 1, false>")


@pytest.mark.parametrize("cfg5", [False, True], ids=["reference_task", "cfg5_wind"])
def test_flight_envelope_edges(torch_mod, cfg5):
    """tests/test_gpu_envelope.py's lanes (stratosphere, supersonic, alpha / beta outside the
    tables, inverted attitudes, the crash floor), p99 per group of 256 lanes over 30 steps; a lane
    leaves at its first done, and the done flags agree exactly."""
    w = fe.edge_workload(cfg5)
    d = fe.dense(w)
    _case(torch_mod, "edges_cfg5_wind" if cfg5 else "edges", w,
          "f16_step_var_kernel<3, 1, false>" if cfg5 else "f16_step_kernel", exact_done=True)
    # the edges were really visited, and lanes crashed
    assert d.done[:8].any() and (d.frames[-1, :, 2] > 11000.0).sum() > 50 and (d.frames[-1, :, 3] > 1.2).sum() > 50
