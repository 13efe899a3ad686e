"""State parity: every field the device carries against the fp64 oracle after one step.

The other physics tests see the HIP step through the 12 observed quantities of the newest frame.
Here both sides start from the same planted corner states (tests/state_corners.py: actuators
far from / within a frame of / on their targets and at their clamps, TEF on every segment of its
traverse in waves that skip it, mix it and never skip it, PID integrators saturating and small,
every airspeed / alpha / Mach switch on either side, N2 around its target and in the nn clamp,
the four augmentor transitions), take the same actions, and the whole canonical state is compared
field by field:

    err <= 3 * (the oracle's own divergence when started one fp32 ulp away) + floor

per unguarded lane (state_corners.check_state; floor: 4 fp32 ulps at the field's range, counted
from the operations for the few fields at the end of longer fp32 chains, state_corners.floors; a lane is guarded when a switch input comes within
1e-3 of its threshold at some frame, at most 2 % of lanes: tests/test_state_corners_cpu.py). Flags
and integer bookkeeping are compared exactly on every lane. With $F16_STATE_PARITY_JSON set, each
case's ratio table is written there (profiles/state_parity.json)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import state_corners as sc  # noqa: E402
from state_corners import LX, NAMES  # noqa: E402

from f16_jsb_amd.abi import F16_OBS_DIM, F16C_EPA_C, F16C_EPA_S, F16C_GUST, F16L_VC_KTS  # noqa: E402

N = sc.N_LANES
_TABLES = {}


@pytest.fixture(scope="module")
def torch_mod(gpu):
    import torch
    yield torch
    path = os.environ.get("F16_STATE_PARITY_JSON")
    if path and _TABLES:
        with open(path, "w") as f:
            json.dump({"test": "tests/test_gpu_state_parity.py", "lanes": N, "factor": sc.FACTOR,
                       "bound": "err <= factor * envelope[field] + floor[field]; ratio = max over unguarded lanes "
                                "of err / bound (exact fields: 1 if any lane differs)",
                       "cases": _TABLES}, f, indent=1)


def _assert_planted(got, s):
    """get_state before the step returns what set_state was given: exact, except the fields the
    canonical form re-encodes (calibrated airspeed, relative 1e-6; the Earth angle's cos / sin)
    and the latch entries recomputed at load; fields the device does not carry read 0."""
    want = sc.device_roundtrip(s)
    vc = LX + F16L_VC_KTS
    enc = [F16C_EPA_C, F16C_EPA_S, vc] + sc.RECOMPUTED
    keep = [c for c in range(s.shape[1]) if c not in enc]
    bad = [NAMES[c] for c in keep if not np.array_equal(got[:, c], want[:, c])]
    assert not bad, "set_state / get_state changed %s" % bad
    np.testing.assert_allclose(got[:, vc], s[:, vc], rtol=1e-6, atol=0)
    np.testing.assert_allclose(got[:, [F16C_EPA_C, F16C_EPA_S]], s[:, [F16C_EPA_C, F16C_EPA_S]], rtol=0, atol=1e-12)
    # recomputed from the stored state exactly as a frame computes them: fp32 round-off away
    # from the oracle's stored latch (body rates rad/s, ground speed relative)
    np.testing.assert_allclose(got[:, sc.RECOMPUTED[:3]], s[:, sc.RECOMPUTED[:3]], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, sc.RECOMPUTED[3]], s[:, sc.RECOMPUTED[3]], rtol=1e-5, atol=0)


def _case(torch, name, kind, down_sample, want_kernel, steps=1, skip=(), **env_kw):
    from f16_jsb_amd.env import F16Envs
    s, a, groups = sc.planted(kind)
    ref, pre, mask, env = sc.oracle_case(kind, down_sample, steps)
    k = env_kw.pop("stack_k", 4)
    g = F16Envs(N, stack_k=k, seed=sc.SEED, down_sample=down_sample, cfg5=kind == "cfg5", **env_kw)
    try:
        g.reset(goals=sc.far_goals(N))
        g.set_state(np.array(s))  # (a writable copy: the shared planted state is read-only)
        g.set_obs(np.zeros((N, k, F16_OBS_DIM), np.float32))
        assert g.step_kernel_name == want_kernel, g.step_kernel_name
        _assert_planted(g.get_state().cpu().numpy(), s)
        act = torch.as_tensor(np.ascontiguousarray(a), device=g.device)
        for _ in range(steps):
            out = g.step(act)
            assert int(out.terminated.sum()) == 0 and int(out.truncated.sum()) == 0
        got = g.get_state().cpu().numpy()
    finally:
        g.close()
    rep = sc.check_state(got, ref, env, mask, frames=down_sample * steps, steps=steps, skip=skip,
                         not_carried_zero=True)
    _TABLES[name] = {"kernel": want_kernel, "down_sample": down_sample, "steps": steps,
                     "guarded_lanes": int(mask.sum()), "groups": sc.group_ratios(rep),
                     "fields": {f: v for f, v in rep.items() if f != "failed"}}
    worst = sorted(((v["ratio"], f) for f, v in rep.items() if f != "failed"), reverse=True)[:8]
    print("%s: worst ratios %s" % (name, ", ".join("%s %.3g" % (f, r) for r, f in worst)))
    msg = ["%s: err %.3e bound %.3e, %s" % (f, rep[f]["err"], rep[f]["bound"], sc.describe(groups, rep[f]["lane"]))
           for f in rep["failed"] if f in rep]
    assert not rep["failed"], "%s (%s): fields over their bound: %s\n%s" % (name, want_kernel, rep["failed"],
                                                                         "\n".join(msg))


@pytest.mark.parametrize("down_sample", [1, 2, 4])
def test_contiguous(torch_mod, down_sample):
    _case(torch_mod, "contiguous_ds%d" % down_sample, "plain", down_sample, "f16_step_kernel")


@pytest.mark.parametrize("down_sample", [1, 4])
def test_window_bench_layout(torch_mod, down_sample):
    _case(torch_mod, "window_ds%d" % down_sample, "plain", down_sample, "f16_step_win_nt_kernel<0, 1, false>",
          obs_layout="window")


@pytest.mark.parametrize("down_sample", [1, 4])
def test_steady_wind_on_half_the_lanes(torch_mod, down_sample):
    """set_state with wind switches the handle to the wind kernels (tests/test_gpu_state.py)."""
    _case(torch_mod, "wind_ds%d" % down_sample, "wind", down_sample, "f16_step_var_kernel<2, 1, false>")


def test_cfg5_two_waves(torch_mod, monkeypatch):
    """The cfg5 handle's two-waves-per-SIMD instance (forced at this size, as test_gpu_window.py
    does). The gust itself is tests/test_gpu_cfg5.py's: every field but F16C_GUST."""
    monkeypatch.setenv("F16ENV_OCC", "2")
    _case(torch_mod, "cfg5_ds4", "cfg5", 4, "f16_step_var_kernel<3, 2, false>",
          skip=tuple(range(F16C_GUST, F16C_GUST + 3)))


def test_k10_global_tables(torch_mod):
    _case(torch_mod, "k10_ds4", "plain", 4, "f16_step_gt_kernel<0, false>", stack_k=10)


def test_two_steps_without_reinjection(torch_mod):
    """The second step reads the state and latch the STEP kernel stored, not set_state's; guard
    and envelope over all eight frames."""
    _case(torch_mod, "two_steps_ds4", "plain", 4, "f16_step_kernel", steps=2)
