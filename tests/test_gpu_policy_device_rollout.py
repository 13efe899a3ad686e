"""collect_rollout's DevicePolicy fast path (values / log-probs written straight into the
buffer's rows, actions through one reused scratch) against the same policy driven through a
plain closure on the generic path: the same bits everywhere."""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

N, K, T, MAX_STEPS, SEED, STEP0 = 4097, 4, 12, 5, 21, 1000


def _policy(gpu):
    import bench
    from f16_jsb_amd.policy import DevicePolicy
    net = bench.MlpActorCritic(K * 15, "cpu", seed=2)
    dev = lambda layers: [(w.to(gpu), b.to(gpu)) for w, b in layers]  # noqa: E731
    # log_std = 1: samples with std e, so some leave the action Box
    return DevicePolicy.from_layers(dev(net.pi), dev(net.vf), dev([net.act_w])[0], dev([net.val_w])[0],
                                    torch.ones(4, device=gpu), stack_k=K, seed=SEED)


def _rollout(gpu, pol, mode, bootstrap, n=N, value_fn=None):
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.rollout import FIELDS, DeviceRolloutBuffer, collect_rollout
    envs = F16Envs(n, stack_k=K, device=gpu, seed=5, obs_layout="window", max_steps=MAX_STEPS)
    envs.reset()
    buf = DeviceRolloutBuffer(T, n, K, gpu)
    if mode == "fast":
        last_v, last_d = collect_rollout(envs, buf, SEED, STEP0, policy_fn=pol, value_fn=value_fn, bootstrap=bootstrap)
    else:
        calls = []

        def closure(obs):
            calls.append(1)
            return pol(obs, step=STEP0 + len(calls) - 1)
        last_v, last_d = collect_rollout(envs, buf, SEED, STEP0, policy_fn=closure, value_fn=pol.value,
                                         bootstrap=bootstrap)
        assert len(calls) == T
    buf.compute_returns_and_advantage(last_v, last_d)
    out = {f: getattr(buf, f).clone() for f in FIELDS}
    out["last_values"], out["last_dones"] = last_v.clone(), last_d.clone()
    envs.close()
    return out


@pytest.fixture(scope="module")
def rollouts(gpu):
    pol = _policy(gpu)
    return {(m, b): _rollout(gpu, pol, m, b) for m, b in (("fast", "deferred"), ("closure", "deferred"),
                                                         ("fast", "per_step"))}


def test_fast_path_equals_closure_on_the_generic_path(rollouts):
    a, b = rollouts[("fast", "deferred")], rollouts[("closure", "deferred")]
    assert set(a) == set(b)
    for f in a:
        assert torch.equal(a[f], b[f]), f
    # lanes truncated inside the rollout and bootstrapped (the rewards carry gamma * V)
    assert a["episode_starts"][1:].sum() > 0 and torch.all(torch.isfinite(a["returns"]))
    assert a["values"].abs().sum() > 0 and a["log_probs"].abs().sum() > 0


def test_deferred_bootstrap_equals_per_step(rollouts):
    a, b = rollouts[("fast", "deferred")], rollouts[("fast", "per_step")]
    for f in a:
        assert torch.equal(a[f], b[f]), f


def test_stash_over_the_byte_limit_falls_back_to_per_step(gpu, monkeypatch):
    """A deferred stash one byte over rollout.STASH_MAX_BYTES is not allocated: the collector
    bootstraps per step instead (V called T + 1 times: every step and the last values, where the
    stash needs at most two calls) and, DevicePolicy.value being batch-invariant, leaves the same
    bits as the unpatched deferred run and as an explicit per_step run. 257 envs: one full
    256-lane block and one lane; max_steps 5 < T, so every lane truncates inside the rollout."""
    from f16_jsb_amd import rollout
    n, pol, calls = 257, _policy(gpu), []

    def counted(obs):
        calls.append(1)
        return pol.value(obs)

    def run(bootstrap):
        del calls[:]
        return _rollout(gpu, pol, "fast", bootstrap, n=n, value_fn=counted), len(calls)
    deferred, n_deferred = run("deferred")
    per_step, n_per_step = run("per_step")
    stash_bytes = rollout.stash_capacity(n, T, MAX_STEPS) * K * 15 * 4
    monkeypatch.setattr(rollout, "STASH_MAX_BYTES", stash_bytes - 1)
    fallback, n_fallback = run("deferred")
    assert n_deferred <= 2 and n_per_step == T + 1 and n_fallback == T + 1
    assert deferred["episode_starts"][1:].sum() > 0  # (lanes did truncate: there was something to bootstrap)
    for f in fallback:
        assert torch.equal(fallback[f], deferred[f]), f
        assert torch.equal(fallback[f], per_step[f]), f


def test_stored_actions_are_the_unclipped_samples(rollouts):
    from f16_jsb_amd.rollout import np_clip_actions
    acts = rollouts[("fast", "deferred")]["actions"]
    assert (acts[..., :3].abs() > 1.0).any() and (acts[..., 3] < 0.0).any()
    assert not torch.equal(np_clip_actions(acts), acts)
