"""The host side of the facades' numpy mode on CPU (f16_jsb_amd/host_staging.py, vec_env.py) over the
stand-in handles of tests/fake_envs.py: the host window mirror (_HostWindow) against a dense
handle -- the K-1 fill of lanes a step reset, the FRESH fill of lanes the previous step reset, host
ring restarts, a masked reset between two steps -- the facade contracts over both staging classes,
copy_obs=True, the shared helpers and the old import path of the facades."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import integration_checks as C
from fake_envs import FakeEnvs, FakeWindowEnvs
from f16_jsb_amd.buffers import split_step_flags, step_flags_bytes
from f16_jsb_amd.env import reference_goal
from f16_jsb_amd.host_staging import _HostStaging, _HostWindow
from f16_jsb_amd.vec_env import F16GymVectorEnv, F16VecEnv, seeded_goals


def _act(n, t):
    return np.full((n, 4), 0.25 * (t % 4), np.float32)


@pytest.mark.parametrize("k,th,max_steps", [(4, 11, 6), (1, 5, 6), (3, 7, 3), (10, 23, 6)])
def test_host_window_follows_dense_handle(k, th, max_steps):
    """_HostWindow beside the fake's own dense arrays: the observation of every step, the terminal
    observation of the lanes it finished, and the observation of the step before, which the next
    step must leave alone."""
    n = 7
    fake = FakeWindowEnvs(n, k, max_steps=max_steps)
    host = _HostWindow(fake, th=th)
    np.testing.assert_array_equal(host.reset_obs(fake.reset()), fake.obs.numpy())
    ended = restarts = 0
    prev = None
    for t in range(40):
        q = host.q
        out = fake.step(host.actions_to_device(_act(n, t)))
        obs, rew, term, trunc = host.step_outputs(out.obs)
        restarts += host.q <= q
        np.testing.assert_array_equal(obs, fake.obs.numpy(), err_msg="obs @%d" % t)
        np.testing.assert_array_equal(rew, fake.rew.numpy())
        idx = np.flatnonzero(term | trunc)
        np.testing.assert_array_equal(idx, np.flatnonzero((fake.term | fake.trunc).numpy()))
        if idx.size:
            tobs, eret, elen = host.done_rows(idx)
            np.testing.assert_array_equal(tobs, fake.terminal_obs.numpy()[idx], err_msg="terminal obs @%d" % t)
            np.testing.assert_array_equal(eret, fake.ep_return.numpy()[idx])
            np.testing.assert_array_equal(elen, fake.ep_len.numpy()[idx])
            ended += idx.size
        if prev is not None:
            np.testing.assert_array_equal(prev[0], prev[1], err_msg="previous obs changed @%d" % t)
        prev = (obs, obs.copy())
    assert ended >= n and restarts >= 1, (ended, restarts)


def test_masked_reset_with_a_fresh_fill_pending():
    """env_method("reset") on two lanes right after a step that finished lanes (lane 1 among them):
    the mirror takes the new windows whole and forgets the fill it owed."""
    n, k = 7, 4
    fake = FakeWindowEnvs(n, k, max_steps=5)
    venv = F16VecEnv(envs=fake)
    assert type(venv._host) is _HostWindow
    np.testing.assert_array_equal(venv.reset(), fake.obs.numpy())
    for t in range(25):
        if t == 5:
            assert 1 in venv._host.prev_reset  # (the odd lanes truncated at their fifth step)
            got = venv.env_method("reset", indices=[1, 4])
            for (o, info), i in zip(got, (1, 4)):
                np.testing.assert_array_equal(o, fake.obs.numpy()[i])
                assert info == {} and np.all(o == o[:1]) and fake.steps[i] == 0
        obs, rew, dones, infos = venv.step(_act(n, t))
        np.testing.assert_array_equal(obs, fake.obs.numpy(), err_msg="obs @%d" % t)
        for i in np.flatnonzero(dones):
            np.testing.assert_array_equal(infos[i]["terminal_observation"], fake.terminal_obs.numpy()[i])


# An observation of whole-copy staging lives in a ring of 3, so it outlasts two further steps, which
# the checks assert; the mirror promises one further step (the device layout's own guarantee), so under
# FakeWindowEnvs that one assertion of check_vecenv_contract is held to the promise: `keep`.
@pytest.mark.parametrize("fake_cls,staging,keep", [(FakeEnvs, _HostStaging, 2), (FakeWindowEnvs, _HostWindow, 1)])
def test_facade_contracts_over_both_stagings(fake_cls, staging, keep):
    C.check_vecenv_contract(fake_cls, staging, keep=keep)
    C.check_gym_vector_contract(fake_cls, staging)


@pytest.mark.parametrize("facade", [F16VecEnv, F16GymVectorEnv])
def test_copy_obs_hands_out_owned_arrays(facade):
    """copy_obs=True: what reset() and step() return belongs to the caller, reset()'s too."""
    n = 6
    env = facade(envs=FakeEnvs(n, 4, max_steps=6), copy_obs=True)
    assert type(env._host) is _HostStaging
    first = env.reset()
    first = first if isinstance(first, np.ndarray) else first[0]
    kept = [(first, first.copy())]
    for t in range(5):
        obs = env.step(_act(n, t))[0]
        kept.append((obs, obs.copy()))
    assert not (kept[0][1] == kept[-1][1]).all()
    h = env._host
    for a, snap in kept:
        np.testing.assert_array_equal(a, snap)
        assert not any(np.shares_memory(a, b.numpy()) for b in h.obs + [h.flags, h.act])


def test_seeded_goals():
    assert seeded_goals([None, None, None]) is None
    g = seeded_goals([5, None, 7, None])
    assert g.shape == (4, 3) and g.dtype == np.float32
    np.testing.assert_array_equal(g[0], reference_goal(5))
    np.testing.assert_array_equal(g[2], reference_goal(7))
    assert np.isnan(g[[1, 3]]).all()


@pytest.mark.parametrize("n", [1, 5, 16])
def test_split_step_flags(n):
    assert step_flags_bytes(n) == (6 * n + 15) // 16 * 16 and step_flags_bytes(n) % 16 == 0
    raw = np.random.default_rng(n).integers(0, 256, step_flags_bytes(n), dtype=np.uint8)
    for buf, f32 in ((raw, np.float32), (torch.from_numpy(raw), torch.float32)):
        rew, term, trunc = split_step_flags(buf, n, f32)
        want = (buf[:n * 4].view(f32), buf[n * 4:n * 5], buf[n * 5:n * 6])
        for got, w in zip((rew, term, trunc), want):
            assert got.dtype == w.dtype and tuple(got.shape) == (n,)
            np.testing.assert_array_equal(np.asarray(got).view(np.uint8), np.asarray(w).view(np.uint8))
        assert np.shares_memory(np.asarray(rew), raw) and np.shares_memory(np.asarray(trunc), raw)


def test_env_forwards_the_facades_and_nothing_private():
    import f16_jsb_amd.env as E
    from f16_jsb_amd import vec_env
    from f16_jsb_amd.env import F16GymEnv as G, F16GymVectorEnv as V, F16VecEnv as S
    assert (S, V, G) == (vec_env.F16VecEnv, vec_env.F16GymVectorEnv, vec_env.F16GymEnv)
    for name in ("_HostWindow", "_HostStaging", "_staging", "_ReadOnlyInfo", "make_gym_env"):
        with pytest.raises(AttributeError):
            getattr(E, name)
