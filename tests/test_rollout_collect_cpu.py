"""collect_rollout's host logic on CPU: the path choice, the early argument checks, the fused path's
slot cursor and policy adaptor, and the deferred bootstrap's stash sizing. No launch: the pieces
under test hold no GPU call, and the fused driver is run against a stub that records what the raw
slot step is handed."""
from __future__ import annotations

import itertools
from types import SimpleNamespace

import pytest
import torch

from f16_jsb_amd import rollout
from f16_jsb_amd.abi import F16_FLAG_GUSTS, F16_FLAG_NO_AUTORESET, F16_SLOT_CLIP, RolloutSlot, config_default
from f16_jsb_amd.layouts import StepOut
from f16_jsb_amd.rollout import (DeviceRolloutBuffer, can_defer, choose_path, collect_rollout, slot_cursor,
                                 stash_capacity)

U64 = 2 ** 64 - 1
LAYOUTS = pytest.mark.parametrize("window", [False, True], ids=["contiguous", "window"])


# ---------------------------------------------------------------------------------------------------
# the slot cursor
@LAYOUTS
@pytest.mark.parametrize("clip", [False, True], ids=["random", "policy"])
def test_slot_cursor_points_the_slot_at_the_buffers_rows(window, clip):
    """T = 3, n = 5: every address the slot carries at step t is the buffer row's own data_ptr();
    act_step wraps at 64 bits (step0 = 2**64 - 1); the last step's next_start is the carry and the
    windowed last step writes no frame; each layout leaves the other's frame field alone."""
    T, n, step0 = 3, 5, U64
    buf, carry = DeviceRolloutBuffer(T, n, 4, "cpu"), torch.empty(n)
    slot, move = slot_cursor(buf, carry, window, 2 ** 64 + 7, step0, clip)
    assert (slot.act_seed, slot.flags, slot.reserved) == (7, F16_SLOT_CLIP if clip else 0, 0)
    for t in range(T):
        assert move(t) is slot
        last = t == T - 1
        assert slot.act_step == (step0 + t) & U64 == (t - 1) % 2 ** 64
        assert slot.actions == buf.actions[t].data_ptr()
        assert slot.rewards == buf.rewards[t].data_ptr()
        assert slot.next_start == (carry if last else buf.episode_starts[t + 1]).data_ptr()
        assert slot.features is None
        if window:
            assert slot.frame is None
            assert slot.next_frame == (None if last else buf.frames[t + 1].data_ptr())
        else:
            assert slot.frame == buf.frames[t].data_ptr() and slot.next_frame is None
        assert slot.flags == (F16_SLOT_CLIP if clip else 0)


class SlotEnvs:
    """A fused env's surface with no dynamics: records the slot and action address of every raw
    slot step (the observation counts the steps)."""

    def __init__(self, n, k, window, device="cpu", **cfg):
        self.torch, self.n, self.k, self.window, self.device = torch, n, k, window, torch.device(device)
        self.cfg = config_default(n_envs=n, stack_k=k, **cfg)
        self._act = torch.zeros((n, 4))
        self.obs = torch.zeros((n, k, 15))
        self.calls = []

    def step_rollout(self, *args, **kw):
        raise AssertionError("the collector steps through _step_rollout_raw")

    def _step_rollout_raw(self, slot, act_ptr):
        self.calls.append(({name: getattr(slot, name) for name, _ in RolloutSlot._fields_}, act_ptr))
        self.obs = self.obs + 1.0
        none = torch.zeros(self.n, dtype=torch.uint8)
        return StepOut(self.obs, torch.zeros(self.n), none, none, self.obs, None, None)


@LAYOUTS
def test_fused_driver_random_policy(window):
    """The driver around the slot step, random policy: obs0, episode_starts[0] (ones on a fresh
    env, the carried starts on the next rollout) and the windowed layout's frames[0] are primed, the
    slot carries no CLIP flag and no action address, act_step = step0 + t, the buffer ends full
    and the carry becomes envs._last_episode_starts and last_dones."""
    T, n, k = 3, 8, 4  # (n = 5's 300-byte frame row would send the contiguous layout down the generic path)
    envs, buf = SlotEnvs(n, k, window), DeviceRolloutBuffer(T, n, k, "cpu")
    envs.obs += 3.0
    buf.frames.fill_(-1.0)
    assert choose_path(envs, buf, None, True, True) == "fused"  # (no rollout_random: not persistent)
    last_v, last_d = collect_rollout(envs, buf, seed=9, step0=100)
    assert buf.full and torch.equal(buf.obs0, torch.full((n, k, 15), 3.0))
    assert torch.equal(buf.episode_starts[0], torch.ones(n))
    assert torch.equal(buf.frames[0], torch.full((n, 15), 3.0 if window else -1.0))
    assert [(s["act_seed"], s["act_step"], s["flags"], a) for s, a in envs.calls] == [(9, 100 + t, 0, None) for t in range(T)]
    assert last_d is envs._last_episode_starts and last_d.data_ptr() == envs.calls[-1][0]["next_start"]
    assert torch.equal(last_v, torch.zeros(n)) and torch.equal(envs.obs, torch.full((n, k, 15), 3.0 + T))
    last_d.fill_(0.25)
    collect_rollout(envs, buf, seed=9, step0=100 + T)
    assert torch.equal(buf.episode_starts[0], torch.full((n,), 0.25))


def test_fused_driver_closure_policy(monkeypatch):
    """With a policy the slot holds F16_SLOT_CLIP and the step is handed the address of the
    policy's own (aligned, contiguous) actions; values / log-probs land in the buffer's rows and
    last_values = V(final obs). The bootstrap kernel is the GPU's: here it is replaced by nothing."""
    monkeypatch.setattr(rollout, "_PerStepBootstrap", lambda buf, vfn: rollout._NoBootstrap())
    T, n, k = 3, 5, 4
    envs, buf, acts = SlotEnvs(n, k, True), DeviceRolloutBuffer(T, n, k, "cpu"), []

    def policy(obs):
        acts.append(torch.full((n, 4), float(len(acts))))
        return acts[-1], obs[:, -1, 0] * 2.0, obs[:, -1, 0] * -3.0
    last_v, _ = collect_rollout(envs, buf, policy_fn=policy, bootstrap="per_step")
    assert [(s["flags"], a) for s, a in envs.calls] == [(F16_SLOT_CLIP, x.data_ptr()) for x in acts[:T]]
    steps = torch.arange(T, dtype=torch.float32)[:, None].expand(T, n)
    assert torch.equal(buf.values, steps * 2.0) and torch.equal(buf.log_probs, steps * -3.0)
    assert torch.equal(last_v, torch.full((n,), T * 2.0))


# ---------------------------------------------------------------------------------------------------
# the deferred bootstrap's stash
def _most_truncations(T, max_steps, terminations=False):
    """The most times one lane can truncate in T steps, by running the TimeLimit counter from
    every count a lane can start a rollout with (and, if asked, under every pattern of
    terminations, which restart the counter like a truncation does)."""
    best = 0
    patterns = itertools.product((False, True), repeat=T) if terminations else [(False,) * T]
    for pattern in patterns:
        for count0 in range(max_steps):
            count, hits = count0, 0
            for terminated in pattern:
                count += 1
                if terminated:
                    count = 0
                elif count >= max_steps:
                    count, hits = 0, hits + 1
            best = max(best, hits)
    return best


def test_stash_capacity_is_the_most_truncations():
    for T in range(1, 14):
        for max_steps in range(1, 8):
            want = _most_truncations(T, max_steps, terminations=T <= 8)
            for n in (1, 5):
                assert stash_capacity(n, T, max_steps) == n * want, (n, T, max_steps)


def _sizes(n=5, T=12, k=4, max_steps=5, flags=0):
    return (SimpleNamespace(cfg=SimpleNamespace(flags=flags, max_steps=max_steps)),
            SimpleNamespace(n_envs=n, n_steps=T, k=k))


def test_deferral_flips_to_per_step_exactly_at_the_byte_limit(monkeypatch):
    envs, buf = _sizes()
    stash_bytes = stash_capacity(5, 12, 5) * 4 * 15 * 4
    assert stash_bytes == 15 * 240 and stash_bytes < rollout.STASH_MAX_BYTES
    policy = lambda obs: None  # noqa: E731
    assert can_defer(envs, buf, policy, "deferred")
    for limit, want in ((stash_bytes + 1, True), (stash_bytes, True), (stash_bytes - 1, False)):
        monkeypatch.setattr(rollout, "STASH_MAX_BYTES", limit)
        assert can_defer(envs, buf, policy, "deferred") is want, limit


def test_deferral_needs_a_policy_autoreset_and_the_mode():
    policy = lambda obs: None  # noqa: E731
    envs, buf = _sizes()
    assert can_defer(envs, buf, policy, "deferred")
    assert not can_defer(envs, buf, None, "deferred")
    assert not can_defer(envs, buf, policy, "per_step")
    assert not can_defer(_sizes(flags=F16_FLAG_NO_AUTORESET | F16_FLAG_GUSTS)[0], buf, policy, "deferred")
    assert can_defer(_sizes(flags=F16_FLAG_GUSTS)[0], buf, policy, "deferred")  # (another flag is not that one)


# ---------------------------------------------------------------------------------------------------
# the path choice
class _At:
    """A tensor's address, as choose_path reads it (x.data_ptr(), x[0].data_ptr())."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address

    def __getitem__(self, i):
        return self


def _choice_before_the_split(envs, buf, policy_fn, fused, persistent):
    """collect_rollout's conditions as they stood inline before the paths were split."""
    n, window = buf.n_envs, bool(getattr(envs, "window", False))
    use_fused = fused and hasattr(envs, "step_rollout") and buf.actions.data_ptr() % 16 == 0 \
        and (window or (buf.frames[0].data_ptr() % 16 == 0 and (n * 15 * 4) % 16 == 0))
    use_persistent = use_fused and persistent and policy_fn is None and hasattr(envs, "rollout_random") \
        and not (envs.cfg.flags & F16_FLAG_NO_AUTORESET)
    return "persistent" if use_persistent else "fused" if use_fused else "generic"


_BASE = dict(fused=True, persistent=True, policy=False, step_rollout=True, rollout_random=True, window=False,
             autoreset=True, actions_at=4096, frames_at=8192, n=4)
_FLIPS = dict(fused=False, persistent=False, policy=True, step_rollout=False, rollout_random=False, window=True,
              autoreset=False, actions_at=4096 + 8, frames_at=8192 + 4, n=5)  # (n = 5: a 300-byte frame row)


def _choose(c, choose=choose_path):
    envs = SimpleNamespace(cfg=SimpleNamespace(flags=0 if c["autoreset"] else F16_FLAG_NO_AUTORESET))
    for name in ("step_rollout", "rollout_random"):
        if c[name]:
            setattr(envs, name, None)
    if c["window"]:
        envs.window = True
    buf = SimpleNamespace(n_envs=c["n"], actions=_At(c["actions_at"]), frames=_At(c["frames_at"]))
    return choose(envs, buf, (lambda obs: None) if c["policy"] else None, c["fused"], c["persistent"])


def test_path_choice_each_condition():
    assert _choose(_BASE) == "persistent"
    want = dict(fused="generic", step_rollout="generic", actions_at="generic", frames_at="generic", n="generic",
                persistent="fused", policy="fused", rollout_random="fused", autoreset="fused", window="persistent")
    for name, value in _FLIPS.items():
        assert _choose(dict(_BASE, **{name: value})) == want[name], name
    # the windowed layout writes no frame through the slot's 16-byte stores: its alignment does not matter
    for name in ("frames_at", "n"):
        assert _choose(dict(_BASE, window=True, **{name: _FLIPS[name]})) == "persistent", name


def test_path_choice_every_combination_as_before_the_split():
    names = list(_BASE)
    for values in itertools.product(*((_BASE[k], _FLIPS[k]) for k in names)):
        c = dict(zip(names, values))
        assert _choose(c) == _choose(c, _choice_before_the_split), c


def test_path_choice_of_a_foreign_env():
    from fake_envs import FakeEnvs
    assert choose_path(FakeEnvs(6, k=3), DeviceRolloutBuffer(4, 6, 3, "cpu")) == "generic"


# ---------------------------------------------------------------------------------------------------
# checks before the first write
def _marked_buffer(T, n, k):
    buf = DeviceRolloutBuffer(T, n, k, "cpu")
    buf.pos = 2
    for x in buf.state_dict().values():
        x.fill_(7.0)
    return buf, {f: x.clone() for f, x in buf.state_dict().items()}


def _untouched(buf, before):
    return buf.pos == 2 and all(torch.equal(x, before[f]) for f, x in buf.state_dict().items())


@pytest.mark.parametrize("with_policy", [False, True], ids=["random", "policy"])
def test_bad_bootstrap_raises_on_the_generic_path_before_any_write(with_policy):
    from fake_envs import FakeEnvs
    envs = FakeEnvs(6, k=3)
    envs.reset()
    buf, before = _marked_buffer(4, 6, 3)
    policy = (lambda obs: (torch.zeros(6, 4), torch.zeros(6), torch.zeros(6))) if with_policy else None
    with pytest.raises(ValueError, match="bootstrap must be 'deferred' or 'per_step'"):
        collect_rollout(envs, buf, policy_fn=policy, bootstrap="defered")
    assert _untouched(buf, before) and not hasattr(envs, "_last_episode_starts")
    assert int(envs.steps.sum()) == 0  # (the env was not stepped either)


@pytest.mark.parametrize("rollout_random", [False, True], ids=["fused", "persistent"])
def test_bad_bootstrap_raises_on_the_device_paths_before_any_write(rollout_random):
    envs = SlotEnvs(5, 4, True)
    if rollout_random:
        envs.rollout_random = None  # (never reached)
    buf, before = _marked_buffer(3, 5, 4)
    assert choose_path(envs, buf) == ("persistent" if rollout_random else "fused")
    with pytest.raises(ValueError, match="bootstrap must be"):
        collect_rollout(envs, buf, bootstrap="")
    assert _untouched(buf, before) and envs.calls == []


def test_device_mismatch_raises_before_any_write():
    envs = SlotEnvs(5, 4, True, device="cuda:0")  # (a device's name alone: nothing is placed there)
    buf, before = _marked_buffer(3, 5, 4)
    with pytest.raises(ValueError, match="rollout buffer on cpu, envs on cuda:0"):
        collect_rollout(envs, buf)
    assert _untouched(buf, before) and envs.calls == [] and not hasattr(envs, "_last_episode_starts")
