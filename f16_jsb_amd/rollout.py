"""Device-resident PPO rollout storage, GAE and the rank-0 gather (BASELINE cfg 4).

The caller side of the hot path: SB3's `collect_rollouts`
(on_policy_algorithm.py:162-268) fills a numpy `RolloutBuffer` (buffers.py:343-522) one env at
a time. Here the buffer lives in HBM as [n_steps][n_envs] tensors, GAE runs as the HIP kernel
`f16env_gae` (bit-exact with buffers.py:403-438's float32 numpy recurrence), and after a
rollout every rank's shard lands on rank 0 with RCCL gathers over xGMI
(`torch.distributed` backend "nccl" is RCCL on ROCm).

Frame dedup: a stacked observation is K overlapping frames, so the buffer keeps
only the newest frame per step plus the stack before step 0, and rebuilds any step's stack
from those and `episode_starts` (a reset observation is K copies of its first frame). That
cuts the gathered observation bytes by K.

The update's data side (buffers.py:481-521): `DeviceRolloutBuffer.get` / `minibatches` yield
shuffled minibatches, each gathered from the deduplicated log by one `f16env_rollout_minibatch`
launch, so the stacked (T, N, K, 15) array is never materialised.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Dict, Optional

import torch

from ._lib import check, fn, lib
from .abi import F16_FLAG_NO_AUTORESET, F16_OBS_DIM, F16_SLOT_CLIP, RolloutSlot, RolloutView
from .buffers import need_tensor, stream_ptr
from .layouts import U64, as_act
from .policy import DevicePolicy

FIELDS = ("frames", "actions", "rewards", "episode_starts", "values", "log_probs", "advantages", "returns")
# device memory the deferred timeout bootstrap may take for its stash of terminal observations
STASH_MAX_BYTES = 1 << 30


class DeviceRolloutBuffer:
    def __init__(self, n_steps: int, n_envs: int, stack_k: int, device, gamma: float = 0.99,
                 gae_lambda: float = 0.95, act_dim: int = 4):
        self.n_steps, self.n_envs, self.k = int(n_steps), int(n_envs), int(stack_k)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.device = torch.device(device)
        f32 = torch.float32
        z = lambda *s: torch.zeros(*s, dtype=f32, device=self.device)  # noqa: E731
        self.frames = z(self.n_steps, self.n_envs, F16_OBS_DIM)       # newest frame of obs[t]
        self.obs0 = z(self.n_envs, self.k, F16_OBS_DIM)                # full stack of obs[0]
        self.actions = z(self.n_steps, self.n_envs, act_dim)
        self.rewards = z(self.n_steps, self.n_envs)
        self.episode_starts = z(self.n_steps, self.n_envs)
        self.values = z(self.n_steps, self.n_envs)
        self.log_probs = z(self.n_steps, self.n_envs)
        self.advantages = z(self.n_steps, self.n_envs)
        self.returns = z(self.n_steps, self.n_envs)
        self.pos = 0

    def reset(self):
        self.pos = 0

    @property
    def full(self) -> bool:
        return self.pos == self.n_steps

    def add(self, obs, action, reward, episode_start, value, log_prob):
        """RolloutBuffer.add (buffers.py:440-479) with device tensors; obs is (N, K, 15)."""
        if self.pos >= self.n_steps:
            raise RuntimeError("rollout buffer is full")
        t = self.pos
        if t == 0:
            self.obs0.copy_(obs)
        self.frames[t].copy_(obs[:, -1])
        self.actions[t].copy_(action.reshape(self.n_envs, -1))
        self.rewards[t].copy_(reward.reshape(-1))
        self.episode_starts[t].copy_(episode_start.reshape(-1).to(torch.float32))
        self.values[t].copy_(value.reshape(-1))
        self.log_probs[t].copy_(log_prob.reshape(-1))
        self.pos += 1

    def compute_returns_and_advantage(self, last_values, dones, stream=None):
        """buffers.py:403-438 on the GPU (HIP kernel f16env_gae)."""
        if self.device.type != "cuda":
            raise RuntimeError("GAE runs on the GPU (f16env_gae); buffer is on %s" % self.device)
        lv = torch.as_tensor(last_values).reshape(-1).to(self.device, torch.float32).contiguous()
        dn = torch.as_tensor(dones).reshape(-1).to(self.device, torch.uint8).contiguous()
        if lv.numel() != self.n_envs or dn.numel() != self.n_envs:  # the kernel reads n_envs of each
            raise ValueError("last_values and dones must hold n_envs = %d entries, got %d and %d"
                             % (self.n_envs, lv.numel(), dn.numel()))
        s = ctypes.c_void_p(stream) if stream is not None else stream_ptr(self.device)
        check(lib().f16env_gae(s, self.n_steps, self.n_envs, self.rewards.data_ptr(),
                               self.values.data_ptr(), self.episode_starts.data_ptr(), lv.data_ptr(),
                               dn.data_ptr(), self.gamma, self.gae_lambda, self.advantages.data_ptr(),
                               self.returns.data_ptr()), "f16env_gae")

    # ----------------------------------------------------------------------------------------
    def observations(self, steps=None):
        return rebuild_observations(self.frames, self.obs0, self.episode_starts, self.k, steps)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {f: getattr(self, f) for f in FIELDS} | {"obs0": self.obs0}

    def get(self, batch_size: Optional[int] = None, indices=None, generator=None):
        """RolloutBuffer.get (buffers.py:481-506) on the device: a generator of RolloutSamples over
        one shuffled pass of the n_steps * n_envs transitions, each minibatch gathered by one
        f16env_rollout_minibatch launch from the frame-deduplicated log (nothing proportional to
        T * N * K is ever allocated; see rollout_minibatch and flat_index for the order).
        The permutation is `indices` when given (a numpy array or CPU tensor, e.g. SB3's own
        np.random.permutation(T * N), is moved to the device once; range-checked once), else
        torch.randperm(T * N, device=..., generator=generator) (whose own sort needs a few times the
        permutation's 8 B per transition while it runs; the pass itself holds the permutation and
        the minibatches in flight). batch_size None: one batch of everything; a short last
        minibatch is yielded as it is; every yield is fresh tensors."""
        if not self.full:
            raise RuntimeError("rollout buffer is not full (pos %d of %d)" % (self.pos, self.n_steps))
        return _minibatches(self, self.k, self.n_steps * self.n_envs, self.device, batch_size, indices, generator)


ACTION_LOW = (-1.0, -1.0, -1.0, 0.0)   # jsbsim_gym.py:143-148 action Box
ACTION_HIGH = (1.0, 1.0, 1.0, 1.0)


def np_clip_actions(a):
    """np.clip(actions, action_space.low, action_space.high) (on_policy_algorithm.py:216) in
    torch with numpy's clip-ufunc semantics: min(max(x, lo), hi), max(a, b) = a if a is NaN or
    a > b else b (so NaN passes and -0 clips to +0 at a 0 bound) -- the in-kernel clip
    (f16_rng.h np_clip) computes the same."""
    lo = torch.tensor(ACTION_LOW, dtype=a.dtype, device=a.device)
    hi = torch.tensor(ACTION_HIGH, dtype=a.dtype, device=a.device)
    m = torch.where(torch.isnan(a) | (a > lo), a, lo)
    return torch.where(torch.isnan(m) | (m < hi), m, hi)


def choose_path(envs, buf, policy_fn=None, fused: bool = True, persistent: bool = True) -> str:
    """Which way collect_rollout collects, from its arguments' attributes alone (no launch, no
    allocation): "persistent" (one launch), "fused" (one rollout-slot launch per step) or
    "generic" (envs.step + buf.add). Fused needs an env with step_rollout and the 16-byte
    alignment its vector stores assume: of buf.actions and, for the contiguous layout, of
    buf.frames[0] and the frame row; persistent also the random policy, an env with
    rollout_random and auto-reset on."""
    if not (fused and hasattr(envs, "step_rollout") and buf.actions.data_ptr() % 16 == 0):
        return "generic"
    if not getattr(envs, "window", False) and (buf.frames[0].data_ptr() % 16 or (buf.n_envs * F16_OBS_DIM * 4) % 16):
        return "generic"
    if persistent and policy_fn is None and hasattr(envs, "rollout_random") and not envs.cfg.flags & F16_FLAG_NO_AUTORESET:
        return "persistent"
    return "fused"


def slot_cursor(buf, carry, window: bool, seed: int, step0: int, clip: bool):
    """(slot, move): the RolloutSlot of a fused rollout and move(t) -> slot, which points its rows
    at step t by integer arithmetic on addresses and row strides taken here, once (the buffer
    was allocated with these shapes: no per-step views or checks on the launch path). The
    contiguous layout writes frames[t], the windowed one frames[t + 1] (the returned
    observation's newest frame; the last step none); next_start is episode_starts[t + 1], the
    last step's `carry`. No GPU call."""
    n, T, step0 = buf.n_envs, buf.n_steps, int(step0)
    slot = RolloutSlot(int(seed) & U64, 0, None, None, None, None, None, None, F16_SLOT_CLIP if clip else 0, 0)
    fr0, ac0, rw0, st0 = (x.data_ptr() for x in (buf.frames, buf.actions, buf.rewards, buf.episode_starts))
    fb, ab, rb, last = n * F16_OBS_DIM * 4, n * 16, n * 4, carry.data_ptr()

    def move(t):
        slot.act_step = (step0 + t) & U64
        if window:
            slot.next_frame = fr0 + (t + 1) * fb if t + 1 < T else None
        else:
            slot.frame = fr0 + t * fb
        slot.actions, slot.rewards = ac0 + t * ab, rw0 + t * rb
        slot.next_start = st0 + (t + 1) * rb if t + 1 < T else last
        return slot
    return slot, move


def stash_capacity(n: int, T: int, max_steps: int) -> int:
    """Rows the deferred bootstrap's stash needs: a lane truncates at most once per max_steps
    steps (auto-reset restarts its counter), so at most (T - 1) // max_steps + 1 times in T."""
    return n * ((T - 1) // max(1, int(max_steps)) + 1)


def can_defer(envs, buf, policy_fn, bootstrap: str) -> bool:
    """Whether the timeout bootstrap is deferred: asked for, with a policy, on an auto-resetting
    handle, and the stash within STASH_MAX_BYTES (very short TimeLimits: else per step)."""
    return policy_fn is not None and bootstrap == "deferred" and not int(envs.cfg.flags) & F16_FLAG_NO_AUTORESET \
        and stash_capacity(buf.n_envs, buf.n_steps, envs.cfg.max_steps) * buf.k * F16_OBS_DIM * 4 <= STASH_MAX_BYTES


class _DeferredBootstrap:
    """The stash of the truncated lanes' terminal observations: push after each step
    (f16env_bootstrap_stash, no host sync), apply once after the loop."""

    def __init__(self, envs, buf):
        dev, self.n, self.k, self.gamma = buf.device, buf.n_envs, buf.k, buf.gamma
        self.cap = stash_capacity(buf.n_envs, buf.n_steps, envs.cfg.max_steps)
        self.stash = torch.empty((self.cap, buf.k, F16_OBS_DIM), dtype=torch.float32, device=dev)
        self.idx = torch.empty(self.cap, dtype=torch.int64, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.dev, self.fn = dev, lib().f16env_bootstrap_stash
        self.ptrs = (self.stash.data_ptr(), self.idx.data_ptr(), self.count.data_ptr(), self.cap)

    def push(self, out, t):
        tobs, n = out.terminal_obs, self.n
        check(self.fn(stream_ptr(self.dev), n, self.k, tobs.data_ptr(), tobs.stride(0), tobs.stride(1),
                      out.terminated.data_ptr(), out.truncated.data_ptr(), t * n, *self.ptrs), "f16env_bootstrap_stash")

    def apply(self, vfn, rewards):
        """V once over every stashed terminal observation, then rewards += gamma * V."""
        m = int(self.count.item())
        if m > self.cap:
            raise RuntimeError("bootstrap stash overflow (%d > %d)" % (m, self.cap))
        if m:
            tv = vfn(self.stash[:m]).reshape(-1).to(torch.float32).contiguous()
            check(lib().f16env_bootstrap_apply(stream_ptr(self.dev), m, rewards.data_ptr(), self.idx.data_ptr(),
                                               tv.data_ptr(), self.gamma), "f16env_bootstrap_apply")


class _NoBootstrap:
    """The same two calls for the random policy, which has no value function: nothing bootstraps."""

    def push(self, out, t):
        pass

    def apply(self, vfn, rewards):
        pass


class _PerStepBootstrap(_NoBootstrap):
    """V over the step's whole batch of terminal observations every step
    (f16env_bootstrap_timeouts): nothing is left to apply."""

    def __init__(self, buf, vfn):
        self.dev, self.n, self.gamma, self.vfn = buf.device, buf.n_envs, buf.gamma, vfn
        self.rw0, self.fn = buf.rewards.data_ptr(), lib().f16env_bootstrap_timeouts

    def push(self, out, t):
        tv = self.vfn(out.terminal_obs).reshape(-1).to(torch.float32).contiguous()
        check(self.fn(stream_ptr(self.dev), self.n, self.rw0 + t * self.n * 4, out.terminated.data_ptr(),
                      out.truncated.data_ptr(), tv.data_ptr(), self.gamma), "f16env_bootstrap_timeouts")


def _policy_adaptor(envs, buf, policy_fn, step0: int):
    """act(obs, t) -> the address of step t's (N, 4) actions, values[t] and log_probs[t] written:
    None for the random policy (the step kernel draws them); a DevicePolicy writes the buffer's
    rows itself and its actions into one reused scratch (no per-step copies or shape fix-ups);
    a closure's results are copied in."""
    n, values, log_probs = buf.n_envs, buf.values, buf.log_probs
    if policy_fn is None:
        return lambda obs, t: None
    if isinstance(policy_fn, DevicePolicy):
        scratch = torch.empty((n, 4), dtype=torch.float32, device=buf.device)
        forward_into, step0, ptr = policy_fn.forward_into, int(step0), scratch.data_ptr()

        def act(obs, t):
            forward_into(obs, step0 + t, scratch, values[t], log_probs[t])
            return ptr
        return act
    held = [None]  # (the actions stay alive until the next step's replace them)

    def act(obs, t):
        a, v, lp = policy_fn(obs)
        held[0] = a = as_act(envs, a.reshape(n, 4), "policy actions")
        values[t].copy_(v.reshape(-1))
        log_probs[t].copy_(lp.reshape(-1))
        return a.data_ptr()
    return act


def _collect_persistent(envs, buf, seed, step0, carry):
    """The whole rollout in one launch (random policy); returns the final observation."""
    envs.rollout_random(seed, step0, buf.n_steps, buf.frames, buf.actions, buf.rewards,
                        buf.episode_starts[1:] if buf.n_steps > 1 else None, carry)
    return envs.obs


def _collect_fused(envs, buf, seed, step0, policy_fn, vfn, bootstrap, carry):
    """One rollout-slot launch per step; per step: the slot's addresses, at most one policy
    call, the launch, at most one bootstrap call. Returns the final observation."""
    obs, window = envs.obs, bool(getattr(envs, "window", False))
    if window:  # the log's first frame; step t then writes frames[t + 1] (the returned obs's newest)
        buf.frames[0].copy_(obs[:, -1])
    move = slot_cursor(buf, carry, window, seed, step0, clip=policy_fn is not None)[1]
    act = _policy_adaptor(envs, buf, policy_fn, step0)
    boot = _NoBootstrap() if policy_fn is None else _DeferredBootstrap(envs, buf) \
        if can_defer(envs, buf, policy_fn, bootstrap) else _PerStepBootstrap(buf, vfn)
    step, push = envs._step_rollout_raw, boot.push
    for t in range(buf.n_steps):
        out = step(move(t), act(obs, t))
        push(out, t)
        obs = out.obs
    boot.apply(vfn, buf.rewards)
    return obs


def _collect_generic(envs, buf, seed, step0, policy_fn, vfn, starts, zeros):
    """envs.step + buf.add per step (any env with obs / step / sample_actions); returns the
    final observation and the episode starts after the last step."""
    obs = envs.obs
    for t in range(buf.n_steps):
        obs = obs.clone()  # (an env may reuse its observation buffer in the step below)
        if policy_fn is not None:
            act, v, lp = policy_fn(obs)
            act = act.reshape(buf.n_envs, -1).to(torch.float32)
            out = envs.step(np_clip_actions(act).contiguous())
            rew = bootstrap_timeouts(out.rew, out.terminated, out.truncated, vfn(out.terminal_obs), buf.gamma)
        else:
            act, v, lp = envs.sample_actions(seed, step0 + t), zeros, zeros
            out = envs.step(act)
            rew = out.rew
        buf.add(obs, act, rew, starts, v, lp)
        obs = out.obs
        starts = (out.terminated | out.truncated).to(torch.float32)
    return obs, starts


def collect_rollout(envs, buf: DeviceRolloutBuffer, seed: int = 0, step0: int = 0, policy_fn=None, value_fn=None,
                    fused: bool = True, persistent: bool = True, bootstrap: str = "deferred"):
    """collect_rollouts (on_policy_algorithm.py:162-268) over device tensors. Starts from the
    envs' current observation; returns (last_values, last_dones) for GAE (:258-262).

    policy_fn(obs) -> (actions, values, log_probs): the policy in the loop (:199-202), called on
    the (N, K, 15) device observation. The env steps np.clip(actions, low, high) (:216; clipped
    in the step kernel), the buffer stores the UNCLIPPED actions with the values and log-probs
    (:247-254); a lane that ended by truncation alone bootstraps rewards += gamma *
    V(terminal_obs) (:236-245, f16env_bootstrap_timeouts: V is evaluated on the whole batch of
    terminal observations, no host sync, only those lanes' rewards change); V = value_fn(obs) ->
    values when given, else policy_fn's values; last_values = V(final obs).
    policy_fn None: the uniform random policy from the device Philox stream (seed, step0 + t),
    values and log-probs zero, no bootstrap.
    policy_fn a DevicePolicy (f16_jsb_amd.policy): the fused path calls its kernel with
    step = step0 + t and the buffer's own rows as outputs (values[t], log_probs[t]; the actions
    through one reused (N, 4) scratch the step's slot reads), and value_fn defaults to its
    .value -- bit-identical to the same policy driven through a closure on the generic path.

    fused: each step is ONE launch (f16env_step_rollout / f16env_window_step_rollout) that takes
    (or draws) the actions and writes the slot's actions / rewards / next episode starts and one
    frame of the frame-deduplicated log itself, instead of a sampling launch, the step and six
    buffer copies (RolloutBuffer.add, buffers.py:440-479).
    persistent (no policy_fn): the whole rollout is ONE launch (f16env_rollout_random /
    f16env_window_rollout_random) that keeps every env's state on-chip across the steps:
    bit-identical to the fused launches.
    bootstrap "deferred" (fused path, auto-resetting handles): the terminal observations of the
    lanes that end by truncation alone are appended to a device stash after each step
    (f16env_bootstrap_stash, no host sync) and V runs ONCE over the stash after the loop
    (f16env_bootstrap_apply scatters gamma * V into the rewards) -- the value network does not
    change during a rollout, so this is :236-245's arithmetic with one evaluation instead of one
    per step over the whole batch; "per_step": V over the step's whole batch of terminal
    observations every step (f16env_bootstrap_timeouts). The two agree bit for bit when V's value
    for a row does not depend on the batch it is evaluated in. SB3 itself evaluates each terminal
    observation in a batch of ONE (`predict_values(terminal_obs)[0]` inside its per-env loop,
    :236-245); both modes here evaluate a batch, so for a value head whose GEMMs round a row
    differently at another batch size the bootstrapped rewards may differ from SB3's, and between
    the two modes, in the last bits (tests/test_gpu_policy_rollout.py
    test_bootstrap_modes_vs_batch_of_one bounds it); the lanes that bootstrap are the same.
    Any other `bootstrap`, on every path, and a fused rollout whose buffer and envs sit on
    different devices raise ValueError before anything is written."""
    if bootstrap not in ("deferred", "per_step"):
        raise ValueError("bootstrap must be 'deferred' or 'per_step'")
    path = choose_path(envs, buf, policy_fn, fused, persistent)
    dev, n = buf.device, buf.n_envs
    if path == "fused" and getattr(envs, "device", dev) != dev:
        raise ValueError("rollout buffer on %s, envs on %s" % (dev, envs.device))
    vfn = value_fn if value_fn is not None else policy_fn.value if isinstance(policy_fn, DevicePolicy) \
        else (lambda o: policy_fn(o)[1])
    zeros = torch.zeros(n, dtype=torch.float32, device=dev)
    starts = getattr(envs, "_last_episode_starts", None)
    if starts is None:
        starts = torch.ones(n, dtype=torch.float32, device=dev)
    buf.reset()
    if path == "generic":  # (buf.add keeps obs0 and episode_starts[0] itself)
        obs, starts = _collect_generic(envs, buf, seed, step0, policy_fn, vfn, starts, zeros)
    else:
        buf.obs0.copy_(envs.obs)
        buf.episode_starts[0].copy_(starts)
        starts = torch.empty(n, dtype=torch.float32, device=dev)  # the carry: the episode starts after the last step
        if path == "persistent":
            obs = _collect_persistent(envs, buf, seed, step0, starts)
        else:
            obs = _collect_fused(envs, buf, seed, step0, policy_fn, vfn, bootstrap, starts)
        buf.pos = buf.n_steps
    envs._last_episode_starts = starts
    return (vfn(obs).reshape(-1).to(torch.float32) if policy_fn is not None else zeros), starts


def bootstrap_timeouts(rewards, terminated, truncated, terminal_values, gamma: float):
    """on_policy_algorithm.py:236-245 vectorised: for lanes that ended by truncation only,
    rewards += gamma * V(terminal_observation) (float32 per-op rounding as SB3; the HIP kernel
    f16env_bootstrap_timeouts computes the same in place)."""
    mask = truncated.bool() & ~terminated.bool()
    g = torch.tensor(gamma, dtype=torch.float32, device=rewards.device)
    add = g * terminal_values.reshape(-1).to(torch.float32)
    return torch.where(mask, rewards + add, rewards)


def rebuild_observations(frames, obs0, episode_starts, k: int, steps=None):
    """Stacked observations (T, N, K, 15) from newest frames, the initial stack and
    episode starts: obs[t][j] = frame[max(t - (K-1) + j, s_t)] where s_t is the last episode
    start <= t; indices before step 0 come from the initial stack (oldest first)."""
    T, N, D = frames.shape
    dev = frames.device
    tt = torch.arange(T, device=dev)
    if steps is None:
        steps = tt
    steps = torch.as_tensor(steps, device=dev)
    # last episode start at or before t, per env (-inf if none)
    marks = torch.where(episode_starts.bool(), tt[:, None].expand(T, N), torch.full((T, N), -(1 << 30), device=dev))
    last_start = torch.cummax(marks, dim=0).values                      # (T, N)
    j = torch.arange(k, device=dev)
    src = steps[:, None] - (k - 1) + j[None, :]                          # (S, K)
    ls = last_start[steps]                                               # (S, N)
    idx = torch.maximum(src[:, None, :], ls[:, :, None])                # (S, N, K)
    from_frames = idx >= 0
    fi = idx.clamp(min=0)
    e = torch.arange(N, device=dev)[None, :, None].expand_as(fi)
    out_f = frames[fi, e]                                                # (S, N, K, D)
    oi = (idx + (k - 1)).clamp(0, k - 1)                                 # position in obs0
    out_0 = obs0[e, oi]                                                  # (S, N, K, D)
    return torch.where(from_frames[..., None], out_f, out_0)


def gather_to_rank0(buf: DeviceRolloutBuffer, group=None, chunk_steps: Optional[int] = None,
                    fields=FIELDS) -> Optional[Dict[str, torch.Tensor]]:
    """Gather every rank's rollout shard to rank 0 (RCCL over xGMI on MI355X, gloo in CPU
    tests). Returns on rank 0 a dict of RANK-MAJOR tensors (world, n_steps, n_envs, ...) -- rank
    r's shard at [r], i.e. global envs [r * n_envs, (r + 1) * n_envs) as env_id_base assigns them
    -- plus 'obs0' (world, n_envs, K, 15); None on other ranks. ``env_major`` turns a field into
    the (n_steps, world * n_envs, ...) layout of a single-GPU buffer.

    The output is allocated once and every collective writes straight into it: chunk [t0, t1)
    of rank r lands in the contiguous view out[r, t0:t1], so rank 0 moves each byte once (no
    per-chunk temporaries, no strided re-copy). Gathers are chunked over steps (chunk_steps) to
    bound each collective's size; a short last chunk is fine."""
    import torch.distributed as dist

    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    T = buf.n_steps
    chunk = T if not chunk_steps else max(1, int(chunk_steps))
    out = {}
    for f in tuple(fields) + ("obs0",):
        x = getattr(buf, f)
        if not x.is_contiguous():
            x = x.contiguous()
        res = torch.empty((world,) + tuple(x.shape), dtype=x.dtype, device=x.device) if rank == 0 else None
        if f == "obs0":
            dist.gather(x, list(res.unbind(0)) if rank == 0 else None, dst=0, group=group)
        else:
            for t0 in range(0, T, chunk):
                t1 = min(T, t0 + chunk)
                dist.gather(x[t0:t1], [res[r, t0:t1] for r in range(world)] if rank == 0 else None, dst=0, group=group)
        if rank == 0:
            out[f] = res
    return out if rank == 0 else None


def env_major(x: torch.Tensor) -> torch.Tensor:
    """(world, T, N, ...) rank-major gather output -> (T, world * N, ...) (a copy)."""
    w, T, N = x.shape[:3]
    return x.transpose(0, 1).reshape((T, w * N) + tuple(x.shape[3:]))


# ------------------------------------------------------------------------------------------------
# The PPO update's data side: shuffled minibatches straight from the frame-deduplicated log.
RolloutSamples = namedtuple("RolloutSamples", ("observations", "actions", "old_values", "old_log_prob",
                                               "advantages", "returns"))
RolloutSamples.__doc__ = """One minibatch of device tensors, SB3's RolloutBufferSamples field for field
(type_aliases.py): observations (B, K, 15), actions (B, 4), old_values, old_log_prob, advantages,
returns (B,)."""

VIEW_FIELDS = ("frames", "obs0", "episode_starts", "values", "log_probs", "advantages", "returns", "actions")


def flat_index(t, env, n_steps: int):
    """Flat index of transition (step t, global env) in SB3's swap_and_flatten order over the
    (T, n_envs) buffer (buffers.py:36-50, :493-503): env * n_steps + t. After gather_to_rank0 the
    global env of shard r's env n is r * n_envs + n. Ints, numpy arrays or tensors."""
    return env * n_steps + t


def unflatten_index(i, n_steps: int):
    """flat_index's inverse: (t, env)."""
    return i % n_steps, i // n_steps


class _View:
    """The checked source of a sampler: the ctypes view, what keeps its tensors alive, its sizes."""

    def __init__(self, src, k=None):
        sd = src.state_dict() if hasattr(src, "state_dict") else src
        missing = [f for f in VIEW_FIELDS if f not in sd]
        if missing:
            raise ValueError("rollout source lacks %s" % ", ".join(missing))
        fr = sd["frames"]
        if not isinstance(fr, torch.Tensor) or fr.dim() not in (3, 4):
            raise ValueError("frames must be a (T, N, 15) or (world, T, N, 15) tensor")
        lead = tuple(fr.shape[:-1])
        W, T, N = ((1,) + lead) if fr.dim() == 3 else lead
        wrap = (lambda *s: s) if fr.dim() == 3 else (lambda *s: (W,) + s)
        if k is None:
            k = getattr(src, "k", None) or sd["obs0"].shape[-2]
        k = int(k)
        if not 1 <= k <= 64 or min(W, T, N) < 1:
            raise ValueError("stack_k must be in 1..64 and world, n_steps, n_envs >= 1")
        shapes = {"frames": wrap(T, N, F16_OBS_DIM), "obs0": wrap(N, k, F16_OBS_DIM), "actions": wrap(T, N, 4)}
        if fr.device.type != "cuda":
            raise ValueError("the minibatch sampler runs on the GPU (f16env_rollout_minibatch); the rollout is on %s"
                             % fr.device)
        for f in VIEW_FIELDS:
            need_tensor(sd[f], shapes.get(f, wrap(T, N)), torch.float32, fr.device, f, 16 if f == "actions" else 4)
        self.device, self.k, self.total = fr.device, k, W * T * N
        self.tensors = tuple(sd[f] for f in VIEW_FIELDS)
        self.view = RolloutView(W, k, T, N, *(x.data_ptr() for x in self.tensors))
        self.ref = ctypes.byref(self.view)


def _check_samples(out, batch: int, k: int, device):
    shapes = ((batch, k, F16_OBS_DIM), (batch, 4), (batch,), (batch,), (batch,), (batch,))
    if not isinstance(out, tuple) or len(out) != 6:
        raise ValueError("out must be a RolloutSamples of six tensors")
    for x, shape, name in zip(out, shapes, RolloutSamples._fields):
        need_tensor(x, shape, torch.float32, device, "out." + name, 16 if len(shape) > 1 else 4)


def rollout_minibatch(src, indices, k: Optional[int] = None, out: Optional[RolloutSamples] = None) -> RolloutSamples:
    """RolloutBuffer._get_samples (buffers.py:508-521) for one batch of flat indices, one launch of
    f16env_rollout_minibatch on the current stream.
    src: a full DeviceRolloutBuffer, its state_dict(), or the dict gather_to_rank0 returns (world
    from frames.dim(); the rank-major tensors are used in place, no env_major copy); k the stack
    depth (default: the buffer's, or obs0's). indices: int64 tensor on the device, flat_index order.
    Row b of every output is transition indices[b]; observations are rebuilt per sample by
    rebuild_observations' rule. An index outside [0, world * n_envs * n_steps) reads nothing and
    yields a row of NaN (DeviceRolloutBuffer.get range-checks its caller's indices instead).
    out: caller-owned RolloutSamples to write into. With `out` given the call allocates nothing and
    never synchronises, so it can be captured in a HIP graph."""
    v = src if isinstance(src, _View) else _View(src, k)
    batch = indices.numel() if isinstance(indices, torch.Tensor) else 0
    need_tensor(indices, (batch,), torch.int64, v.device, "indices", 8)
    if out is None:
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=v.device)  # noqa: E731
        out = RolloutSamples(e(batch, v.k, F16_OBS_DIM), e(batch, 4), e(batch), e(batch), e(batch), e(batch))
    else:
        _check_samples(out, batch, v.k, v.device)
    sampler = fn("f16env_rollout_minibatch")
    if batch:
        check(sampler(stream_ptr(v.device), v.ref, batch, indices.data_ptr(), *(x.data_ptr() for x in out)),
              "f16env_rollout_minibatch")
    return out


def _minibatches(src, k, total: int, device, batch_size, indices, generator):
    """The checks of a sampling pass, made when it is asked for; then its generator."""
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError("batch_size must be >= 1")
    if indices is not None:
        perm = torch.as_tensor(indices)
        if perm.dim() != 1 or perm.dtype not in (torch.int64, torch.int32):
            raise ValueError("indices must be a 1-D integer array")
        if perm.numel():
            lo, hi = (int(x) for x in torch.aminmax(perm))
            if lo < 0 or hi >= total:
                raise ValueError("indices must lie in [0, %d), got [%d, %d]" % (total, lo, hi))
    view = _View(src, k)
    if indices is None:
        perm = torch.randperm(total, device=device, generator=generator)
    else:
        perm = perm.to(device=device, dtype=torch.int64).contiguous()
    step = perm.numel() if batch_size is None else int(batch_size)

    def gen():
        for i in range(0, perm.numel(), max(1, step)):
            yield rollout_minibatch(view, perm[i:i + step])
    return gen()


def minibatches(gathered: Dict[str, torch.Tensor], k: Optional[int] = None, batch_size: Optional[int] = None,
                indices=None, generator=None):
    """DeviceRolloutBuffer.get over the dict gather_to_rank0 returns on rank 0: one shuffled pass
    over all world * n_envs * n_steps transitions, the rank-major tensors read in place."""
    fr = gathered["frames"]
    return _minibatches(gathered, k, int(fr.numel() // F16_OBS_DIM), fr.device, batch_size, indices, generator)
