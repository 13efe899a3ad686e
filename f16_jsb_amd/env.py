"""Host side of the MI355X F-16 environment: the handle.

``F16Envs``   -- thin owner of one libf16env handle: device tensors in, device tensors out
                 (the throughput path; no per-step allocation, no host sync); what depends on
                 the observation layout is in layouts.py.
``reference_goal`` -- jsbsim_gym.py:312-323 with numpy's default_rng(seed), used for
                 seeded resets so seeded goals match the reference bit for bit.
The drop-in facades over a handle (F16VecEnv, F16GymVectorEnv, F16GymEnv) are in vec_env.py, the
host staging of their numpy mode in host_staging.py; the three class names still resolve here.
"""
from __future__ import annotations

import ctypes
from functools import partial
from typing import Optional

import numpy as np

from ._lib import F16EnvError, check, lib
from .abi import (RolloutSlot, F16C_N, F16_IC_N, F16_OBS_DIM, F16_FLAG_NAN_GUARD, F16_FLAG_NO_AUTORESET,
                  F16_FLAG_OBS_CHECK, F16_SLOT_CLIP, EnvConfig, algorithmic_bytes_per_env_step, config_default)
from .buffers import need_tensor, split_step_flags, step_flags_bytes
from .layouts import U64, StepOut, _ContiguousLayout, _default_history, _ptr, _WindowLayout, as_act  # noqa: F401


def reference_goal(seed) -> np.ndarray:
    """Goal of JSBSimEnv.reset(seed) (jsbsim_gym.py:312-323), float32 (x, y, alt)."""
    rng = np.random.default_rng(seed)
    distance_m = rng.uniform(1000.0, 10000.0)
    bearing_rad = rng.uniform(0, 2 * np.pi)
    altitude_m = rng.uniform(1000.0, 4000.0)
    g = np.zeros(3, dtype=np.float32)
    g[0] = distance_m * np.cos(bearing_rad)
    g[1] = distance_m * np.sin(bearing_rad)
    g[2] = altitude_m
    return g


class F16Envs:
    """N F-16 envs on one GPU behind the C ABI. All tensors are torch tensors on ``device``. The
    layout object chosen at creation (layouts.py) owns the observation buffers and their calls."""

    def __init__(self, n_envs: int, stack_k: int = 10, device=None, seed: int = 0,
                 env_id_base: int = 0, max_steps: int = 1200, down_sample: int = 4,
                 autoreset: bool = True, ic=None, nan_guard: bool = False, obs_check: bool = False,
                 obs_layout: str = "contiguous", history: int = 0, window_order: str = "position",
                 fused_features: bool = False, fused_poses: bool = False, **cfg_kw):
        """obs_layout "contiguous": observations in two ping-pong (N, K, 15) buffers (f16env_step).
        obs_layout "window": observations are (N, K, 15) views of two per-env frame histories of
        `history` positions of 64-B frame slots, position-major [T][N][16] (f16env_step_window:
        only the new frame is written per step, one contiguous block per position; view strides
        (16, N*16, 1)); history 0 = max(256, 2K) (a restart every T-K+1 steps); window_order
        "env" keeps the histories env-major [N][T][16] instead (strides (T*16, 16, 1)). Both
        layouts give identical values and the same validity (an observation stays valid until the
        step after next). A consumer that needs a flat (N, K*15) array copies the window (reshape);
        the features kernel (f16_jsb_amd.features) reads it in place.
        fused_features (windowed layout): every step also keeps the policy features of both windows
        (obs_features(), features.py:37-67 per frame) in its own epilogue (f16env_window_step_ex,
        F16_STEP_FEATURE_WINDOW), no second launch; obs_features() is then a view. Off by default:
        the plain step's instance carries none of that code.
        fused_poses (windowed layout): every step also writes the render/telemetry pose of the
        returned observation's newest frame (poses(), telemetry.poses of obs[:, -1], the same
        bits) in its epilogue (f16env_window_step_ex, F16_STEP_POSES): no second launch."""
        import torch

        if not torch.cuda.is_available():
            raise F16EnvError("F16Envs needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.torch = torch
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise F16EnvError("device must be a cuda (ROCm) device, got %s" % self.device)
        self.n, self.k = n, k = int(n_envs), int(stack_k)
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        # the caller's current stream on this device (the raw handle: 0.03 us, where
        # torch.cuda.current_stream() builds a Stream object per call, ~1.7 us)
        raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        self._stream = partial(raw or (lambda i: torch.cuda.current_stream(i).cuda_stream), dev_index)
        flags = int(cfg_kw.pop("flags", 0)) | (0 if autoreset else F16_FLAG_NO_AUTORESET) \
            | (F16_FLAG_NAN_GUARD if nan_guard else 0) | (F16_FLAG_OBS_CHECK if obs_check else 0)
        self.cfg: EnvConfig = config_default(n_envs=n_envs, stack_k=stack_k, seed=seed, env_id_base=env_id_base,
                                             max_steps=max_steps, down_sample=down_sample, flags=flags, ic=ic, **cfg_kw)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().f16env_create(ctypes.byref(self.cfg), self.device.index or 0, ctypes.byref(h)), "f16env_create")
        self._h = h
        f32, dev = torch.float32, self.device
        # rewards (f32), terminated, truncated (u8) in ONE allocation, so a host-side consumer
        # (F16VecEnv's numpy mode) moves the three with a single device-to-host copy
        self.step_flags = torch.zeros(step_flags_bytes(n), dtype=torch.uint8, device=dev)
        self.rew, self.term, self.trunc = split_step_flags(self.step_flags, n, f32)
        self.ep_return = torch.zeros(n, dtype=torch.float64, device=dev)
        self.ep_len = torch.zeros(n, dtype=torch.int32, device=dev)
        self._act = torch.zeros((n, 4), dtype=f32, device=dev)
        self._last_episode_starts = None  # (written by rollout.collect_rollout: the next rollout's episode_starts[0])
        self.fused_features, self.fused_poses = bool(fused_features), bool(fused_poses)
        self.window = obs_layout == "window"
        # a host mirror can follow this handle one frame slot per step (host_staging._HostWindow)
        self.mirrors_by_slot = self.window and window_order == "position"
        try:
            if obs_layout not in ("contiguous", "window"):
                raise ValueError("obs_layout must be 'contiguous' or 'window'")
            self._layout = lay = (_WindowLayout if self.window else _ContiguousLayout)(
                h, self._stream, torch, dev, n, k, self.cfg,
                (self.rew, self.term, self.trunc, self.ep_return, self.ep_len), history=history,
                window_order=window_order, fused_features=self.fused_features, fused_poses=self.fused_poses)
        except Exception:
            self.close()
            raise
        if self.window:
            self.T, self.feature_window_calls = lay.T, lay.derived.calls
        # the layout's step entry points, bound here: step() pays no attribute hop for them
        self._step_plain, self._step_rollout_raw = lay.step, lay.step_slot

    obs = property(lambda self: self._layout.obs)
    terminal_obs = property(lambda self: self._layout.terminal_obs)  # (windowed: the other history's window)

    def new_frame_slots(self):
        """Windowed layout: the last step's two new (N, 16) slot blocks, of the current and of the
        other history."""
        return self._layout.new_slots()

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            lib().f16env_destroy(h)
            h.value = None  # (the layout holds the same object: its calls are refused from here on)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def waves_per_simd(self) -> int:
        """Occupancy the step kernel variant of this handle is built for (1 or 2)."""
        return self._layout.waves_per_simd

    @property
    def step_kernel_name(self) -> str:
        """The step kernel instance this handle launches (the symbol rocprofv3 reports)."""
        return lib().f16env_step_kernel_name(self._h).decode()

    @property
    def state_bytes_per_env(self) -> int:
        return int(lib().f16env_state_bytes_per_env())

    def algorithmic_bytes_per_env_step(self) -> int:
        """Bytes per env step of this handle's layout (abi.algorithmic_bytes_per_env_step)."""
        return algorithmic_bytes_per_env_step(self.k, self.state_bytes_per_env, self._layout.name)

    def stack_bytes_per_env_step(self) -> int:
        """SURVEY.md 8(d)'s B(K): the bytes of the same step with the stack materialised."""
        return algorithmic_bytes_per_env_step(self.k, self.state_bytes_per_env)

    # --------------------------------------------------------------------------------------
    def reset(self, mask=None, goals=None, ic=None):
        """Reset lanes (mask: bool/uint8 (N,) or None=all). goals (N,3) float32 or None
        (device RNG); ic (N, F16_IC_N) float64 or None (config IC). Returns obs (N,K,15)."""
        t = self.torch
        m = None if mask is None else t.as_tensor(mask, device=self.device).to(t.uint8).contiguous()
        g = None if goals is None else t.as_tensor(goals, device=self.device, dtype=t.float32).contiguous()
        c = None if ic is None else t.as_tensor(ic, device=self.device, dtype=t.float64).contiguous()
        for name, x, shape in (("mask", m, (self.n,)), ("goals", g, (self.n, 3)), ("ic", c, (self.n, F16_IC_N))):
            if x is not None and tuple(x.shape) != shape:
                raise ValueError("%s must be %s, got %s" % (name, shape, tuple(x.shape)))
        return self._layout.reset(_ptr(m), _ptr(g), _ptr(c))

    _as_act = as_act

    def step(self, actions, done_idx=None, n_done=None, features=None, seed=None, step=None) -> StepOut:
        """One env step for all lanes; ``actions`` (N,4) float32 device tensor (or host
        array, copied). Returns device tensors; obs alternates between two buffers.
        done_idx (N,) / n_done (1,) int32 device tensors receive the compacted list of lanes
        that finished (optional). features: an (N, K, 17) float32 device tensor that receives
        the policy features of the returned obs (features.py:37-67) in the same call.
        actions None with seed / step: the actions are drawn inside the step kernel from the
        sample_actions(seed, step) stream (bit-identical to step(sample_actions(seed, step)),
        without the sampling launch and the action read; windowed layout: f16env_window_step_ex,
        contiguous: the rollout-slot step with an empty slot)."""
        if actions is None:
            if seed is None or step is None:
                raise ValueError("actions=None needs seed and step (the in-kernel sample_actions stream)")
            if done_idx is not None or n_done is not None or features is not None:
                raise ValueError("in-kernel actions: no done list / features argument")
            return self._layout.step_ex(None, int(seed), int(step))
        if features is not None:
            return self.step_rollout(0, 0, features=features, policy_actions=actions)
        act = self._as_act(actions)
        if done_idx is None and n_done is None:  # the common case: one ctypes call on cached addresses
            return self._step_plain(act)
        if done_idx is None or n_done is None:
            raise ValueError("done_idx and n_done go together")
        need_tensor(done_idx, (self.n,), self.torch.int32, self.device, "done_idx")
        need_tensor(n_done, (1,), self.torch.int32, self.device, "n_done")
        return self._step_plain(act, done_idx, n_done)

    def step_rollout(self, seed: int, step: int, frame=None, actions=None, rewards=None, next_start=None,
                     policy_actions=None, features=None, next_frame=None, clip: bool = False) -> StepOut:
        """One env step that also writes one rollout-buffer slot, with no extra launch
        (f16env_step_rollout / f16env_window_step_rollout): the actions, the rewards and the next
        slot's episode starts, and one frame of the frame-deduplicated log -- the contiguous
        layout writes `frame` (the newest frame of the observation acted on), the windowed layout
        `next_frame` (the newest frame of the returned observation, i.e. the next slot's frame).
        policy_actions None: actions drawn in-kernel from the sample_actions(seed, step) stream
        (bit-identical). clip: the env steps np.clip(policy_actions, low, high) over the action Box
        (on_policy_algorithm.py:216) while `actions` receives policy_actions unclipped (:247-254)."""
        n, f32 = self.n, self.torch.float32
        act = None if policy_actions is None else self._as_act(policy_actions, "policy_actions")
        for name, x, shape in (("frame", frame, (n, F16_OBS_DIM)), ("next_frame", next_frame, (n, F16_OBS_DIM)),
                               ("actions", actions, (n, 4)), ("rewards", rewards, (n,)),
                               ("next_start", next_start, (n,)), ("features", features, (n, self.k, 17))):
            need_tensor(x, shape, f32, self.device, name, optional=True)
        slot = RolloutSlot(int(seed) & U64, int(step) & U64, _ptr(frame), _ptr(actions), _ptr(rewards),
                           _ptr(next_start), _ptr(features), _ptr(next_frame), F16_SLOT_CLIP if clip else 0, 0)
        return self._layout.step_slot_checked(slot, _ptr(act))

    # _step_rollout_raw(slot, act_ptr), bound in __init__: step_rollout with a prepared RolloutSlot and
    # action address and no argument checks -- collect_rollout validates its buffers once per rollout
    # and moves the slot's row addresses itself (the per-step host cost is the launch, not the checks)

    def rollout_random(self, seed: int, step0: int, n_steps: int, frames, actions, rewards, next_start,
                       last_start) -> None:
        """n_steps env steps in ONE launch under the uniform random policy (f16env_rollout_random /
        f16env_window_rollout_random: actions from the sample_actions(seed, step0 + t) stream,
        state kept on-chip): writes the rollout slots frames (T, N, 15) (frames[t] = newest frame
        of the observation step t acts on), actions (T, N, 4), rewards (T, N), next_start (T-1, N)
        (episode starts of slots 1..T-1) and last_start (N,), and leaves the env at its
        observation after the last step (self.obs). Bit-identical to n_steps step_rollout calls.
        Any stack_k and mode (cfg5: random ICs + gusts). Windowed layout: the final observation
        is written into both histories at a window beside the current one (when no such window
        fits in the history, the current windows are first moved to its front); no terminal
        observation is kept for the last step's finished lanes."""
        T, n, f32 = int(n_steps), self.n, self.torch.float32
        for name, x, shape in (("frames", frames, (T, n, F16_OBS_DIM)), ("actions", actions, (T, n, 4)),
                               ("rewards", rewards, (T, n)), ("last_start", last_start, (n,))):
            need_tensor(x, shape, f32, self.device, name)
        need_tensor(next_start, (T - 1, n), f32, self.device, "next_start", optional=T == 1)
        self._layout.rollout_random(int(seed) & U64, int(step0) & U64, T, frames, actions, rewards, next_start, last_start)

    def profile_kernel(self, fn, launches: int, times: Optional[list] = None):
        """Run fn() (which issues `launches` steps) with the step kernel's own dispatch events
        recording each launch; returns (avg_ms, min_ms, launches timed). `times`, a list,
        receives each launch's (start, stop) in ms from the first launch's start."""
        L = lib()
        check(L.f16env_profile_begin(self._h, int(launches)), "f16env_profile_begin")
        fn()
        if times is not None:
            buf = (ctypes.c_double * (2 * int(launches)))()
            got = L.f16env_profile_times(self._h, buf, int(launches))
            if got < 0:
                check(got, "f16env_profile_times")
            times.extend((buf[2 * i], buf[2 * i + 1]) for i in range(got))
        avg, mn, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        check(L.f16env_profile_end(self._h, ctypes.byref(avg), ctypes.byref(mn), ctypes.byref(cnt)), "f16env_profile_end")
        return avg.value, mn.value, cnt.value

    def _count(self, what: str) -> int:
        c = ctypes.c_uint64()
        check(getattr(lib(), what)(self._h, self._stream(), ctypes.byref(c)), what)
        return int(c.value)

    @property
    def nonfinite_count(self) -> int:
        """Lanes quarantined by the NaN guard (nan_guard=True) since creation; waits for the
        handle's stream. A quarantined lane ended its step terminated (terminated == 3) with
        reward 0 and was reset."""
        return self._count("f16env_nonfinite_count")

    @property
    def obs_bounds_count(self) -> int:
        """Lane-steps since creation whose new observation frame had a finite value outside the
        observation space (obs_check=True; jsbsim_gym.py:268-285's warning, counted on the
        device). Waits for the handle's stream."""
        return self._count("f16env_obs_bounds_count")

    def get_state(self):
        s = self.torch.zeros((self.n, F16C_N), dtype=self.torch.float64, device=self.device)
        check(lib().f16env_get_state(self._h, self._stream(), _ptr(s)), "f16env_get_state")
        return s

    def set_state(self, canon):
        s = self.torch.as_tensor(canon, dtype=self.torch.float64, device=self.device).contiguous()
        if tuple(s.shape) != (self.n, F16C_N):
            raise ValueError("state must be (N, %d)" % F16C_N)
        check(lib().f16env_set_state(self._h, self._stream(), _ptr(s)), "f16env_set_state")
        self._layout.state_written()
        self.torch.cuda.current_stream(self.device).synchronize()

    def set_obs(self, obs):
        """Overwrite the current observation (window layout: both histories' windows, so the
        next step continues from it)."""
        self._layout.set_obs(self.torch.as_tensor(obs, dtype=self.torch.float32))

    def poses(self):
        """(N, 10) float32 render/telemetry poses of the current observation's newest frame
        (telemetry.poses(self.obs[:, -1]), JSBSimEnv.render, jsbsim_gym.py:381-415). A fused_poses
        handle's step writes them in its epilogue, so after such a step this is the bound buffer with
        no launch; otherwise (or after any other op) f16env_poses computes them. Valid until the next op."""
        return self._layout.poses()

    def obs_features(self):
        """(N, K, 17) float32 policy features of the current observation (features.py:37-67 per
        frame; LMA_features.py:757-765 over the stack), equal bit for bit to
        features.features(self.obs). Windowed layout: kept in two feature histories beside the
        frame histories ([T][N][17] per parity, position-major; the result is a view, valid
        until the first call after the next step, which writes the other parity's rows), so a
        call after each step transforms one frame per env (f16env_features_window_step) instead
        of K, and a rollout-slot step (step_rollout, collect_rollout) keeps them in its own
        epilogue (F16_SLOT_FEATURE_WINDOW: no launch here at all); layouts._Derived says when
        both whole windows are transformed instead. Contiguous layout: features(self.obs)."""
        return self._layout.obs_features()

    def trim(self, ic):
        t = self.torch
        c = t.as_tensor(ic, dtype=t.float64, device=self.device).contiguous()
        out = t.zeros_like(c)
        res = t.zeros((self.n, 3), dtype=t.float64, device=self.device)
        check(lib().f16env_trim(self._h, self._stream(), _ptr(c), _ptr(out), _ptr(res)), "f16env_trim")
        return out, res

    def sample_actions(self, seed: int, step: int, out=None, steps: int | None = None):
        """Uniform Box actions from the device Philox stream keyed by (seed, env id, step)
        (action_space.sample() per env, jsbsim_gym.py:143-148): (N, 4) for `step`, or with
        `steps` = T the (T, N, 4) batches of steps step .. step+T-1 in ONE launch
        (f16env_sample_actions_steps, bit-identical to T single calls)."""
        t = self.torch
        shape = (self.n, 4) if steps is None else (int(steps), self.n, 4)
        if out is None:
            out = t.empty(shape, dtype=t.float32, device=self.device)
        need_tensor(out, shape, t.float32, self.device, "out")
        fn = "f16env_sample_actions" if steps is None else "f16env_sample_actions_steps"
        check(getattr(lib(), fn)(self._h, self._stream(), int(seed) & U64, int(step) & U64, *shape[:-2], _ptr(out)), fn)
        return out


def __getattr__(name):  # the facades' old import path (lazy, as in __init__.py); nothing else is forwarded
    if name in ("F16VecEnv", "F16GymVectorEnv", "F16GymEnv"):
        from . import vec_env
        return getattr(vec_env, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
