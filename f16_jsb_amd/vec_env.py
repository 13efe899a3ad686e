"""The drop-in boundary: what a user of the reference touches, over one ``F16Envs`` handle (env.py).

``F16VecEnv``       -- the reference's VecEnv boundary
                       (stable_baselines3/common/vec_env/base_vec_env.py:50-357 VecEnv ABC,
                       dummy_vec_env.py:56-83 auto-reset / info contract, monitor.py:85-111
                       episode stats), returning numpy like DummyVecEnv.
``F16GymVectorEnv`` -- gymnasium.vector.VectorEnv, autoreset SAME_STEP.
``F16GymEnv``       -- one env with gym.make("JSBSim-v0")'s single-env surface.
``make_gym_env`` / ``make_gym_vector_env`` -- the gymnasium entry points of "JSBSim-v0".
In numpy mode the outputs reach the host through a staging object (host_staging.py).
"""
from __future__ import annotations

import time
from copy import deepcopy
from typing import Any, Optional, Sequence

import numpy as np
import torch

from . import spaces
from .abi import F16C_GOAL, F16C_STEP
from .env import F16Envs, reference_goal
from .host_staging import _HostStaging, _staging
from .layouts import StepOut


def _optional_class(module: str, name: str):
    """A base class from an optional dependency (stable_baselines3 / gymnasium), or None."""
    try:
        mod = __import__(module, fromlist=[name])
        return getattr(mod, name)
    except Exception:  # noqa: BLE001 - absent or broken: the duck-typed surface is used
        return None


# stable_baselines3/common/base_class.py:215 accepts an env as-is only when
# isinstance(env, VecEnv); gymnasium learners check gymnasium.Env / gymnasium.vector.VectorEnv.
# When those libraries are importable the facades below ARE subclasses of their ABCs.
SB3VecEnv = _optional_class("stable_baselines3.common.vec_env.base_vec_env", "VecEnv")
GymEnv = _optional_class("gymnasium", "Env")
GymVectorEnv = _optional_class("gymnasium.vector", "VectorEnv")


def _bases(*classes):
    return tuple(c for c in classes if c is not None) or (object,)


class _ReadOnlyInfo(dict):
    """The info dict of every lane that did not finish its step: {"TimeLimit.truncated": False}
    (dummy_vec_env.py:56-73 through TimeLimit + Monitor). ONE shared, immutable instance per
    step instead of N fresh dicts; lanes that finished get fresh dicts of their own."""

    def _ro(self, *a, **k):
        raise TypeError("info of a lane that did not finish is shared and read-only")

    __setitem__ = __delitem__ = update = pop = popitem = clear = setdefault = _ro  # type: ignore[assignment]

    def copy(self):
        return dict(self)

    def __deepcopy__(self, memo):
        return dict(self)


_NOT_DONE_INFO = _ReadOnlyInfo({"TimeLimit.truncated": False})


# -- what the two vector facades share --------------------------------------------------------------
def seeded_goals(seeds) -> Optional[np.ndarray]:
    """Reset goals for per-lane seeds: None when no lane is seeded, else (N, 3) float32 with the
    reference's numpy stream (reference_goal, jsbsim_gym.py:312-323) in the seeded rows and NaN in
    the others, which draw the device goal -- all in ONE reset, so each lane's episode counter
    advances once."""
    if all(s is None for s in seeds):
        return None
    goals = np.full((len(seeds), 3), np.nan, np.float32)
    for i, s in enumerate(seeds):
        if s is not None:
            goals[i] = reference_goal(s)
    return goals


def _open(self, envs, num_envs, return_numpy, copy_obs, **kw):
    """The attributes both vector facades have: the handle (`envs`, or a new one that steps in the
    windowed layout when observations go to the host anyway -- no per-step stack rewrite: 16.9 vs
    27.8 us at K = 10, 65 536 envs -- and in dense (N, K, 15) buffers in device mode, unless the
    caller names a layout), its numpy-mode staging and the episode clock."""
    if envs is None:
        kw.setdefault("obs_layout", "window" if return_numpy else "contiguous")
        envs = F16Envs(num_envs, **kw)
    self.envs, self.num_envs = envs, envs.n
    self.render_mode = None
    self.return_numpy, self.copy_obs = bool(return_numpy), bool(copy_obs)
    self._host = _staging(envs, self.copy_obs) if self.return_numpy else None
    self._t_start = time.time()


def _episode_stats(self, idx):
    """Of the lanes idx that finished: terminal observations, episode returns and lengths, and the
    seconds since the last reset(). The returns are still to be rounded to 6 places, by each facade
    in its own way: the returns are short decimals, a tie at the 7th place is common (6 of 2056
    episodes measured), and there Monitor's round() (monitor.py:96-109, F16VecEnv) and np.round
    (F16GymVectorEnv) part ways."""
    return (*self._host.done_rows(idx), round(time.time() - self._t_start, 6))


def _t_where(mask, x, other):
    if not isinstance(x, torch.Tensor):
        x = torch.full(mask.shape, float(x), device=mask.device)
    return torch.where(mask, x, torch.as_tensor(other, dtype=x.dtype, device=x.device))


class F16VecEnv(*_bases(SB3VecEnv)):
    """Vectorised drop-in for ``DummyVecEnv([lambda: Monitor(gym.make("JSBSim-v0"))] * N)``.

    Honours the SB3 VecEnv contract (base_vec_env.py:50-357): ``reset() -> obs``,
    ``step_async/step_wait -> (obs, rews, dones, infos)``, auto-reset with
    ``infos[i]["terminal_observation"]`` and ``infos[i]["TimeLimit.truncated"]``
    (dummy_vec_env.py:56-73), Monitor's ``infos[i]["episode"] = {r, l, t}``
    (monitor.py:96-109), ``seed()`` applied at the next reset (:292-309). When
    stable_baselines3 is importable this class IS a ``VecEnv`` subclass, so
    ``BaseAlgorithm._wrap_env`` (base_class.py:215) takes it as-is.

    Numpy mode (default, what SB3 consumes): the handle steps in the windowed layout and the
    host keeps a pinned mirror of its frame histories, so per step only the new frame slots
    (2 x N x 64 B) and the packed rewards/flags cross PCIe, one stream sync (_HostWindow); the
    obs returned by reset() and step() is a strided (N, K, 15) numpy view of that mirror, valid
    until the step after next (SB3 stores it one step later). ``copy_obs=True`` returns owned
    contiguous copies instead (whole-observation D2H per step, _HostStaging), for consumers that
    keep observations longer. Infos of lanes that did not finish share one read-only dict.
    ``return_numpy=False`` keeps everything on the GPU (infos is then None: the caller reads the
    ``last_step`` device tensors). ``envs=`` wraps an existing handle instead of creating one."""

    metadata = {"render_modes": []}

    def __init__(self, num_envs: int = 1, stack_k: int = 10, device=None, seed: int = 0,
                 return_numpy: bool = True, env_id_base: int = 0, envs=None, copy_obs: bool = False, **kw):
        _open(self, envs, num_envs, return_numpy, copy_obs, stack_k=stack_k, device=device, seed=seed,
              env_id_base=env_id_base, **kw)
        n, c = self.num_envs, self.envs.cfg
        self._attrs: dict = {}
        # constants of the reference env (jsbsim_gym.py:103-118) that get_attr answers
        self._const = {"num_stacked_frames": self.envs.k, "max_episode_steps": int(c.max_steps),
                       "down_sample": int(c.down_sample), "dg": float(c.dg_m)}
        obs_space, act_space = spaces.observation_space(self.envs.k), spaces.action_space()
        if SB3VecEnv is not None:
            SB3VecEnv.__init__(self, n, obs_space, act_space)  # base_vec_env.py:59-94
        else:
            self.observation_space, self.action_space = obs_space, act_space
            self.reset_infos: list = [{} for _ in range(n)]
            self._seeds: list = [None for _ in range(n)]
            self._options: list = [{} for _ in range(n)]
        self._actions = None
        self.last_step: Optional[StepOut] = None

    # -- VecEnv API -------------------------------------------------------------------------
    def reset(self):
        obs = self.envs.reset(goals=seeded_goals(self._seeds))
        self._seeds = [None for _ in range(self.num_envs)]
        self._options = [{} for _ in range(self.num_envs)]
        self.reset_infos = [{} for _ in range(self.num_envs)]
        self._t_start = time.time()
        return self._host.reset_obs(obs) if self.return_numpy else obs

    def step_async(self, actions) -> None:
        self._actions = actions

    def step_wait(self):
        if not self.return_numpy:
            out = self.envs.step(self._actions)
            self.last_step = out
            return out.obs, out.rew, (out.terminated | out.truncated).bool(), None
        out = self.envs.step(self._host.actions_to_device(self._actions))
        self.last_step = out
        obs, rew, term_u8, trunc_u8 = self._host.step_outputs(out.obs)
        dones = (term_u8 | trunc_u8).astype(bool)
        infos = [_NOT_DONE_INFO] * self.num_envs
        idx = np.flatnonzero(dones)
        if idx.size:
            tobs, eret, elen, t = _episode_stats(self, idx)
            for j, i in enumerate(idx.tolist()):
                info = {"TimeLimit.truncated": bool(trunc_u8[i] and not term_u8[i]),
                        "terminal_observation": tobs[j],
                        "episode": {"r": round(float(eret[j]), 6), "l": int(elen[j]), "t": t}}
                if term_u8[i] & 2:  # NaN guard quarantine (nan_guard=True)
                    info["nonfinite"] = True
                infos[i] = info
        return obs, rew.copy(), dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self) -> None:
        self.envs.close()

    def seed(self, seed: Optional[int] = None) -> Sequence[Optional[int]]:
        if seed is None:
            seed = int(np.random.randint(0, np.iinfo(np.uint32).max, dtype=np.uint32))
        self._seeds = [seed + idx for idx in range(self.num_envs)]
        return self._seeds

    def set_options(self, options=None) -> None:
        if options is None:
            options = {}
        self._options = deepcopy([options] * self.num_envs) if isinstance(options, dict) else deepcopy(options)

    def _indices(self, indices):
        if indices is None:
            return range(self.num_envs)
        if isinstance(indices, int):
            return [indices]
        return indices

    def get_attr(self, attr_name: str, indices=None) -> list:
        idx = list(self._indices(indices))
        if attr_name in self._attrs:
            return [self._attrs[attr_name] for _ in idx]
        if attr_name in ("render_mode", "observation_space", "action_space", "metadata"):
            return [getattr(self, attr_name) for _ in idx]
        if attr_name == "spec":
            return [None for _ in idx]
        if attr_name in self._const:
            return [self._const[attr_name] for _ in idx]
        # per-lane attributes of the reference env (jsbsim_gym.py:103-118), read from the device state
        if attr_name == "state":  # jsbsim_gym.py:181-193: newest frame's 12 state values
            rows = self.envs.obs[:, -1, :12].index_select(0, self.envs.torch.as_tensor(idx, device=self.envs.device))
            return list(rows.cpu().numpy())
        if attr_name in ("current_step", "goal"):
            st = self.envs.get_state().cpu().numpy()
            if attr_name == "current_step":
                return [int(st[i, F16C_STEP]) for i in idx]
            return [st[i, F16C_GOAL:F16C_GOAL + 3].astype(np.float32) for i in idx]
        raise AttributeError(attr_name)

    def set_attr(self, attr_name: str, value: Any, indices=None) -> None:
        self._attrs[attr_name] = value

    def env_method(self, method_name: str, *method_args, indices=None, **method_kwargs) -> list:
        """The single-env methods that make sense on device lanes: render (no renderer: None,
        like an env without render_mode), get_wrapper_attr (gymnasium >= 1.0 attribute access),
        reset (the indexed lanes, new goals from the device stream)."""
        idx = list(self._indices(indices))
        if method_name == "render":
            return [None for _ in idx]
        if method_name == "get_wrapper_attr":
            return self.get_attr(method_args[0], idx)
        if method_name == "reset":
            mask = np.zeros(self.num_envs, np.uint8)
            mask[idx] = 1
            full = self.envs.reset(mask=mask)
            if self._host is not None:  # the host mirror takes the new windows
                self._host.reset_obs(full)
            obs = full[self.envs.torch.as_tensor(idx, device=self.envs.device)]
            return [(o, {}) for o in obs.cpu().numpy()]
        raise AttributeError("F16VecEnv lanes have no per-env method %r" % method_name)

    def env_is_wrapped(self, wrapper_class, indices=None) -> list:
        name = getattr(wrapper_class, "__name__", str(wrapper_class))
        # Monitor / TimeLimit / PositionReward semantics are built into the kernel
        wrapped = name in ("Monitor", "TimeLimit", "PositionReward")
        return [wrapped for _ in self._indices(indices)]

    def has_attr(self, attr_name: str) -> bool:
        try:
            self.get_attr(attr_name, 0)
            return True
        except AttributeError:
            return False

    def get_images(self):
        raise NotImplementedError("rendering is out of scope (SURVEY.md component #9)")

    def render(self, mode: Optional[str] = None):
        return None

    @property
    def unwrapped(self):
        return self


class F16GymVectorEnv(*_bases(GymVectorEnv)):
    """gymnasium.vector.VectorEnv surface over the same kernel (the north star's "Gymnasium
    VectorEnv step()/reset()"), for gymnasium-native learners; a VectorEnv subclass when
    gymnasium is importable (registered as "JSBSim-v0"'s vector entry point,
    f16_jsb_amd/__init__.py). Autoreset mode SAME_STEP -- what the kernel does: a lane that
    terminates or truncates returns its reset observation in the same step, and

      infos["final_obs"] / infos["_final_obs"]   final (K,15) observation / mask
      infos["episode"] = {"r", "l", "t"}, infos["_episode"]   (RecordEpisodeStatistics keys)

    are filled for the finished lanes (gymnasium's vector-info convention: a value array plus a
    "_key" boolean mask). ``reset(seed=s)`` seeds env i with s + i (the reference's
    default_rng(seed) goal, jsbsim_gym.py:312-323). Single-env semantics are jsbsim_gym.py's
    JSBSimEnv wrapped in TimeLimit(1200) and PositionReward(1e-2) (jsbsim_gym.py:537-545).

    Numpy mode returns observations as strided views of a pinned host mirror of the windowed
    handle's frame histories (_HostWindow): an obs array stays valid until the step after next
    (the next step leaves it intact, the one after overwrites it). A consumer that keeps
    observations longer passes ``copy_obs=True`` (contiguous copies; whole-observation
    device-to-host copies per step). ``infos["final_obs"]`` is always a copy."""

    metadata = {"autoreset_mode": "SameStep", "render_modes": []}

    def __init__(self, num_envs: int = 1, stack_k: int = 10, device=None, seed: int = 0,
                 return_numpy: bool = True, envs=None, copy_obs: bool = False, **kw):
        _open(self, envs, num_envs, return_numpy, copy_obs, stack_k=stack_k, device=device, seed=seed, **kw)
        self.single_observation_space = spaces.observation_space(self.envs.k)
        self.single_action_space = spaces.action_space()
        self.observation_space = spaces.batch_space(self.single_observation_space, self.num_envs)
        self.action_space = spaces.batch_space(self.single_action_space, self.num_envs)
        self.spec = None
        self.closed = False

    def reset(self, *, seed=None, options=None):
        goals = None
        if seed is not None:
            seeds = [seed + i for i in range(self.num_envs)] if isinstance(seed, int) else list(seed)
            if len(seeds) != self.num_envs:
                raise ValueError("need one seed per env")
            goals = seeded_goals(seeds)
        obs = self.envs.reset(goals=goals)
        self._t_start = time.time()
        return (self._host.reset_obs(obs) if self.return_numpy else obs), {}

    def step(self, actions):
        if not self.return_numpy:
            out = self.envs.step(actions)
            term, trunc = out.terminated.bool(), out.truncated.bool()
            done = term | trunc
            infos = {}
            if bool(done.any()):
                t = round(time.time() - self._t_start, 6)
                infos["final_obs"] = out.terminal_obs.clone()
                infos["_final_obs"] = done
                infos["episode"] = {"r": _t_where(done, out.ep_return, 0.0), "l": _t_where(done, out.ep_len, 0),
                                    "t": _t_where(done, t, 0.0)}
                infos["_episode"] = done
            return out.obs, out.rew, term, trunc, infos
        out = self.envs.step(self._host.actions_to_device(actions))
        obs, rew, term_u8, trunc_u8 = self._host.step_outputs(out.obs)
        term, trunc = term_u8.astype(bool), trunc_u8.astype(bool)
        done = term | trunc
        infos = {}
        idx = np.flatnonzero(done)
        if idx.size:
            tobs, eret, elen, t = _episode_stats(self, idx)
            final = np.zeros_like(obs)
            final[idx] = tobs
            r = np.zeros(self.num_envs)
            r[idx] = np.round(eret, 6)
            ln = np.zeros(self.num_envs, np.int32)
            ln[idx] = elen
            infos["final_obs"] = final
            infos["_final_obs"] = done
            infos["episode"] = {"r": r, "l": ln, "t": np.where(done, t, 0.0)}
            infos["_episode"] = done
        return obs, rew.copy(), term, trunc, infos

    def close(self, **kwargs):
        if not self.closed:
            self.envs.close()
            self.closed = True

    def render(self):
        return None

    @property
    def unwrapped(self):
        return self


class F16GymEnv(*_bases(GymEnv)):
    """ONE env with the single-env gymnasium surface of ``gym.make("JSBSim-v0")``
    (jsbsim_gym.py:537-545: JSBSimEnv wrapped in PositionReward(1e-2), TimeLimit(1200)) over a
    one-lane handle: ``reset(seed, options) -> (obs (K,15), {})`` with the default_rng(seed)
    goal of jsbsim_gym.py:312-323 (seed None: the device goal stream), ``step(action) ->
    (obs, reward, terminated, truncated, {})``, no auto-reset (the caller resets, as with the
    reference). A gymnasium.Env subclass when gymnasium is importable; the entry point
    "JSBSim-v0" is registered to (f16_jsb_amd/__init__.py), so an unchanged train.py gets a
    GPU-backed env from gym.make -- one env, SB3 then wraps it in Monitor + DummyVecEnv as it
    does the reference's. For throughput use F16VecEnv."""

    metadata = {"render_modes": []}

    def __init__(self, stack_k: int = 10, device=None, seed: int = 0, envs=None, **kw):
        self.envs = envs if envs is not None else F16Envs(1, stack_k=stack_k, device=device, seed=seed,
                                                          autoreset=False, **kw)
        self.observation_space = spaces.observation_space(self.envs.k)
        self.action_space = spaces.action_space()
        self.render_mode = None
        self._host = _HostStaging(self.envs, ring=2)

    def reset(self, *, seed=None, options=None):
        if GymEnv is not None:
            GymEnv.reset(self, seed=seed)  # gymnasium's np_random seeding (jsbsim_gym.py:302)
        goals = None if seed is None else reference_goal(seed)[None]
        return self._host.reset_obs(self.envs.reset(goals=goals))[0].copy(), {}

    def step(self, action):
        out = self.envs.step(self._host.actions_to_device(np.asarray(action, np.float32).reshape(1, 4)))
        obs, rew, term, trunc = self._host.step_outputs(out.obs)
        return obs[0].copy(), float(rew[0]), bool(term[0]), bool(trunc[0]), {}

    def render(self):
        return None

    def close(self):
        self.envs.close()

    @property
    def unwrapped(self):
        return self


def make_gym_env(**kw) -> F16GymEnv:
    """gymnasium entry point of "JSBSim-v0" (jsbsim_gym.py:537-545 wrap_jsbsim counterpart)."""
    kw.pop("root", None)  # JSBSimEnv(root=...) names a JSBSim data directory: nothing to load here
    return F16GymEnv(**kw)


def make_gym_vector_env(num_envs: int = 1, **kw) -> F16GymVectorEnv:
    """gymnasium vector entry point of "JSBSim-v0" (gymnasium.make_vec)."""
    kw.pop("root", None)
    return F16GymVectorEnv(num_envs=num_envs, **kw)
