"""Numpy mode of the facades (vec_env.py): pinned host buffers the outputs of a handle land in.

Two classes, one contract -- what a facade calls, whichever ``_staging`` chose:
  reset_obs(obs_dev) -> obs                         after a reset (whole or masked) of the handle
  step_outputs(obs_dev) -> (obs, rew, term, trunc)  after a step; one wait for the stream
  done_rows(idx) -> (terminal_obs, ep_return, ep_len)   of the lanes idx that finished the step
  actions_to_device(actions) -> the (N, 4) device tensor to step with
``_HostStaging`` copies the whole observation; ``_HostWindow`` mirrors a windowed handle's frame
histories and copies the new slots alone. Of the handle they use its public tensors, ``cfg`` and,
for the mirror, ``mirrors_by_slot`` / ``new_frame_slots()``; on a CPU device nothing is pinned
and nothing is waited for, so both run over the tests' stand-in handles.
"""
from __future__ import annotations

import numpy as np

from .abi import F16_FLAG_NO_AUTORESET, F16_OBS_DIM
from .buffers import split_step_flags
from .layouts import as_act


class _HostStaging:
    """Whole-observation copies, one stream sync per step. obs goes to a ring of `ring` pinned
    (N, K, 15) buffers -- the arrays a step returns stay valid for `ring` - 1 further steps (SB3
    copies obs into its buffers one step later: on_policy_algorithm.py:250-257,
    off_policy_algorithm.py _store_transition), or with `copy` are owned copies; rewards /
    terminated / truncated arrive by ONE copy of the handle's packed step_flags buffer."""

    def __init__(self, envs, ring: int = 3, copy: bool = False):
        t = envs.torch
        self.t, self.envs, self.copy = t, envs, copy
        self.pin = pin = envs.device.type == "cuda"
        n, k = envs.n, envs.k
        self.obs = [t.empty((n, k, F16_OBS_DIM), dtype=t.float32, pin_memory=pin) for _ in range(ring)]
        self.flags = t.empty(envs.step_flags.shape, dtype=t.uint8, pin_memory=pin)
        self.rew_term_trunc = split_step_flags(self.flags.numpy(), n, np.float32)  # (views: filled by each step)
        self.act = t.empty((n, 4), dtype=t.float32, pin_memory=pin)
        self.i = 0

    def actions_to_device(self, actions):
        """Host actions -> the handle's device action buffer through pinned staging; tensors on
        the device go through as_act (aligned float32 (N, 4) ones untouched)."""
        t, e = self.t, self.envs
        if isinstance(actions, t.Tensor):
            if actions.device == e.device and actions.numel() == e.n * 4:
                return as_act(e, actions.reshape(e.n, 4))
            actions = actions.detach().to("cpu", t.float32).numpy()
        a = np.asarray(actions, dtype=np.float32)
        if a.size != e.n * 4:
            raise ValueError("actions must hold (N, 4) = (%d, 4) values, got shape %s" % (e.n, a.shape))
        self.act.numpy()[...] = a.reshape(e.n, 4)
        e._act.copy_(self.act, non_blocking=True)
        return e._act

    def _wait(self):
        if self.pin:  # (a CPU handle's copies are done when they return)
            self.t.cuda.current_stream(self.envs.device).synchronize()

    def _obs_to_host(self, obs_dev, flags: bool):
        o = self.obs[self.i]
        self.i = (self.i + 1) % len(self.obs)
        o.copy_(obs_dev, non_blocking=True)
        if flags:
            self.flags.copy_(self.envs.step_flags, non_blocking=True)
        self._wait()
        return np.array(o.numpy()) if self.copy else o.numpy()

    def reset_obs(self, obs_dev):
        return self._obs_to_host(obs_dev, False)

    def step_outputs(self, obs_dev):
        return (self._obs_to_host(obs_dev, True), *self.rew_term_trunc)

    def done_rows(self, idx: np.ndarray):
        """terminal obs, episode return / length of the lanes in idx (small device gathers)."""
        e, t = self.envs, self.t
        i = t.as_tensor(idx, dtype=t.int64).to(e.device, non_blocking=True)
        return self._terminal_obs(idx, i), e.ep_return.index_select(0, i).cpu().numpy(), e.ep_len.index_select(0, i).cpu().numpy()

    def _terminal_obs(self, idx, i):
        return self.envs.terminal_obs.index_select(0, i).cpu().numpy()


class _HostWindow(_HostStaging):
    """Numpy mode over a windowed handle (the "window" layout, position-major): the host keeps
    a pinned mirror of the device's two frame histories, [2][Th][N][16], and per step copies
    only the step's new 64-B slot block of each (position p of both device histories: 2 x N x 64
    B, contiguous) instead of the whole (N, K, 15) observation (N x K x 60 B: 39 MB per step at
    65 536 envs, K = 10). The host then repeats what the windowed step kernel does to the
    windows of reset lanes (f16_step.h step_body, WIN): lanes reset by this step get K-1 copies of
    their reset frame in the current history's window, lanes reset by the previous step get
    the same fill from the other history (the kernel's FRESH fill). The observation returned is
    a strided numpy view (N, K, 15) of the current host history's window (strides 64 B, N x 64 B,
    4 B), valid until the step after next -- the device layout's guarantee, which SB3 needs
    (it stores obs one step later, on_policy_algorithm.py:247-254); the terminal observation is
    the other history's window, as on the device. The host ring has its own Th positions and
    moves its last K-1 to the front when full."""

    def __init__(self, envs, th: int = 0):
        super().__init__(envs, ring=0)  # (the pinned flags and action staging; no observation ring)
        self.Th = int(th) if th else max(128, 4 * envs.k)
        self.H = self.t.zeros((2, self.Th, envs.n, 16), dtype=self.t.float32, pin_memory=self.pin)
        self.Hn = self.H.numpy()
        self.par, self.q, self.prev_reset = 0, envs.k - 1, None
        self.autoreset = not (int(envs.cfg.flags) & F16_FLAG_NO_AUTORESET)

    def _view(self, par: int) -> np.ndarray:
        k, q = self.envs.k, self.q
        return self.Hn[par, q - k + 1:q + 1, :, :F16_OBS_DIM].transpose(1, 0, 2)

    def reset_obs(self, obs_dev):
        """The whole current window, into both host histories."""
        k = self.envs.k
        self.q, self.prev_reset = k - 1, None
        w = obs_dev.transpose(0, 1)
        for b in (0, 1):
            self.H[b, :k, :, :F16_OBS_DIM].copy_(w, non_blocking=True)
        self._wait()
        return self._view(self.par)

    def step_outputs(self, obs_dev):
        e, k = self.envs, self.envs.k
        q = self.q + 1
        if q >= self.Th:  # host restart: the last K-1 positions to the front of both histories
            for b in (0, 1):
                self.Hn[b, :k - 1] = self.Hn[b, q - k + 1:q]
            q = k - 1
        par = self.par ^ 1
        new, other = e.new_frame_slots()  # position p of the current and of the other device history
        self.H[par, q].copy_(new, non_blocking=True)
        self.H[par ^ 1, q].copy_(other, non_blocking=True)
        self.flags.copy_(e.step_flags, non_blocking=True)
        self._wait()
        rew, term, trunc = self.rew_term_trunc
        Hc = self.Hn[par]
        if k > 1 and self.prev_reset is not None and self.prev_reset.size:  # the kernel's FRESH fill
            idx = self.prev_reset
            Hc[q - k + 1:q, idx] = self.Hn[par ^ 1, q - 1, idx][None]
        self.prev_reset = None
        if self.autoreset:
            idx = np.flatnonzero(term | trunc)
            if idx.size:
                if k > 1:  # lanes reset by this step: K-1 copies of their reset frame
                    Hc[q - k + 1:q, idx] = Hc[q, idx][None]
                self.prev_reset = idx
        self.q, self.par = q, par
        return self._view(par), rew, term, trunc

    def _terminal_obs(self, idx, i):
        """The other host history's window."""
        return np.ascontiguousarray(self._view(self.par ^ 1)[idx])


def _staging(envs, copy_obs: bool = False):
    """The numpy-mode staging for a handle: the host window mirror for handles that say they can be
    mirrored slot by slot (only the new slots cross PCIe), else -- copy_obs, another layout, a stand-in
    without the attribute -- whole-observation copies, owned by the caller under copy_obs."""
    if not copy_obs and getattr(envs, "mirrors_by_slot", False):
        return _HostWindow(envs)
    return _HostStaging(envs, copy=copy_obs)
