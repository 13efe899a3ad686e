"""The two observation layouts behind ``F16Envs`` (env.py chooses one at creation): each owns its
buffers, their cached addresses and the ctypes entry points that take them, and both offer the
same calls -- obs / terminal_obs, reset, step (with or without a done list), step_ex (in-kernel
actions, fused features / poses), step_slot(_checked) (the rollout-slot step), rollout_random,
set_obs, state_written, obs_features, poses, waves_per_simd. Arguments arrive validated
(buffers.need_tensor / as_act): nothing here checks a caller's buffer."""
from __future__ import annotations

import ctypes
from collections import namedtuple

from ._lib import check, lib
from .abi import (RolloutSlot, F16_OBS_DIM, F16_FLAG_NO_AUTORESET, F16_SLOT_FEATURE_WINDOW,
                  F16_STEP_FEATURE_WINDOW, F16_STEP_POSES)

StepOut = namedtuple("StepOut", "obs rew terminated truncated terminal_obs ep_return ep_len")
U64 = 0xFFFFFFFFFFFFFFFF


def _ptr(t):
    return None if t is None else t.data_ptr()


def _default_history(k: int) -> int:
    """Default window history T: a restart every T-K+1 steps; 2 x 256 x 64 B = 32 KiB per env."""
    return max(256, 2 * k)


def as_act(e, x, name="actions"):
    """x as an aligned contiguous (N, 4) float32 tensor on e.device: used as it is when it is
    one already, else copied into e._act (the one place that states this rule)."""
    t = e.torch
    if not (isinstance(x, t.Tensor) and x.device == e.device and x.dtype == t.float32 and x.is_contiguous()
            and x.data_ptr() % 16 == 0):
        e._act.copy_(t.as_tensor(x, dtype=t.float32).reshape(e.n, 4), non_blocking=True)
        x = e._act
    if x.shape != (e.n, 4):
        raise ValueError("%s must be (N, 4), got %s" % (name, tuple(x.shape)))
    return x


class _ContiguousLayout:
    """Observations in two ping-pong (N, K, 15) buffers: a step reads one and writes the other."""
    name = "contiguous"

    def __init__(self, h, stream, torch, device, n, k, cfg, outs, fused_features=False, fused_poses=False, **_):
        if fused_features or fused_poses:
            raise ValueError("fused_features / fused_poses need obs_layout='window'")
        self.h, self.stream, self.cur = h, stream, 0
        self.bufs = [torch.zeros((n, k, F16_OBS_DIM), dtype=torch.float32, device=device) for _ in range(2)]
        self.terminal_obs = torch.zeros((n, k, F16_OBS_DIM), dtype=torch.float32, device=device)
        rew, term, trunc, ep_return, ep_len = outs
        self._out = (rew, term, trunc, self.terminal_obs, ep_return, ep_len)
        # the handle's own buffers never move: their addresses are taken once, not per step
        self._buf_ptr = [o.data_ptr() for o in self.bufs]
        self._out_ptr = tuple(o.data_ptr() for o in self._out)
        self._step_fn, self._slot_fn = lib().f16env_step, lib().f16env_step_rollout

    obs = property(lambda self: self.bufs[self.cur])
    waves_per_simd = property(lambda self: int(lib().f16env_step_waves_per_simd(self.h)))

    def reset(self, m, g, c):
        check(lib().f16env_reset(self.h, self.stream(), m, g, c, self._buf_ptr[self.cur]), "f16env_reset")
        return self.obs

    def step(self, act, done_idx=None, n_done=None) -> StepOut:
        cur = self.cur  # one ctypes call on cached addresses
        check(self._step_fn(self.h, self.stream(), act.data_ptr(), self._buf_ptr[cur], self._buf_ptr[cur ^ 1],
                            *self._out_ptr, None if done_idx is None else done_idx.data_ptr(),
                            None if n_done is None else n_done.data_ptr()), "f16env_step")
        self.cur = cur ^ 1
        return StepOut(self.bufs[cur ^ 1], *self._out)

    def step_ex(self, act, seed: int, step: int) -> StepOut:  # in-kernel actions: an empty rollout slot
        return self.step_slot(RolloutSlot(seed & U64, step & U64, None, None, None, None, None, None, 0, 0), _ptr(act))

    def step_slot_checked(self, slot, act_ptr) -> StepOut:
        if slot.next_frame is not None:
            raise ValueError("the contiguous layout writes frame (the acted-on observation's newest frame), not next_frame")
        return self.step_slot(slot, act_ptr)

    def step_slot(self, slot, act_ptr) -> StepOut:
        cur = self.cur
        check(self._slot_fn(self.h, self.stream(), ctypes.byref(slot), act_ptr, self._buf_ptr[cur],
                            self._buf_ptr[cur ^ 1], *self._out_ptr, None, None), "f16env_step_rollout")
        self.cur = cur ^ 1
        return StepOut(self.bufs[cur ^ 1], *self._out)

    def rollout_random(self, sd, st, T, *bufs) -> None:
        cur = self.cur
        check(lib().f16env_rollout_random(self.h, self.stream(), sd, st, T, self._buf_ptr[cur], self._buf_ptr[cur ^ 1],
                                          *map(_ptr, bufs)), "f16env_rollout_random")
        self.cur = cur ^ 1

    def set_obs(self, o) -> None:
        self.obs.copy_(o)

    def state_written(self) -> None:  # (nothing here is derived from the state)
        pass

    def obs_features(self):
        from .features import features
        return features(self.obs)

    def poses(self):
        from .telemetry import poses
        return poses(self.obs)


class _Derived:
    """Whether the windowed layout's derived windows -- the policy features of both frame windows
    and the pose export -- describe the current observation. The rule: every op that changes the
    frame windows (a step, reset, set_state, set_obs, rollout_random) leaves the feature windows
    one op further behind and the poses stale.
      * Features current (0 behind): obs_features() launches nothing. If they also hold the last
        step's ahead fills (the next step's window fills of the lanes that step reset), the next
        step may keep them itself (F16_SLOT_FEATURE_WINDOW / F16_STEP_FEATURE_WINDOW: "fused").
      * One op behind, that op a step, ahead fills held: obs_features() transforms the one new
        frame per env and applies that step's ahead fills ("incremental").
      * Otherwise (never written; after a reset, set_state, set_obs or rollout_random; after a
        step not followed by a call) it transforms both whole windows ("full") and applies the
        ahead fills only if the last op was a step -- after any other op the lanes due a fill are
        not known, so the call after the step that follows is "full" once more.
    A history restart moves current feature windows along with the frames. poses() is the bound
    buffer only while no op followed the step (or the poses() call) that wrote it."""

    def __init__(self):
        self.calls = {"incremental": 0, "full": 0, "fused": 0}  # F16Envs.feature_window_calls
        self._behind = 2          # window changes since the features were written (2: or more / never)
        self._by_step = False     # the last window change was a step
        self._ahead = False       # the feature windows hold the last step's ahead fills
        self._poses = False

    def windows_changed(self, by_step: bool) -> None:
        self._behind = 2 if self._behind else 1
        self._by_step = by_step
        self._poses = False

    def can_fuse_features(self) -> bool:
        return self._ahead and self._behind == 0

    def features_due(self):
        """What obs_features() has to launch: None, "incremental" or "full"."""
        if self._behind == 0:
            return None
        return "incremental" if self._ahead and self._behind == 1 and self._by_step else "full"

    def features_written(self, how: str) -> bool:
        """`how` ("incremental", "full", "fused") brought them up to date; returns whether the
        ahead fills are held (after "full": whether to apply them now)."""
        self.calls[how] += 1
        self._behind = 0
        if how == "full":
            self._ahead = self._by_step
        return self._ahead

    def histories_restarted(self) -> bool:
        """The frame windows moved to the front: whether the feature windows have to move along."""
        return self._behind == 0

    def poses_written(self) -> None:
        self._poses = True

    def poses_current(self) -> bool:
        return self._poses


class _WindowLayout:
    """Observations as (N, K, 15) views of two per-env frame histories of T positions of 64-B frame
    slots: a step writes the new frame to position p+1 of both; the observation is the window ending
    there in the history of the new parity, the terminal observation the other history's window."""
    name = "window"

    def __init__(self, h, stream, torch, device, n, k, cfg, outs, history=0, window_order="position",
                 fused_features=False, fused_poses=False):
        T = int(history) if history else _default_history(k)
        if T < 2 * k:
            raise ValueError("history must be >= 2 * stack_k")
        if window_order not in ("position", "env"):
            raise ValueError("window_order must be 'position' or 'env'")
        self.h, self.stream, self.torch, self.device, self.n, self.k, self.T = h, stream, torch, device, n, k, T
        self.env_major = window_order == "env"
        self.autoreset = 0 if int(cfg.flags) & F16_FLAG_NO_AUTORESET else 1
        self.fused_features, self.fused_poses = bool(fused_features), bool(fused_poses)
        L = lib()
        check(L.f16env_set_window_order(h, 1 if self.env_major else 0), "f16env_set_window_order")
        # [parity][position][env][16] (64-B frame slots, position-major) or [parity][env][position][16]
        self.hist = torch.zeros((2, n, T, 16) if self.env_major else (2, T, n, 16), dtype=torch.float32, device=device)
        self.hist_ptr = (self.hist[0].data_ptr(), self.hist[1].data_ptr())
        self.rows = self.hist.transpose(1, 2) if self.env_major else self.hist  # [parity][position][env][16] view
        # every (parity, newest position) window, viewed once here: a step's host cost stays one ctypes call
        self._views = [[self.rows[b, p - k + 1:p + 1, :, :F16_OBS_DIM].transpose(0, 1) if p >= k - 1 else None
                        for p in range(T)] for b in (0, 1)]
        self.cur, self.p = 0, k - 1   # parity / newest frame position of the current observation's window
        self.derived = _Derived()
        self.fh = self.fh_ptr = self._fviews = None   # feature histories, made at the first use
        self.poses_buf = None                         # (N, 10) pose export of a fused_poses handle
        self._out = outs
        self._out_ptr = tuple(o.data_ptr() for o in outs)
        check(L.f16env_window_bind(h, *self.hist_ptr, T, *self._out_ptr), "f16env_window_bind")
        self._step_bound, self._step_list = L.f16env_window_step_bound, L.f16env_step_window
        self._step_ex, self._slot_fn = L.f16env_window_step_ex, L.f16env_window_step_rollout
        if self.fused_features or self.fused_poses:
            if L.f16env_window_resets_deferred(h):
                # the deferred-reset step (cfg5 with F16ENV_ICC_PERIOD=0): the epilogue extras
                # would describe the pre-reset window, and f16env_window_step_ex refuses them --
                # refused here instead of at the first step
                raise ValueError("fused_features / fused_poses are not available with the deferred-reset "
                                 "windowed step (cfg5 with F16ENV_ICC_PERIOD=0)")
            self.step = self._step_fused
        if self.fused_features:
            self._feature_hist()
        if self.fused_poses:
            self.poses_buf = torch.zeros((n, 10), dtype=torch.float32, device=device)
            check(L.f16env_window_poses_bind(h, self.poses_buf.data_ptr()), "f16env_window_poses_bind")

    def window(self, other: int = 0):
        """(N, K, 15) view of the current (other=0) or other-parity history's window."""
        return self._views[self.cur ^ other][self.p]

    obs = property(window)
    terminal_obs = property(lambda self: self.window(1))
    waves_per_simd = property(lambda self: int(lib().f16env_step_window_waves_per_simd(self.h)))

    def new_slots(self):
        """The last step's two new (N, 16) slot blocks: position p of the current and of the other history."""
        return self.rows[self.cur, self.p], self.rows[self.cur ^ 1, self.p]

    def reset(self, m, g, c):
        check(lib().f16env_reset_window(self.h, self.stream(), m, g, c, self.hist_ptr[self.cur], self.T, self.p),
              "f16env_reset_window")
        self.derived.windows_changed(by_step=False)
        return self.window()

    def _advance(self):
        """(stream, parity, position) of the next step: the new frame goes to position p+1 of
        both histories (after a restart when p+1 reaches T)."""
        s = self.stream()
        p = self.p + 1
        if p >= self.T:  # move the last K-1 frames to the front of both histories
            check(lib().f16env_window_restart(self.h, s, *self.hist_ptr, self.T, self.p), "f16env_window_restart")
            if self.derived.histories_restarted():
                k = self.k   # (K-1 whole rows: one contiguous device-to-device copy per parity)
                for b in (0, 1):
                    self.fh[b, :k - 1].copy_(self.fh[b, self.p - k + 2:self.p + 1])
            p = self.k - 1
        return s, self.cur ^ 1, p

    def _advanced(self, cur, p, fused: bool = False) -> StepOut:
        self.cur, self.p = cur, p
        self.derived.windows_changed(True)
        if fused:
            self.derived.features_written("fused")
        rew, term, trunc, ep_return, ep_len = self._out
        return StepOut(self._views[cur][p], rew, term, trunc, self._views[cur ^ 1][p], ep_return, ep_len)

    def step(self, act, done_idx=None, n_done=None) -> StepOut:
        s, cur, p = self._advance()
        if done_idx is None:  # the common case: five arguments, the rest bound at creation
            check(self._step_bound(self.h, s, act.data_ptr(), cur, p), "f16env_window_step_bound")
        else:
            check(self._step_list(self.h, s, act.data_ptr(), self.hist_ptr[cur], self.hist_ptr[cur ^ 1], self.T, p,
                                  *self._out_ptr, done_idx.data_ptr(), n_done.data_ptr()), "f16env_step_window")
        return self._advanced(cur, p)

    def _step_fused(self, act, done_idx=None, n_done=None) -> StepOut:  # (with a done list: no extras)
        if done_idx is not None:
            return _WindowLayout.step(self, act, done_idx, n_done)
        return self.step_ex(act, 0, 0)

    def step_ex(self, act, seed: int, step: int) -> StepOut:
        """f16env_window_step_ex: act None draws the actions in the kernel (sample_actions(seed,
        step)); a fused_features handle also keeps its feature windows in the step's epilogue
        whenever they are current before it, and catches them up after a step that could not."""
        fw = self.fused_features and self.derived.can_fuse_features()
        s, cur, p = self._advance()
        flags = (F16_STEP_FEATURE_WINDOW if fw else 0) | (F16_STEP_POSES if self.fused_poses else 0)
        check(self._step_ex(self.h, s, _ptr(act), cur, p, flags, seed & U64, step & U64), "f16env_window_step_ex")
        out = self._advanced(cur, p, fw)
        if self.fused_poses:
            self.derived.poses_written()
        if self.fused_features and not fw:
            self.obs_features()  # whole windows + the step's ahead fills: the next step fuses
        return out

    def step_slot_checked(self, slot, act_ptr) -> StepOut:
        if slot.frame is not None:
            raise ValueError("the windowed layout writes next_frame (the returned observation's newest frame), not frame")
        return self.step_slot(slot, act_ptr)

    def step_slot(self, slot, act_ptr) -> StepOut:
        """The rollout-slot step; it keeps the feature windows itself (F16_SLOT_FEATURE_WINDOW)
        when they are current, so its epilogue brings them to the new position."""
        fw = self.derived.can_fuse_features()
        slot.flags = (slot.flags | F16_SLOT_FEATURE_WINDOW) if fw else (slot.flags & ~F16_SLOT_FEATURE_WINDOW)
        s, cur, p = self._advance()
        check(self._slot_fn(self.h, s, ctypes.byref(slot), act_ptr, cur, p), "f16env_window_step_rollout")
        return self._advanced(cur, p, fw)

    def rollout_random(self, sd, st, T, *bufs) -> None:
        k, p = self.k, self.p
        q = p + k if p + k < self.T else k - 1  # the output window: beside the input one
        if q - k + 1 <= p and p - k + 1 <= q:
            # (T < 3K - 1 and the window near the front): move the current windows
            # of both histories to positions 0 .. K-1 first; the output window K .. 2K-1 then
            # fits whenever T >= 2K (window_check's bound). The lanes' FRESH marks describe
            # window-relative positions, so they stay valid.
            self.rows[:, :k].copy_(self.rows[:, p - k + 1:p + 1].clone())
            p, q = k - 1, 2 * k - 1
        check(lib().f16env_window_rollout_random(self.h, self.stream(), sd, st, T, self.cur, p, q, *map(_ptr, bufs)),
              "f16env_window_rollout_random")
        self.p = q
        self.derived.windows_changed(by_step=False)

    def set_obs(self, o) -> None:
        self.window(0).copy_(o)
        self.window(1).copy_(o)
        # both windows are whole now: lanes reset before this need no refill at the next step
        check(lib().f16env_window_clear_fresh(self.h, self.stream()), "f16env_window_clear_fresh")
        self.derived.windows_changed(by_step=False)

    def state_written(self) -> None:
        self.derived.windows_changed(by_step=False)

    def poses(self):
        from .telemetry import poses
        if self.poses_buf is not None and self.derived.poses_current():
            return self.poses_buf
        self.derived.poses_written()  # (the bound buffer, when there is one, is current from here on)
        return poses(self.window(), out=self.poses_buf)  # (the newest frame of each stack, read in place)

    def obs_features(self):
        from .features import FEATURES_DIM
        n, k, L = self.n, self.k, lib()
        self._feature_hist()
        cur, p = self.cur, self.p
        how = self.derived.features_due()
        if how is not None:
            wrow, wenv = (16, self.T * 16) if self.env_major else (n * 16, 16)
            s = self.stream()
            if how == "full":
                for b in (cur, cur ^ 1):  # positions p-K+1 .. p of history b: K "rows" of N frames
                    check(L.f16env_features_strided(s, k, n, self.hist_ptr[b] + 4 * (p - k + 1) * wrow, wrow, wenv,
                                                    self.fh_ptr[b] + 4 * (p - k + 1) * n * FEATURES_DIM),
                          "f16env_features_strided")
            # "incremental": the new frame and the ahead fills; "full" after a step: the ahead fills alone
            # (the next step's window fills of the lanes this state's step reset: the kernel's invariant)
            if self.derived.features_written(how):
                check(L.f16env_features_window_step(s, n, k, p, self.hist_ptr[cur], wrow, wenv, self.fh_ptr[cur],
                                                    self.fh_ptr[cur ^ 1], self._out_ptr[1], self._out_ptr[2],
                                                    self.autoreset, 1 if how == "incremental" else 0),
                      "f16env_features_window_step")
        v = self._fviews[cur][p]
        if v is None:
            v = self._fviews[cur][p] = self.fh[cur, p - k + 1:p + 1].transpose(0, 1)
        return v

    def _feature_hist(self) -> None:
        """The two feature histories [T][N][17] beside the frame histories, allocated and bound once (steps
        that keep them update them in their epilogue); positions outside the window are written before read."""
        if self.fh is None:
            from .features import FEATURES_DIM
            t = self.torch
            self.fh = t.empty((2, self.T, self.n, FEATURES_DIM), dtype=t.float32, device=self.device)
            self.fh_ptr = (self.fh[0].data_ptr(), self.fh[1].data_ptr())
            check(lib().f16env_window_feature_bind(self.h, *self.fh_ptr), "f16env_window_feature_bind")
            self._fviews = [[None] * self.T for _ in range(2)]
