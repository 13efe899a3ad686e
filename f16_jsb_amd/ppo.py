"""The PPO minibatch update on the device (f16env_ppo_loss_head, f16env_ppo_adam_step; include/f16env.h).

SB3's PPO.train (ppo/ppo.py:310-400) does, per minibatch, `evaluate_actions`, the clipped
surrogate / value / entropy losses, `loss.backward()`, `clip_grad_norm_` and `optimizer.step()`:
several dozen tiny torch launches. `DevicePPO` does the same on a `DevicePolicy`'s blob in six HIP
launches and no host synchronisation: the forward (deterministic: its action is the mean), the
advantage moments, the loss head (d_mean, d_values, partial sums), the backward's two launches
(f16env_policy_backward) and one block of clip + Adam that writes the blob in place.

    ppo = DevicePPO(pol, lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)
    for mb in buf.get(256):
        ppo.update(mb)
    ppo.stats            # device float[8] of the last update (abi.PPO_STATS); reading it synchronises
    ppo.set_hyper(lr=..., clip_range=...)     # a schedule: one stream-ordered copy, graphs follow it

No stable_baselines3 import. No fallback: without the library or a GPU it raises.
"""
from __future__ import annotations

import ctypes

import torch

from .abi import F16_POLICY_OFF_LOG_STD, F16_PPO_NORMALIZE_ADV, PPO_HYPER, PPO_STATS
from .buffers import need_tensor, stream_ptr
from .policy import ACT_DIM


class DevicePPO:
    """Standard PPO's minibatch update (normalised advantages, no value clipping) in place on
    `pol.blob`, with torch.optim.Adam's state (exp_avg, exp_avg_sq, step) in blob layout on the device.

    The hyper-parameters live in a device array (`hyper`, abi.PPO_HYPER order) that the kernels read
    when they run, so `set_hyper` takes effect in a captured graph without a re-capture. The buffers
    (`mean`, `values`, `d_mean`, `d_values`, the two workspaces) are sized by `max_batch`; outside a
    stream capture they grow with the batch, inside one a larger batch raises.

    The blob's version counter: after an eager `update` / `step_from` the blob's autograd version is
    advanced, so a `loss.backward()` through `pol.evaluate_actions` results from before the step is
    refused by torch's saved-tensor check as after `optimizer.step()`. A graph replay cannot do that
    (it runs no Python): do not keep autograd graphs over the blob across replays. Captured
    forwards see the new weights, because it is the same storage."""

    def __init__(self, pol, lr: float = 3e-4, clip_range: float = 0.2, ent_coef: float = 0.0, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, normalize_advantage: bool = True, betas=(0.9, 0.999), eps: float = 1e-5,
                 max_batch: int = 256, max_blocks: int = 0):
        from ._lib import F16EnvError, fn
        if pol.device.type != "cuda":
            raise F16EnvError("DevicePPO runs on the GPU (f16env_ppo_loss_head, f16env_ppo_adam_step); the policy is "
                              "on %s and there is no fallback" % pol.device)
        self._ws_fn, self._blocks_fn, self._head, self._adam = map(fn, (
            "f16env_ppo_workspace", "f16env_ppo_head_blocks", "f16env_ppo_loss_head", "f16env_ppo_adam_step"))
        self.pol, self.device = pol, pol.device
        self.normalize_advantage = bool(normalize_advantage)
        self.max_blocks = int(max_blocks)
        self.logstd_off = int(pol.offsets[F16_POLICY_OFF_LOG_STD])
        z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=self.device)  # noqa: E731
        self.hyper, self.stats = z(len(PPO_HYPER)), z(len(PPO_STATS))
        self.grad, self.exp_avg, self.exp_avg_sq = z(pol.n_floats), z(pol.n_floats), z(pol.n_floats)
        self.step = z(1, dtype=torch.int32)
        self._hyper = {}
        self.set_hyper(lr=lr, clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                       beta1=betas[0], beta2=betas[1], eps=eps)
        self.max_batch = 0
        self.reserve(max_batch)

    # ------------------------------------------------------------------------------------------
    def set_hyper(self, **kw):
        """Set any of abi.PPO_HYPER (lr, clip_range, ent_coef, vf_coef, max_grad_norm, beta1, beta2,
        eps): one stream-ordered 32-byte copy into the device array; later launches and replays of
        captured graphs read the new values. Not for use inside a stream capture."""
        for key in kw:
            if key not in PPO_HYPER:
                raise ValueError("unknown hyper-parameter %r (one of %s)" % (key, ", ".join(PPO_HYPER)))
        self._hyper.update({key: float(v) for key, v in kw.items()})
        self.hyper.copy_(torch.tensor([self._hyper[key] for key in PPO_HYPER], dtype=torch.float32), non_blocking=True)
        return self

    def reserve(self, n: int):
        """Size the buffers and both workspaces for minibatches of up to n rows (call it ahead of a
        stream capture: nothing may be allocated inside one)."""
        from ._lib import check
        n = int(n)
        if n <= self.max_batch:
            return self
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a minibatch of %d rows inside a stream capture, the buffers hold %d: construct with "
                               "max_batch >= %d or call reserve(%d) ahead of the capture" % (n, self.max_batch, n, n))
        need = ctypes.c_int64(0)
        check(self._ws_fn(n, self.max_blocks, ctypes.byref(need)), "f16env_ppo_workspace")
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=self.device)  # noqa: E731
        self.mean, self.d_mean = e(n, ACT_DIM), e(n, ACT_DIM)
        self.values, self.d_values, self._log_probs = e(n), e(n), e(n)
        self._head_ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device=self.device)
        self.pol.reserve_backward(n)
        self.max_batch = n
        return self

    def _bump(self):
        if not torch.cuda.is_current_stream_capturing():
            torch.autograd.graph.increment_version(self.pol.blob)

    # ------------------------------------------------------------------------------------------
    def update(self, observations, actions=None, old_values=None, old_log_prob=None, advantages=None, returns=None):
        """One minibatch update: forward -> loss head -> backward -> clip + Adam, all on the current
        stream, no host synchronisation. Takes a RolloutSamples (or any six-tuple in its order) or the
        six tensors: observations (n, K, D) as DevicePolicy reads them, actions (n, 4) 16-B aligned,
        old_values, old_log_prob, advantages, returns (n,), contiguous float32 on the device.
        `returns` is the value target; old_values is checked and not read (standard PPO without
        value clipping). Afterwards `grad` holds the complete gradient (before clipping) and `stats`
        the statistics. n == 0 does nothing."""
        from ._lib import check
        if actions is None and isinstance(observations, tuple) and len(observations) == 6:
            observations, actions, old_values, old_log_prob, advantages, returns = observations
        pol = self.pol
        n = pol._check_obs(observations)
        need_tensor(actions, (n, ACT_DIM), torch.float32, self.device, "actions", 16)
        for x, name in ((old_values, "old_values"), (old_log_prob, "old_log_prob"), (advantages, "advantages"),
                        (returns, "returns")):
            need_tensor(x, (n,), torch.float32, self.device, name)
        if n == 0:
            return self
        self.reserve(n)
        mean, values, d_mean, d_values = self.mean[:n], self.values[:n], self.d_mean[:n], self.d_values[:n]
        pol.forward_into(observations, 0, mean, values, self._log_probs[:n], deterministic=True)
        blocks = ctypes.c_int32(0)
        check(self._blocks_fn(n, self.max_blocks, ctypes.byref(blocks)), "f16env_ppo_head_blocks")
        check(self._head(stream_ptr(self.device), n, mean.data_ptr(), values.data_ptr(), actions.data_ptr(),
                         old_log_prob.data_ptr(), advantages.data_ptr(), returns.data_ptr(),
                         pol.blob.data_ptr() + 4 * self.logstd_off, self.hyper.data_ptr(),
                         F16_PPO_NORMALIZE_ADV if self.normalize_advantage else 0, self.max_blocks,
                         self._head_ws.data_ptr(), self._head_ws.numel(), d_mean.data_ptr(), d_values.data_ptr()),
              "f16env_ppo_loss_head")
        pol.backward_blob(observations, d_mean, d_values, out=self.grad)
        check(self._adam(stream_ptr(self.device), pol.n_floats, pol.blob.data_ptr(), self.grad.data_ptr(), self.exp_avg.data_ptr(),
                         self.exp_avg_sq.data_ptr(), self.step.data_ptr(), self.hyper.data_ptr(), self.logstd_off,
                         self._head_ws.data_ptr(), blocks.value, self.stats.data_ptr()), "f16env_ppo_adam_step")
        self._bump()
        return self

    def step_from(self, grad_blob):
        """Clip + Adam alone on a gradient in blob layout (e.g. pol.blob.grad formed by autograd):
        f16env_ppo_adam_step without a head. `grad_blob` is not changed; stats[6:8] are written."""
        from ._lib import check
        need_tensor(grad_blob, (self.pol.n_floats,), torch.float32, self.device, "grad_blob")
        check(self._adam(stream_ptr(self.device), self.pol.n_floats, self.pol.blob.data_ptr(), grad_blob.data_ptr(),
                         self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.step.data_ptr(), self.hyper.data_ptr(),
                         0, None, 0, self.stats.data_ptr()), "f16env_ppo_adam_step")
        self._bump()
        return self

    def train(self, src, n_epochs: int, batch_size: int, generator=None, target_kl=None):
        """ppo.py:310-400's loops: n_epochs shuffled passes over a finished rollout (`src`: a full
        DeviceRolloutBuffer, or the dict gather_to_rank0 returns), one `update` per minibatch.
        Returns the number of updates made. With target_kl each minibatch costs one `.item()` on
        approx_kl -- a host synchronisation -- and the loops end once it exceeds 1.5 target_kl; the
        update that crossed it has been applied (SB3 looks before its optimiser step and skips it)."""
        from .rollout import minibatches
        updates = 0
        for _ in range(int(n_epochs)):
            it = src.get(batch_size, generator=generator) if hasattr(src, "get") \
                else minibatches(src, batch_size=batch_size, generator=generator)
            for mb in it:
                self.update(mb)
                updates += 1
                if target_kl is not None and self.stats[PPO_STATS.index("approx_kl")].item() > 1.5 * target_kl:
                    return updates
        return updates

    # ------------------------------------------------------------------------------------------
    def state_dict(self):
        """Adam's state in blob layout, the step counter and the hyper-parameters (copies)."""
        return {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "step": self.step.clone(),
                "hyper": self.hyper.clone()}

    def load_state_dict(self, sd):
        for key, dst in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq), ("step", self.step)):
            src = torch.as_tensor(sd[key])
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError("%s of shape %s where %s was expected" % (key, tuple(src.shape), tuple(dst.shape)))
            dst.copy_(src.to(dst.dtype), non_blocking=True)
        h = torch.as_tensor(sd["hyper"]).to(torch.float32).reshape(-1).cpu()
        if h.numel() != len(PPO_HYPER):
            raise ValueError("hyper must hold %d values" % len(PPO_HYPER))
        return self.set_hyper(**{key: float(v) for key, v in zip(PPO_HYPER, h)})
