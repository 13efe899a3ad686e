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

The reference trains with AM-PPO (train.py: use_am_ppo, dynago_*, am_ppo_optimizer "DAG"): DynAGO
advantage modulation (f16env_ppo_dynago_update once per rollout, f16env_ppo_loss_head_am per
minibatch) and the DAG or AlphaGrad optimiser (f16env_ppo_dag_step), the same six launches plus
three per rollout:

    ppo = DevicePPO(pol, lr=3e-4, am_ppo={}, optimizer="dag")     # the reference's defaults
    ppo.train(buf, n_epochs=10, batch_size=256)                     # the controller, then the epochs
    ppo.am_state, ppo.am_stats                                      # (alpha, sat); abi.PPO_AM_STATS

No stable_baselines3 import. No fallback: without the library or a GPU it raises.
"""
from __future__ import annotations

import ctypes
import statistics

import torch

from . import _lib  # (a DevicePPO looks its entry points up as _lib.fn when it is built: tests wrap that name)
from ._lib import F16EnvError, check
from .abi import (F16_POLICY_OFF_LOG_STD, F16_PPO_AM_NORMALIZE, F16_PPO_DAG_FIXED_ALPHA, F16_PPO_NORMALIZE_ADV, PPO_AM_STATS,
                  PPO_DAG, PPO_DYNAGO, PPO_HYPER, PPO_STATS, policy_segments)
from .buffers import need_tensor, stream_ptr
from .policy import ACT_DIM

# ppo.py:141-154, the reference's AM-PPO defaults (kappa_controller None: kappa)
AM_PPO_DEFAULTS = dict(tau=1.25, p_star=0.10, kappa=2.0, eta=0.3, rho=0.1, eps=1e-5, alpha_min=1e-12, alpha_max=1e12,
                       rho_sat=0.98, alpha_init=1.0, sat_init=0.10, v_shift=0.0, norm_adv=True, kappa_controller=None)
# ppo/optim/sgd.py:118-132, DAG's (kappa None: tau / Phi^-1(1 - p_star / 2)); :401-403, AlphaGrad's
DAG_DEFAULTS = dict(tau=1.25, p_star=0.10, kappa=None, beta=1.0 / 3.0, eta=0.3, rho=0.1, eps=1e-5, alpha_min=1e-12,
                    alpha_max=1e12, k_val=2.0, lambda_rms=0.3, s_min=0.1, gamma=1.0, ema_beta=0.98, warmup_steps=500,
                    sat_every=10)
DAG_NOT_BUILT = ("momentum", "dampening", "weight_decay", "nesterov", "maximize", "k_sched", "use_exact_sigma",
                 "sigma_every", "foreach", "differentiable", "fused")
OPTIMIZERS = ("adam", "dag", "alphagrad")


def dag_kappa(tau: float, p_star: float) -> float:
    """sgd.py:124-127: tau / Phi^-1(1 - p_star / 2), in fp64 on the host."""
    return float(tau) / statistics.NormalDist().inv_cdf(1.0 - float(p_star) / 2.0)


def _dag_constants(optimizer, kwargs):
    """The optimiser's keyword arguments as the values of abi.PPO_DAG. DAG takes the reference's
    nested form too (hyper=dict(...), shrink=dict(...)); the options PPO._setup_model never passes
    and this kernel does not build are refused."""
    kw = dict(kwargs or {})
    for nested in ("hyper", "shrink"):
        kw.update(kw.pop(nested, None) or {})
    for key in kw:
        if key in DAG_NOT_BUILT:
            raise ValueError("%s is not built: f16env_ppo_dag_step is the optimiser as PPO._setup_model constructs it "
                             "(no momentum, weight decay, nesterov, maximize, k_sched or exact sigma)" % key)
    if optimizer == "alphagrad":
        unknown = set(kw) - {"alpha", "epsilon"}
        if unknown:
            raise ValueError("unknown AlphaGrad argument(s) %s (alpha, epsilon)" % sorted(unknown))
        alpha, epsilon = float(kw.get("alpha", 0.0)), float(kw.get("epsilon", 1e-8))
        if alpha <= 0.0:
            raise ValueError("Invalid alpha value: %s" % alpha)       # (sgd.py:414-417)
        if epsilon <= 0.0:
            raise ValueError("Invalid epsilon value: %s" % epsilon)
        return dict(DAG_DEFAULTS, kappa=0.0, eps=epsilon, alpha=alpha)
    unknown = set(kw) - set(DAG_DEFAULTS)
    if unknown:
        raise ValueError("unknown DAG argument(s) %s (one of %s)" % (sorted(unknown), ", ".join(DAG_DEFAULTS)))
    c = dict(DAG_DEFAULTS, **kw)
    if c["kappa"] is None:
        c["kappa"] = dag_kappa(c["tau"], c["p_star"])
    c["warmup_steps"], c["sat_every"] = int(c["warmup_steps"]), max(1, int(c["sat_every"]))
    return dict(c, alpha=0.0)


class DevicePPO:
    """Standard PPO's minibatch update (normalised advantages, no value clipping) in place on
    `pol.blob`, with torch.optim.Adam's state (exp_avg, exp_avg_sq, step) in blob layout on the device.

    The hyper-parameters live in a device array (`hyper`, abi.PPO_HYPER order) that the kernels read
    when they run, so `set_hyper` takes effect in a captured graph without a re-capture. The buffers
    (`mean`, `values`, `d_mean`, `d_values`, the two workspaces) are sized by `max_batch`; outside a
    stream capture they grow with the batch, inside one a larger batch raises.

    am_ppo: None, or a dict over AM_PPO_DEFAULTS (ppo.py's dynago_* arguments): `update` then takes
    the AM head (modulated advantages; the value target is mod + old_values, `returns` is not read)
    and `train` runs the controller once over the rollout's advantages ahead of the epochs. The
    parameters live in `dynago` (abi.PPO_DYNAGO), the controller's (alpha, sat) in `am_state`.
    optimizer: "adam", or "dag" / "alphagrad" (ppo/optim/sgd.py) with `optimizer_kwargs`; their
    constants live in `dag` (abi.PPO_DAG), DAG's state in `seg_state`, `dag_state`, `dag_counters`.
    lr and max_grad_norm stay in `hyper` for all three. The defaults launch exactly what they did
    before these arguments existed.

    The blob's version counter: after an eager `update` / `step_from` the blob's autograd version is
    advanced, so a `loss.backward()` through `pol.evaluate_actions` results from before the step is
    refused by torch's saved-tensor check as after `optimizer.step()`. A graph replay cannot do that
    (it runs no Python): do not keep autograd graphs over the blob across replays. Captured
    forwards see the new weights, because it is the same storage."""

    def __init__(self, pol, lr: float = 3e-4, clip_range: float = 0.2, ent_coef: float = 0.0, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, normalize_advantage: bool = True, betas=(0.9, 0.999), eps: float = 1e-5,
                 max_batch: int = 256, max_blocks: int = 0, am_ppo=None, optimizer: str = "adam", optimizer_kwargs=None):
        if hasattr(pol, "lma"):  # (before anything else: the refusal needs neither a GPU nor the library)
            from .lma_policy import NO_BACKWARD
            raise NotImplementedError("DevicePPO cannot train a DeviceLMAPolicy: " + NO_BACKWARD)
        if pol.device.type != "cuda":
            raise F16EnvError("DevicePPO runs on the GPU (f16env_ppo_loss_head, f16env_ppo_adam_step); the policy is "
                              "on %s and there is no fallback" % pol.device)
        if optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be one of %s, got %r" % (", ".join(OPTIMIZERS), optimizer))
        if optimizer == "adam" and optimizer_kwargs:
            raise ValueError("Adam's arguments are lr, betas and eps; optimizer_kwargs is for 'dag' and 'alphagrad'")
        self._ws_fn, self._blocks_fn, self._head, self._adam = map(_lib.fn, (
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
        self.am_ppo, self.optimizer = am_ppo is not None, optimizer
        if self.am_ppo:
            unknown = set(am_ppo) - set(AM_PPO_DEFAULTS)
            if unknown:
                raise ValueError("unknown am_ppo key(s) %s (one of %s)" % (sorted(unknown), ", ".join(AM_PPO_DEFAULTS)))
            cfg = dict(AM_PPO_DEFAULTS, **am_ppo)
            if cfg["kappa_controller"] is None:
                cfg["kappa_controller"] = cfg["kappa"]  # (ppo.py:214)
            self._am_head, self._dyn_ws_fn, self._dyn_update = map(_lib.fn, (
                "f16env_ppo_loss_head_am", "f16env_ppo_dynago_workspace", "f16env_ppo_dynago_update"))
            self.am_norm_adv = bool(cfg["norm_adv"])
            self.dynago, self.am_stats = z(len(PPO_DYNAGO)), z(len(PPO_AM_STATS))
            self.am_state = torch.tensor([cfg["alpha_init"], cfg["sat_init"]], dtype=torch.float32, device=self.device)
            self._dynago, self._dyn_ws, self._dyn_n = {}, torch.empty(16, dtype=torch.uint8, device=self.device), 0
            self.set_dynago(**{key: cfg[key] for key in PPO_DYNAGO})
        if optimizer != "adam":
            self._dag_step = _lib.fn("f16env_ppo_dag_step")
            self._dag = _dag_constants(optimizer, optimizer_kwargs)
            self.dag = z(len(PPO_DAG))
            self.set_dag()
            segs = policy_segments(pol.desc)
            self.n_segments = len(segs)
            self._segments = (ctypes.c_int32 * (3 * len(segs)))(*[v for seg in segs for v in seg])
            self.seg_state = torch.tensor([1.0, 0.0] * len(segs), dtype=torch.float32, device=self.device)  # (sgd.py:170-171)
            self.dag_state = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64, device=self.device)
            self.dag_counters = z(4, dtype=torch.int32)
        self.max_batch = 0
        self.reserve(max_batch)

    # ------------------------------------------------------------------------------------------
    def _set(self, names, host, dev, kw, what):
        for key in kw:
            if key not in names:
                raise ValueError("unknown %s %r (one of %s)" % (what, key, ", ".join(names)))
        host.update({key: float(v) for key, v in kw.items()})
        dev.copy_(torch.tensor([host[key] for key in names], dtype=torch.float32), non_blocking=True)
        return self

    def set_hyper(self, **kw):
        """Set any of abi.PPO_HYPER (lr, clip_range, ent_coef, vf_coef, max_grad_norm, beta1, beta2,
        eps): one stream-ordered 32-byte copy into the device array; later launches and replays of
        captured graphs read the new values. Not for use inside a stream capture."""
        return self._set(PPO_HYPER, self._hyper, self.hyper, kw, "hyper-parameter")

    def set_dynago(self, **kw):
        """Set any of abi.PPO_DYNAGO, as set_hyper does (AM-PPO only)."""
        if not self.am_ppo:
            raise ValueError("set_dynago needs am_ppo")
        return self._set(PPO_DYNAGO, self._dynago, self.dynago, kw, "DynAGO parameter")

    def set_dag(self, **kw):
        """Set any of abi.PPO_DAG, as set_hyper does (optimizer 'dag' or 'alphagrad'; AlphaGrad
        reads `alpha` and `eps`, its epsilon)."""
        if self.optimizer == "adam":
            raise ValueError("set_dag needs optimizer 'dag' or 'alphagrad'")
        if self.optimizer == "alphagrad" and float(kw.get("alpha", 1.0)) <= 0.0:
            raise ValueError("Invalid alpha value: %s" % kw["alpha"])
        return self._set(PPO_DAG, self._dag, self.dag, kw, "DAG constant")

    def reserve(self, n: int, rollout: int = 0):
        """Size the buffers and both workspaces for minibatches of up to n rows, and with AM-PPO the
        controller's workspace for `rollout` advantages (call it ahead of a stream capture: nothing
        may be allocated inside one)."""
        n, rollout = int(n), int(rollout)
        capturing = torch.cuda.is_current_stream_capturing()
        if self.am_ppo and rollout > self._dyn_n:
            if capturing:
                raise RuntimeError("a rollout of %d advantages inside a stream capture, the controller's workspace "
                                   "holds %d: call reserve(n, rollout=%d) ahead of the capture" % (rollout, self._dyn_n, rollout))
            need = ctypes.c_int64(0)
            check(self._dyn_ws_fn(rollout, self.max_blocks, ctypes.byref(need)), "f16env_ppo_dynago_workspace")
            self._dyn_ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device=self.device)
            self._dyn_n = rollout
        if n <= self.max_batch:
            return self
        if capturing:
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

    def _optimizer_step(self, grad, logstd_off, head_ws, blocks):
        """Clip + the optimiser's step on `grad`, with the head's workspace or without (None)."""
        pol, s = self.pol, stream_ptr(self.device)
        if self.optimizer == "adam":
            check(self._adam(s, pol.n_floats, pol.blob.data_ptr(), grad.data_ptr(), self.exp_avg.data_ptr(),
                             self.exp_avg_sq.data_ptr(), self.step.data_ptr(), self.hyper.data_ptr(), logstd_off, head_ws,
                             blocks, self.stats.data_ptr()), "f16env_ppo_adam_step")
        else:
            check(self._dag_step(s, pol.n_floats, pol.blob.data_ptr(), grad.data_ptr(), self.hyper.data_ptr(),
                                 self.dag.data_ptr(), self._segments, self.n_segments, self.seg_state.data_ptr(),
                                 self.dag_state.data_ptr(), self.dag_counters.data_ptr(),
                                 F16_PPO_DAG_FIXED_ALPHA if self.optimizer == "alphagrad" else 0, logstd_off, head_ws,
                                 blocks, self.stats.data_ptr()), "f16env_ppo_dag_step")
        self._bump()

    # ------------------------------------------------------------------------------------------
    def update(self, observations, actions=None, old_values=None, old_log_prob=None, advantages=None, returns=None):
        """One minibatch update: forward -> loss head -> backward -> clip + Adam, all on the current
        stream, no host synchronisation. Takes a RolloutSamples (or any six-tuple in its order) or the
        six tensors: observations (n, K, D) as DevicePolicy reads them, actions (n, 4) 16-B aligned,
        old_values, old_log_prob, advantages, returns (n,), contiguous float32 on the device.
        `returns` is the value target; old_values is checked and not read (standard PPO without
        value clipping). With am_ppo it is the other way round: the target is the modulated
        advantage plus old_values (ppo.py:369) and `returns` is checked and not read. Afterwards
        `grad` holds the complete gradient (before clipping) and `stats` the statistics. n == 0 does
        nothing."""
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
        log_std = pol.blob.data_ptr() + 4 * self.logstd_off
        if self.am_ppo:
            check(self._am_head(stream_ptr(self.device), n, mean.data_ptr(), values.data_ptr(), actions.data_ptr(),
                                old_log_prob.data_ptr(), advantages.data_ptr(), old_values.data_ptr(), log_std,
                                self.hyper.data_ptr(), self.dynago.data_ptr(), self.am_state.data_ptr(),
                                F16_PPO_AM_NORMALIZE if self.am_norm_adv else 0, self.max_blocks,
                                self._head_ws.data_ptr(), self._head_ws.numel(), d_mean.data_ptr(), d_values.data_ptr(),
                                self.am_stats.data_ptr()), "f16env_ppo_loss_head_am")
        else:
            check(self._head(stream_ptr(self.device), n, mean.data_ptr(), values.data_ptr(), actions.data_ptr(),
                             old_log_prob.data_ptr(), advantages.data_ptr(), returns.data_ptr(), log_std,
                             self.hyper.data_ptr(), F16_PPO_NORMALIZE_ADV if self.normalize_advantage else 0,
                             self.max_blocks, self._head_ws.data_ptr(), self._head_ws.numel(), d_mean.data_ptr(),
                             d_values.data_ptr()), "f16env_ppo_loss_head")
        pol.backward_blob(observations, d_mean, d_values, out=self.grad)
        self._optimizer_step(self.grad, self.logstd_off, self._head_ws.data_ptr(), blocks.value)
        return self

    def step_from(self, grad_blob):
        """Clip + the optimiser's step alone on a gradient in blob layout (e.g. pol.blob.grad formed
        by autograd): f16env_ppo_adam_step or f16env_ppo_dag_step without a head. `grad_blob` is not
        changed; stats[6:8] are written."""
        need_tensor(grad_blob, (self.pol.n_floats,), torch.float32, self.device, "grad_blob")
        self._optimizer_step(grad_blob, 0, None, 0)
        return self

    def dynago_update(self, advantages):
        """The DynAGO controller over a finished rollout's advantages (ppo.py:289-306, once per
        train() call): any contiguous float32 device tensor, 16-B aligned, read flat. Updates
        `am_state` = (alpha, sat) on the stream; one element or none leaves it as it is. Inside a
        stream capture the workspace must have been sized by reserve(n, rollout=...)."""
        if not self.am_ppo:
            raise ValueError("dynago_update needs am_ppo")
        if not isinstance(advantages, torch.Tensor):
            raise ValueError("advantages must be a tensor, got %s" % type(advantages).__name__)
        need_tensor(advantages, advantages.shape, torch.float32, self.device, "advantages", 16)
        n = advantages.numel()
        self.reserve(0, rollout=n)
        check(self._dyn_update(stream_ptr(self.device), n, advantages.data_ptr(), self.dynago.data_ptr(),
                               self.am_state.data_ptr(), self.max_blocks, self._dyn_ws.data_ptr(), self._dyn_ws.numel()),
              "f16env_ppo_dynago_update")
        return self

    def train(self, src, n_epochs: int, batch_size: int, generator=None, target_kl=None):
        """ppo.py:310-400's loops: n_epochs shuffled passes over a finished rollout (`src`: a full
        DeviceRolloutBuffer, or the dict gather_to_rank0 returns), one `update` per minibatch; with
        am_ppo the controller first, once, over all of `src`'s advantages (ppo.py:289-306).
        Returns the number of updates made. With target_kl each minibatch costs one `.item()` on
        approx_kl -- a host synchronisation -- and the loops end once it exceeds 1.5 target_kl; the
        update that crossed it has been applied (SB3 looks before its optimiser step and skips it)."""
        from .rollout import minibatches
        if self.am_ppo:
            self.dynago_update(src.advantages if hasattr(src, "get") else src["advantages"])
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
    def _state_arrays(self):
        """(key, tensor) of everything that is state beside the hyper-parameters, by configuration."""
        out = [("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq), ("step", self.step)]
        if self.am_ppo:
            out += [("am_state", self.am_state)]
        if self.optimizer != "adam":
            out += [("seg_state", self.seg_state), ("dag_state", self.dag_state), ("dag_counters", self.dag_counters)]
        return out

    def state_dict(self):
        """Adam's state in blob layout, the step counter and the hyper-parameters; with am_ppo the
        controller's state and `dynago`; with DAG / AlphaGrad its state and `dag` (copies)."""
        sd = {key: t.clone() for key, t in self._state_arrays()}
        sd["hyper"] = self.hyper.clone()
        if self.am_ppo:
            sd["dynago"] = self.dynago.clone()
        if self.optimizer != "adam":
            sd["dag"] = self.dag.clone()
        return sd

    def load_state_dict(self, sd):
        for key, dst in self._state_arrays():
            src = torch.as_tensor(sd[key])
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError("%s of shape %s where %s was expected" % (key, tuple(src.shape), tuple(dst.shape)))
            dst.copy_(src.to(dst.dtype), non_blocking=True)
        for key, names, setter in (("hyper", PPO_HYPER, self.set_hyper),
                                   ("dynago", PPO_DYNAGO, self.set_dynago if self.am_ppo else None),
                                   ("dag", PPO_DAG, self.set_dag if self.optimizer != "adam" else None)):
            if setter is None:
                continue
            h = torch.as_tensor(sd[key]).to(torch.float32).reshape(-1).cpu()
            if h.numel() != len(names):
                raise ValueError("%s must hold %d values" % (key, len(names)))
            setter(**{name: float(v) for name, v in zip(names, h)})
        return self
