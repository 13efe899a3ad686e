"""The policy of a rollout on the device (f16env_policy_forward, include/f16env.h ABI 7).

SB3's `collect_rollouts` calls `policy(obs_tensor)` every step (on_policy_algorithm.py:199-202):
for the default `MlpPolicy` that is ActorCriticPolicy.forward -- a flatten, two small MLPs
(torch_layers.py MlpExtractor, separate pi / vf nets), an action head with a state-independent
log_std, a value head, a Gaussian sample and its log-probability -- about twenty torch kernels.
`DevicePolicy` holds the same weights as one packed device blob and runs the whole forward as ONE
HIP launch that reads the observation in place (the windowed view included) and writes actions,
values and log-probs where the caller wants them. It fits `collect_rollout`'s `policy_fn` /
`value_fn` as it is, and `collect_rollout` gives it a fast path (no per-step copies).

    pol = DevicePolicy.from_state_dict(model.policy.state_dict(), stack_k=4)
    last_v, last_d = collect_rollout(envs, buf, policy_fn=pol)
    ...                      # PPO update
    pol.load_state_dict(model.policy.state_dict())   # one copy into the same blob

No stable_baselines3 import: only its key names. No fallback: without the library it raises.
"""
from __future__ import annotations

import ctypes

import torch

from .abi import (F16_POLICY_DETERMINISTIC, F16_POLICY_N_OFFSETS, F16_POLICY_OFF_ACT_B, F16_POLICY_OFF_ACT_W,
                  F16_POLICY_OFF_LOG_STD, F16_POLICY_OFF_VAL_B, F16_POLICY_OFF_VAL_W, F16_POLICY_VALUE_ONLY,
                  policy_blob_layout, policy_desc)

ACT_DIM = 4


def layers_from_state_dict(sd):
    """(pi, vf, act_head, val_head, log_std) from an SB3 ActorCriticPolicy state dict:
    mlp_extractor.policy_net.{0,2,4}.{weight,bias} (Linear layers sit at the even indices of the
    Sequential, the activations between them), mlp_extractor.value_net.*, action_net.*,
    value_net.*, log_std."""
    def branch(name):
        out = []
        for i in (0, 2, 4):
            w = sd.get("mlp_extractor.%s.%d.weight" % (name, i))
            if w is None:
                break
            out.append((w, sd["mlp_extractor.%s.%d.bias" % (name, i)]))
        if not out:
            raise KeyError("state dict has no mlp_extractor.%s.0.weight" % name)
        if "mlp_extractor.%s.6.weight" % name in sd:
            raise ValueError("mlp_extractor.%s has more than 3 hidden layers" % name)
        return out
    return (branch("policy_net"), branch("value_net"), (sd["action_net.weight"], sd["action_net.bias"]),
            (sd["value_net.weight"], sd["value_net.bias"]), sd["log_std"])


def _pack_weight(w, fan_in, rows):
    """torch's W[out][in] -> [rows/32][ceil(in/2)][2][32] (element W[32 to + i][2 s + h]), zero padded."""
    out, inn = w.shape
    if inn != fan_in or out > rows:
        raise ValueError("weight of shape %s where (<= %d, %d) was expected" % (tuple(w.shape), rows, fan_in))
    nks = (fan_in + 1) // 2
    p = torch.zeros((rows, 2 * nks), dtype=torch.float32, device=w.device)
    p[:out, :inn] = w
    return p.reshape(rows // 32, 32, nks, 2).permute(0, 2, 3, 1).reshape(-1)


def _pack_bias(b, rows):
    p = torch.zeros(rows, dtype=torch.float32, device=b.device)
    p[:b.numel()] = b.reshape(-1)
    return p


def pack_blob(desc, pi, vf, act_head, val_head, log_std) -> torch.Tensor:
    """The kernel's weight blob (f16env_policy_blob_layout) as one float32 tensor on the weights'
    device, from lists of (W[out][in], b[out]) per branch, the two heads and log_std[4]."""
    off, total = policy_blob_layout(desc)
    f32 = lambda t: torch.as_tensor(t).detach().to(torch.float32)  # noqa: E731
    pieces, pos = [], 0

    def put(slot, t):
        nonlocal pos
        if off[slot] != pos:
            raise AssertionError("blob layout: slot %d at %d, packer at %d" % (slot, off[slot], pos))
        pieces.append(t)
        pos += t.numel()

    for b, (layers, widths, n) in enumerate(((pi, desc.pi_width, desc.n_pi), (vf, desc.vf_width, desc.n_vf))):
        if len(layers) != n:
            raise ValueError("%s branch: %d layers given, descriptor has %d" % ("vf" if b else "pi", len(layers), n))
        fan_in = desc.K * desc.D
        for l, (w, bias) in enumerate(layers):
            w, bias = f32(w), f32(bias)
            if w.shape[0] != widths[l] or bias.numel() != widths[l]:
                raise ValueError("layer %d of the %s branch is not %d wide" % (l, "vf" if b else "pi", widths[l]))
            put(6 * b + 2 * l, _pack_weight(w, fan_in, widths[l]))
            put(6 * b + 2 * l + 1, _pack_bias(bias, widths[l]))
            fan_in = widths[l]
    for (w, bias), outs, sw, sb, fan_in in ((act_head, ACT_DIM, F16_POLICY_OFF_ACT_W, F16_POLICY_OFF_ACT_B,
                                             desc.pi_width[desc.n_pi - 1]),
                                            (val_head, 1, F16_POLICY_OFF_VAL_W, F16_POLICY_OFF_VAL_B,
                                             desc.vf_width[desc.n_vf - 1])):
        w, bias = f32(w), f32(bias)
        if w.shape[0] != outs or bias.numel() != outs:
            raise ValueError("head must have %d outputs, got %s" % (outs, tuple(w.shape)))
        put(sw, _pack_weight(w, fan_in, 32))
        put(sb, _pack_bias(bias, 32))
    ls = f32(log_std).reshape(-1)
    if ls.numel() != ACT_DIM:
        raise ValueError("log_std must hold %d values" % ACT_DIM)
    put(F16_POLICY_OFF_LOG_STD, ls)
    dev = pieces[0].device
    blob = torch.cat([p.to(dev) for p in pieces])
    assert blob.numel() == total and len(off) == F16_POLICY_N_OFFSETS
    return blob


class DevicePolicy:
    """An SB3-shaped actor-critic MLP policy as one HIP launch per forward.

    pol(obs, step=None) -> (actions (n, 4), values (n,), log_probs (n,)); pol.value(obs) -> values;
    pol.predict(obs, deterministic=True) -> actions. obs: any (n, K, D) float32 device tensor with
    unit last stride (a windowed observation view is read in place). The Gaussian noise comes from
    the device Philox stream keyed by (seed; env_id_base + row, step): `step` defaults to a call
    counter, and shards that pass their env_id_base draw the rows of one big run."""

    def __init__(self, desc, device, seed: int = 0, env_id_base: int = 0):
        self.desc = desc
        self.device = torch.device(device)
        self.k, self.d = int(desc.K), int(desc.D)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.env_id_base = int(env_id_base)
        self.calls = 0
        self.offsets, self.n_floats = policy_blob_layout(desc)
        self.blob = torch.zeros(self.n_floats, dtype=torch.float32, device=self.device)
        self._desc_ref = ctypes.byref(desc)
        if self.device.type == "cuda":
            from ._lib import check, lib
            self._fwd = lib().f16env_policy_forward
            with torch.cuda.device(self.device):  # n = 0: prepares the kernel instance, launches nothing
                check(self._fwd(None, self._desc_ref, None, 0, None, 0, 0, 0, 0, 0, None, None, None, None, 0),
                      "f16env_policy_forward")

    # ------------------------------------------------------------------------------------------
    @classmethod
    def from_layers(cls, pi, vf, act_head, val_head, log_std, stack_k: int, frame_dim: int = 15,
                    activation: str = "tanh", device=None, seed: int = 0, env_id_base: int = 0):
        """pi / vf: lists of (W[out][in], b[out]) tensors; act_head / val_head: (W, b); log_std[4]."""
        desc = policy_desc(stack_k, frame_dim, [w.shape[0] for w, _ in pi], [w.shape[0] for w, _ in vf], activation)
        p = cls(desc, device if device is not None else pi[0][0].device, seed, env_id_base)
        p.load(pi, vf, act_head, val_head, log_std)
        return p

    @classmethod
    def from_state_dict(cls, sd, stack_k: int, frame_dim: int = 15, activation: str = "tanh", device=None,
                        seed: int = 0, env_id_base: int = 0):
        """From stable_baselines3's ActorCriticPolicy.state_dict() (key names only; SB3 not imported)."""
        return cls.from_layers(*layers_from_state_dict(sd), stack_k=stack_k, frame_dim=frame_dim,
                               activation=activation, device=device, seed=seed, env_id_base=env_id_base)

    def load(self, pi, vf, act_head, val_head, log_std):
        """Repack the weights into the same device blob (after a PPO update): one stream-ordered
        copy; captured graphs and bound pointers stay valid."""
        self.blob.copy_(pack_blob(self.desc, pi, vf, act_head, val_head, log_std), non_blocking=True)
        return self

    def load_state_dict(self, sd):
        return self.load(*layers_from_state_dict(sd))

    # ------------------------------------------------------------------------------------------
    def _check_obs(self, obs):
        if not isinstance(obs, torch.Tensor) or obs.device != self.device or obs.device.type != "cuda" \
                or obs.dtype != torch.float32 or obs.dim() != 3 or tuple(obs.shape[1:]) != (self.k, self.d) \
                or obs.stride(2) != 1 or obs.stride(0) < 0 or obs.stride(1) < 0:
            raise ValueError("obs must be a float32 (n, %d, %d) tensor on %s with unit last stride, got %s"
                             % (self.k, self.d, self.device, _describe(obs)))
        return int(obs.shape[0])

    def _check_out(self, x, shape, name, align):
        if not isinstance(x, torch.Tensor) or x.device != self.device or x.dtype != torch.float32 \
                or not x.is_contiguous() or tuple(x.shape) != tuple(shape) or x.data_ptr() % align:
            raise ValueError("%s must be a contiguous %d-byte aligned float32 %s tensor on %s"
                             % (name, align, tuple(shape), self.device))

    def _launch(self, obs, n, step, eps, actions, values, log_probs, flags):
        from ._lib import check
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        check(self._fwd(stream, self._desc_ref, self.blob.data_ptr(), n, obs.data_ptr(), obs.stride(0), obs.stride(1),
                        self.seed, int(step) & 0xFFFFFFFFFFFFFFFF, self.env_id_base,
                        None if eps is None else eps.data_ptr(), None if actions is None else actions.data_ptr(),
                        values.data_ptr(), None if log_probs is None else log_probs.data_ptr(), flags),
              "f16env_policy_forward")

    def forward_into(self, obs, step, actions, values, log_probs, eps=None, deterministic=False):
        """The forward with caller-owned outputs: actions (n, 4) 16-B aligned, values (n,),
        log_probs (n,), contiguous float32 (e.g. rows of a rollout buffer)."""
        n = self._check_obs(obs)
        self._check_out(actions, (n, ACT_DIM), "actions", 16)
        self._check_out(values, (n,), "values", 4)
        self._check_out(log_probs, (n,), "log_probs", 4)
        if eps is not None:
            self._check_out(eps, (n, ACT_DIM), "eps", 16)
        self._launch(obs, n, step, eps, actions, values, log_probs, F16_POLICY_DETERMINISTIC if deterministic else 0)

    def __call__(self, obs, step=None, eps=None, deterministic=False):
        n = self._check_obs(obs)
        if step is None:
            step = self.calls
            self.calls += 1
        actions = torch.empty((n, ACT_DIM), dtype=torch.float32, device=self.device)
        values = torch.empty(n, dtype=torch.float32, device=self.device)
        log_probs = torch.empty(n, dtype=torch.float32, device=self.device)
        self.forward_into(obs, step, actions, values, log_probs, eps=eps, deterministic=deterministic)
        return actions, values, log_probs

    def value(self, obs, out=None):
        n = self._check_obs(obs)
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=self.device)
        else:
            self._check_out(out, (n,), "out", 4)
        self._launch(obs, n, 0, None, None, out, None, F16_POLICY_VALUE_ONLY)
        return out

    def predict(self, obs, deterministic: bool = True):
        """BasePolicy.predict's action for a batch (the mean when deterministic)."""
        return self(obs, deterministic=deterministic)[0]


def _describe(x):
    if not isinstance(x, torch.Tensor):
        return type(x).__name__
    return "%s %s strides %s on %s" % (x.dtype, tuple(x.shape), tuple(x.stride()), x.device)
