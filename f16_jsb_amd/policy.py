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

It also learns in place (f16env_policy_backward): the blob is the parameter, `evaluate_actions`
is differentiable with respect to it through one backward kernel, and the optimiser runs on it:

    pol.requires_grad_(); opt = torch.optim.Adam(pol.parameters(), lr=3e-4, eps=1e-5)
    v, log_prob, entropy = pol.evaluate_actions(mb.observations, mb.actions)
    loss = ...; opt.zero_grad(); loss.backward(); clip_grad_norm_(pol.parameters(), 0.5); opt.step()

No stable_baselines3 import: only its key names. No fallback: without the library it raises.
"""
from __future__ import annotations

import ctypes

import torch

from ._lib import check, fn
from .abi import (F16_POLICY_DETERMINISTIC, F16_POLICY_N_OFFSETS, F16_POLICY_OFF_ACT_B, F16_POLICY_OFF_ACT_W,
                  F16_POLICY_OFF_LOG_STD, F16_POLICY_OFF_VAL_B, F16_POLICY_OFF_VAL_W, F16_POLICY_VALUE_ONLY,
                  policy_blob_layout, policy_desc)
from .buffers import need_tensor, stream_ptr

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


def _unpack_weight(blob, at, fan_in, rows):
    """The inverse of _pack_weight for the piece at blob[at:]: W[rows][fan_in], a view (callers clone)."""
    nks = (fan_in + 1) // 2
    w = blob[at:at + (rows // 32) * nks * 64].reshape(rows // 32, nks, 2, 32)
    return w.permute(0, 3, 1, 2).reshape(rows, 2 * nks)[:, :fan_in]


def _pack_bias(b, rows):
    p = torch.zeros(rows, dtype=torch.float32, device=b.device)
    p[:b.numel()] = b.reshape(-1)
    return p


def pack_blob(desc, pi, vf, act_head, val_head, log_std, fan_in0=None) -> torch.Tensor:
    """The kernel's weight blob (f16env_policy_blob_layout) as one float32 tensor on the weights'
    device, from lists of (W[out][in], b[out]) per branch, the two heads and log_std[4]. fan_in0:
    the first layers' fan-in when it is not K D (an LMA policy's MLPs read the extractor's features)."""
    off, total = policy_blob_layout(desc, fan_in0)
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
        fan_in = desc.K * desc.D if fan_in0 is None else int(fan_in0)
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


def unpack_blob(desc, blob, fan_in0=None):
    """The inverse of pack_blob, on the blob's device: (pi, vf, act_head, val_head, log_std) with
    pi / vf lists of (W[out][in], b[out]) and the heads at their true 4 / 1 rows. Copies, not
    views. A gradient in blob layout (pol.blob.grad) reads per layer the same way."""
    off, total = policy_blob_layout(desc, fan_in0)
    blob = torch.as_tensor(blob).detach()
    if blob.dim() != 1 or blob.numel() != total:
        raise ValueError("a blob of %d floats was expected, got shape %s" % (total, tuple(blob.shape)))

    def piece(slot, rows, outs, fan_in):
        bias = blob[off[slot + 1]:off[slot + 1] + outs]
        return _unpack_weight(blob, off[slot], fan_in, rows)[:outs].clone(), bias.clone()

    branches = []
    for b, (widths, n) in enumerate(((desc.pi_width, desc.n_pi), (desc.vf_width, desc.n_vf))):
        layers, fan_in = [], desc.K * desc.D if fan_in0 is None else int(fan_in0)
        for l in range(n):
            layers.append(piece(6 * b + 2 * l, widths[l], widths[l], fan_in))
            fan_in = widths[l]
        branches.append(layers)
    act_head = piece(F16_POLICY_OFF_ACT_W, 32, ACT_DIM, desc.pi_width[desc.n_pi - 1])
    val_head = piece(F16_POLICY_OFF_VAL_W, 32, 1, desc.vf_width[desc.n_vf - 1])
    ls = off[F16_POLICY_OFF_LOG_STD]
    return branches[0], branches[1], act_head, val_head, blob[ls:ls + ACT_DIM].clone()


def state_dict_from_layers(pi, vf, act_head, val_head, log_std):
    """The layers under SB3's ActorCriticPolicy key names (what layers_from_state_dict reads)."""
    sd = {}
    for name, layers in (("policy_net", pi), ("value_net", vf)):
        for i, (w, b) in enumerate(layers):
            sd["mlp_extractor.%s.%d.weight" % (name, 2 * i)] = w
            sd["mlp_extractor.%s.%d.bias" % (name, 2 * i)] = b
    sd["action_net.weight"], sd["action_net.bias"] = act_head
    sd["value_net.weight"], sd["value_net.bias"] = val_head
    sd["log_std"] = log_std
    return sd


class _MeanAndValue(torch.autograd.Function):
    """(mean, values) of the blob at obs: the forward kernel (deterministic: its action is the
    mean), and f16env_policy_backward as the gradient with respect to the blob."""

    @staticmethod
    def forward(ctx, blob, obs, pol):
        ctx.pol = pol
        ctx.set_materialize_grads(False)  # an unused output's branch is skipped by the kernel, not fed zeros
        ctx.save_for_backward(blob, obs)  # (torch's version check: a step or env write before backward raises)
        return pol._mean_and_value(obs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_mean, d_values):
        _, obs = ctx.saved_tensors  # (unpacking is the version check; the kernel reads pol.blob, the same storage)
        pol = ctx.pol

        def dense(g):  # (a broadcast or sliced upstream gradient: one copy makes it the kernel's input)
            if g is None:
                return None
            g = g.contiguous()
            return g.clone() if g.data_ptr() % 16 else g
        return pol.backward_blob(obs, dense(d_mean), dense(d_values)), None, None


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
        self._desc_ref = ctypes.byref(desc)
        self.offsets, self.n_floats = self._layout()
        self.blob = torch.zeros(self.n_floats, dtype=torch.float32, device=self.device)
        self._bwd_fns = None
        if self.device.type == "cuda":
            self._fwd = fn(self._FWD)
            with torch.cuda.device(self.device):  # n = 0: prepares the kernel instance, launches nothing
                check(self._fwd(None, *self._desc_args(), None, 0, None, 0, 0, 0, 0, 0, None, None, None, None,
                                *(None,) * self._FWD_MORE, 0), self._FWD)

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
        with torch.no_grad():  # (the blob may be a leaf that requires grad)
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

    def _launch(self, obs, n, step, eps, actions, values, log_probs, flags, *more):
        """more: the entry point's further output tensors (_FWD_MORE of them; those not given are NULL)."""
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        more += (None,) * (self._FWD_MORE - len(more))
        check(self._fwd(stream_ptr(self.device), *self._desc_args(), self.blob.data_ptr(), n, obs.data_ptr(), obs.stride(0),
                        obs.stride(1), self.seed, int(step) & 0xFFFFFFFFFFFFFFFF, self.env_id_base, ptr(eps), ptr(actions),
                        values.data_ptr(), ptr(log_probs), *map(ptr, more), flags), self._FWD)

    def forward_into(self, obs, step, actions, values, log_probs, eps=None, deterministic=False):
        """The forward with caller-owned outputs: actions (n, 4) 16-B aligned, values (n,),
        log_probs (n,), contiguous float32 (e.g. rows of a rollout buffer)."""
        n = self._check_obs(obs)
        need_tensor(actions, (n, ACT_DIM), torch.float32, self.device, "actions", 16)
        need_tensor(values, (n,), torch.float32, self.device, "values", 4)
        need_tensor(log_probs, (n,), torch.float32, self.device, "log_probs", 4)
        if eps is not None:
            need_tensor(eps, (n, ACT_DIM), torch.float32, self.device, "eps", 16)
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
            need_tensor(out, (n,), torch.float32, self.device, "out", 4)
        self._launch(obs, n, 0, None, None, out, None, F16_POLICY_VALUE_ONLY)
        return out

    def predict(self, obs, deterministic: bool = True):
        """BasePolicy.predict's action for a batch (the mean when deterministic)."""
        return self(obs, deterministic=deterministic)[0]

    # ------------------------------------------------------------------------------------------
    # learning: the blob is the parameter (f16env_policy_backward writes its gradient in blob layout)
    def parameters(self):
        """[blob]: torch.optim.Adam(pol.parameters()) and clip_grad_norm_(pol.parameters(), c) are
        SB3's optimiser and clipping element for element -- Adam is elementwise, the pads have zero
        gradient and zero state, and the norm of the packed gradient is the norm of the layers'."""
        return [self.blob]

    def requires_grad_(self, flag: bool = True):
        self.blob.requires_grad_(flag)
        return self

    def state_dict(self):
        """The blob's layers under SB3's key names (model.policy.load_state_dict(pol.state_dict()))."""
        return state_dict_from_layers(*unpack_blob(self.desc, self.blob))

    # the entry points, the forward's output pointers past log_probs, the descriptor arguments all of
    # them take and the blob's (offsets, floats): what an LMA policy replaces
    _FWD, _FWD_MORE = "f16env_policy_forward", 0
    _BWD = ("f16env_policy_backward_workspace", "f16env_policy_backward")

    def _desc_args(self):
        return (self._desc_ref,)

    def _layout(self):
        return policy_blob_layout(self.desc)

    def _backward_fns(self):
        if self._bwd_fns is None:  # (taken at the first gradient: an older library still runs the forward)
            self._bwd_fns = fn(self._BWD[0]), fn(self._BWD[1])
        return self._bwd_fns

    def reserve_backward(self, n: int, max_blocks: int = 0):
        """Size the cached workspace for gradients of up to n rows and prepare the kernel instance
        (call it ahead of a stream capture: nothing may be allocated inside one)."""
        ws_fn, bwd = self._backward_fns()
        need = ctypes.c_int64(0)
        check(ws_fn(*self._desc_args(), int(n), int(max_blocks), ctypes.byref(need)), self._BWD[0])
        have = getattr(self, "_bwd_ws", None)
        if have is None or have.numel() < need.value:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the backward workspace must grow inside a stream capture: call "
                                   "reserve_backward(n, max_blocks) ahead of it")
            self._bwd_ws = torch.empty(max(need.value, 16), dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                check(bwd(None, *self._desc_args(), None, 0, None, 0, 0, None, None, None, 0, int(max_blocks), None),
                      self._BWD[1])
        return self._bwd_ws

    def backward_blob(self, obs, d_mean=None, d_values=None, max_blocks: int = 0, out=None):
        """sum over rows of d_mean . d mean / d blob + d_values d value / d blob as a tensor in blob
        layout (two launches; pads and log_std slots +0). d_mean (n, 4) 16-B aligned, d_values (n,),
        contiguous float32 on the device, either may be None (that branch's gradient is zero)."""
        n = self._check_obs(obs)
        if obs.requires_grad:
            raise ValueError("no gradient is formed with respect to obs: pass a tensor that does not require grad")
        if d_mean is None and d_values is None:
            raise ValueError("d_mean and d_values are both None")
        if d_mean is not None:
            need_tensor(d_mean, (n, ACT_DIM), torch.float32, self.device, "d_mean", 16)
        if d_values is not None:
            need_tensor(d_values, (n,), torch.float32, self.device, "d_values", 4)
        if out is None:
            out = torch.empty(self.n_floats, dtype=torch.float32, device=self.device)
        else:
            need_tensor(out, (self.n_floats,), torch.float32, self.device, "out", 16)
        if n == 0:
            return out.zero_()
        ws = self.reserve_backward(n, max_blocks)
        check(self._backward_fns()[1](stream_ptr(self.device), *self._desc_args(), self.blob.data_ptr(), n, obs.data_ptr(),
                                      obs.stride(0), obs.stride(1), None if d_mean is None else d_mean.data_ptr(),
                                      None if d_values is None else d_values.data_ptr(), ws.data_ptr(), ws.numel(),
                                      int(max_blocks), out.data_ptr()), self._BWD[1])
        return out

    def _mean_and_value(self, obs):
        n = self._check_obs(obs)
        mean = torch.empty((n, ACT_DIM), dtype=torch.float32, device=self.device)
        values = torch.empty(n, dtype=torch.float32, device=self.device)
        log_probs = torch.empty(n, dtype=torch.float32, device=self.device)
        self._launch(obs, n, 0, None, mean, values, log_probs, F16_POLICY_DETERMINISTIC)
        return mean, values

    def mean_and_value(self, obs):
        """(mean (n, 4), values (n,)), differentiable with respect to the blob when it requires
        grad (the backward is one kernel, once differentiable); without grad mode just the forward."""
        if isinstance(obs, torch.Tensor) and obs.requires_grad:
            raise ValueError("no gradient is formed with respect to obs: pass a tensor that does not require grad")
        if not (torch.is_grad_enabled() and self.blob.requires_grad):
            return self._mean_and_value(obs)
        return _MeanAndValue.apply(self.blob, obs, self)

    def evaluate_actions(self, obs, actions):
        """ActorCriticPolicy.evaluate_actions for the DiagGaussianDistribution (policies.py,
        distributions.py): (values (n,), log_prob (n,), entropy (n,)). log_std is a view of the
        blob, so its gradient reaches blob.grad through autograd's own slice backward."""
        mean, values = self.mean_and_value(obs)
        ls = self.offsets[F16_POLICY_OFF_LOG_STD]
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * self.blob[ls:ls + ACT_DIM].exp())
        return values, dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)


def _describe(x):
    if not isinstance(x, torch.Tensor):
        return type(x).__name__
    return "%s %s strides %s on %s" % (x.dtype, tuple(x.shape), tuple(x.stride()), x.device)
