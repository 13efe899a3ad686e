"""Checkers of the device policy's backward (f16env_policy_backward, include/f16env.h): an fp64
vector-Jacobian product by torch autograd over plain layers, an exact integer one in numpy int64
(ReLU), the integer data on which every float32 partial sum is exact in any order, the documented
rule for the backward's waves per block, and the PPO loss the autograd test and
tools/policy_backward_ab.py share. No test lives here."""
from __future__ import annotations

import numpy as np
import torch

LDS_BYTES = 160 * 1024
IMAGE_STRIDE = 33          # floats per unit of every LDS image of the backward (32 rows + 1)
EXACT = 1 << 24            # integers of magnitude below 2^24 are exact in float32


def backward_waves(k, d, pi_widths, vf_widths):
    """(waves per block, LDS bytes per wave) of the backward, by DESIGN section 4's rule: a wave
    keeps the observation image (K D rounded up to even inputs), the activation images of the wider
    branch (the sum of its widths) and a delta image (the widest layer), all at 33 floats per unit;
    the block has the most of 4, 2, 1 waves whose images fit 160 KiB."""
    in_dim = k * d
    units = in_dim + in_dim % 2 + max(sum(pi_widths), sum(vf_widths)) + max(list(pi_widths) + list(vf_widths))
    per_wave = 4 * IMAGE_STRIDE * units
    for waves in (4, 2, 1):
        if waves * per_wave <= LDS_BYTES:
            return waves, per_wave
    return 0, per_wave


# ---------------------------------------------------------------------------------------------
# the network in plain torch (any dtype / device): what the kernel's forward computes
def mean_and_value(x, pi, vf, act_head, val_head, activation):
    act = torch.tanh if activation == "tanh" else torch.relu
    x = x.reshape(x.shape[0], -1)
    hp = hv = x
    for w, b in pi:
        hp = act(torch.nn.functional.linear(hp, w, b))
    for w, b in vf:
        hv = act(torch.nn.functional.linear(hv, w, b))
    return torch.nn.functional.linear(hp, *act_head), torch.nn.functional.linear(hv, *val_head)[:, 0]


def evaluate_actions(x, actions, pi, vf, act_head, val_head, log_std, activation):
    """SB3's ActorCriticPolicy.evaluate_actions for a DiagGaussianDistribution."""
    mean, values = mean_and_value(x, pi, vf, act_head, val_head, activation)
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
    return values, dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1)


def ppo_loss(values, log_prob, entropy, advantages, returns, old_log_prob, clip_range=0.2, ent_coef=0.01, vf_coef=0.5):
    """Standard PPO's minibatch loss (normalised advantages, no value clipping): the clipped
    surrogate, the entropy bonus and the value loss. Returns (loss, ratio)."""
    adv = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    value_loss = torch.nn.functional.mse_loss(returns, values)
    return policy_loss + ent_coef * (-entropy.mean()) + vf_coef * value_loss, ratio


def as_params(net, dtype, device="cpu"):
    """A net (pi, vf, act_head, val_head, log_std) as fresh leaves of `dtype` that require grad."""
    leaf = lambda t: torch.as_tensor(t).detach().to(device=device, dtype=dtype).clone().requires_grad_(True)  # noqa: E731
    pi, vf, act, val, ls = net
    return ([(leaf(w), leaf(b)) for w, b in pi], [(leaf(w), leaf(b)) for w, b in vf],
            (leaf(act[0]), leaf(act[1])), (leaf(val[0]), leaf(val[1])), leaf(ls))


def grads_of(params):
    """The .grad of as_params' leaves in the same nesting (zeros where autograd reached nothing)."""
    g = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    pi, vf, act, val, ls = params
    return ([(g(w), g(b)) for w, b in pi], [(g(w), g(b)) for w, b in vf], (g(act[0]), g(act[1])),
            (g(val[0]), g(val[1])), g(ls))


def named_tensors(net):
    """[(name, tensor)] of a net or a gradient in as_params' nesting: the per-tensor comparisons."""
    pi, vf, act, val, ls = net
    out = []
    for name, layers in (("pi", pi), ("vf", vf)):
        for l, (w, b) in enumerate(layers):
            out += [("%s%d.weight" % (name, l), w), ("%s%d.bias" % (name, l), b)]
    return out + [("act.weight", act[0]), ("act.bias", act[1]), ("val.weight", val[0]), ("val.bias", val[1]),
                  ("log_std", ls)]


def vjp(net, obs, d_mean, d_values, activation, dtype=torch.float64):
    """sum_b d_mean[b] . d mean[b] / d theta + d_values[b] d value[b] / d theta by torch autograd on
    the CPU in `dtype`, in the net's nesting (log_std's is zero). d_mean / d_values may be None."""
    p = as_params(net, dtype)
    x = torch.as_tensor(obs).to(dtype)
    mean, values = mean_and_value(x, *p[:4], activation)
    s = 0
    if d_mean is not None:
        s = s + (mean * torch.as_tensor(d_mean).to(dtype)).sum()
    if d_values is not None:
        s = s + (values * torch.as_tensor(d_values).to(dtype)).sum()
    s.backward()
    return grads_of(p)


# ---------------------------------------------------------------------------------------------
# exact integers
def _int_branch(x, layers, head, d_out, absolute):
    """One branch in int64 under ReLU: gradients [(gW, gb)] of the hidden layers then the head.
    absolute=True: the same walk on magnitudes with every mask open -- the sum of absolute values
    behind every activation, delta and gradient element (returned as their largest, too)."""
    w_of = (lambda w: np.abs(w)) if absolute else (lambda w: w)
    hs, zs, h, peak = [x], [], x, 0
    for w, b in layers:
        z = h @ w_of(w).T + w_of(b)
        zs.append(z)
        h = z if absolute else np.maximum(z, 0)
        hs.append(h)
        peak = max(peak, int(np.abs(z).max()))
    w, b = head
    peak = max(peak, int(np.abs(h @ w_of(w).T + w_of(b)).max()))
    delta, grads = d_out, []
    for l in range(len(layers), -1, -1):
        w = head[0] if l == len(layers) else layers[l][0]
        grads.append((delta.T @ hs[l], delta.sum(0)))
        peak = max(peak, int(np.abs(delta).max()), int(np.abs(grads[-1][0]).max()), int(np.abs(grads[-1][1]).max()))
        if l:
            delta = delta @ w_of(w)
            if not absolute:
                delta = delta * (zs[l - 1] > 0)  # ReLU'(0) = 0, as torch
    return grads[::-1], zs, peak


def int_vjp(net, obs, d_mean, d_values):
    """The exact vjp of a ReLU net on integer data (numpy int64), in the net's nesting, plus the
    pre-activations of both branches. d_mean / d_values None: that branch's gradient is zero."""
    i64 = lambda t: np.asarray(t).astype(np.int64)  # noqa: E731
    pi, vf, act, val, ls = net
    x = i64(obs).reshape(len(obs), -1)
    out, zs = [], []
    for layers, head, d_out, width in ((pi, act, d_mean, 4), (vf, val, d_values, 1)):
        d = np.zeros((len(x), width), np.int64) if d_out is None else i64(d_out).reshape(len(x), width)
        g, z, _ = _int_branch(x, [(i64(w), i64(b)) for w, b in layers], (i64(head[0]), i64(head[1])), d, False)
        out.append(g)
        zs += z
    return (out[0][:-1], out[1][:-1], out[0][-1], out[1][-1], np.zeros(4, np.int64)), zs


def int_peak(net, obs, d_mean, d_values):
    """The largest sum of absolute values behind any forward activation, delta or gradient element."""
    a64 = lambda t: np.abs(np.asarray(t).astype(np.int64))  # noqa: E731
    pi, vf, act, val, ls = net
    x = a64(obs).reshape(len(obs), -1)
    return max(_int_branch(x, [(a64(w), a64(b)) for w, b in layers], (a64(head[0]), a64(head[1])),
                           a64(d_out).reshape(len(x), -1), True)[2]
               for layers, head, d_out in ((pi, act, d_mean), (vf, val, d_values)))


NNZ = 4  # non-zero weights per unit: with |x| <= 2 and three layers of 128 the peak stays near 2^20 at n = 257


def int_data(k, d, pi_w, vf_w, n, seed=0):
    """(net, obs (n, k, d), d_mean (n, 4), d_values (n,)) as float32 tensors of small integers:
    observations in [-2, 2], per unit NNZ weights of +-1 at random inputs and a bias in [-1, 1],
    upstream gradients in [-2, 2]. Every entry is drawn independently, so no operand equals its
    transpose or a permutation of itself. Asserts the 2^24 condition (int_peak) and that some
    pre-activations are exactly 0 and some negative."""
    rng = np.random.default_rng(1000 * seed + 100 * k + d + sum(pi_w) + 7 * sum(vf_w))

    def layer(out, fan_in):
        w = np.zeros((out, fan_in), np.int64)
        for o in range(out):
            w[o, rng.choice(fan_in, NNZ, replace=False)] = rng.choice([-1, 1], NNZ)
        return w, rng.integers(-1, 2, out)

    def branch(widths):
        layers, fan_in = [], k * d
        for w in widths:
            layers.append(layer(w, fan_in))
            fan_in = w
        return layers
    pi, vf = branch(pi_w), branch(vf_w)
    net = (pi, vf, layer(4, pi_w[-1]), layer(1, vf_w[-1]), np.zeros(4, np.int64))
    obs = rng.integers(-2, 3, (n, k, d))
    d_mean, d_values = rng.integers(-2, 3, (n, 4)), rng.integers(-2, 3, n)
    assert int_peak(net, obs, d_mean, d_values) < EXACT
    zs = np.concatenate([z.ravel() for z in int_vjp(net, obs, d_mean, d_values)[1]])
    assert (zs == 0).any() and (zs < 0).any() and (zs > 0).any()
    f32 = lambda t: torch.from_numpy(np.asarray(t).astype(np.float32))  # noqa: E731
    net32 = ([(f32(w), f32(b)) for w, b in pi], [(f32(w), f32(b)) for w, b in vf], (f32(net[2][0]), f32(net[2][1])),
             (f32(net[3][0]), f32(net[3][1])), f32(net[4]))
    return net32, f32(obs), f32(d_mean), f32(d_values)


def tanh_data(k, d, pi_w, vf_w, n, seed=0):
    """The forward tests' nets: weights N(0, 2 / fan_in), biases N(0, 0.01), standard-normal rows
    and upstream gradients, float32."""
    rng = np.random.default_rng(2000 * seed + 100 * k + d + sum(pi_w) + 7 * sum(vf_w))
    f32 = lambda a: torch.from_numpy(a.astype(np.float32))  # noqa: E731

    def layer(out, fan_in):
        return f32(rng.standard_normal((out, fan_in)) * np.sqrt(2.0 / fan_in)), f32(rng.standard_normal(out) * 0.1)

    def branch(widths):
        layers, fan_in = [], k * d
        for w in widths:
            layers.append(layer(w, fan_in))
            fan_in = w
        return layers
    net = (branch(pi_w), branch(vf_w), layer(4, pi_w[-1]), layer(1, vf_w[-1]), f32(rng.standard_normal(4) * 0.1))
    return net, f32(rng.standard_normal((n, k, d))), f32(rng.standard_normal((n, 4))), f32(rng.standard_normal(n))


def pack(desc, grads):
    """A gradient in the net's nesting in blob layout (policy.pack_blob: float32)."""
    from f16_jsb_amd.policy import pack_blob
    t = lambda a: torch.as_tensor(np.asarray(a)) if not isinstance(a, torch.Tensor) else a  # noqa: E731
    pi, vf, act, val, ls = grads
    return pack_blob(desc, [(t(w), t(b)) for w, b in pi], [(t(w), t(b)) for w, b in vf], (t(act[0]), t(act[1])),
                     (t(val[0]), t(val[1])), t(ls))


def rule_of_four(got, ref64, torch32):
    """The project's precision rule per parameter tensor: {name: (err of got, allowance)} with
    allowance = 4 max(err of torch float32, 2^-24 max|ref|), errors as max abs against fp64."""
    out = {}
    for (name, g), (_, r), (_, t) in zip(named_tensors(got), named_tensors(ref64), named_tensors(torch32)):
        r = r.detach().double().cpu()
        err = (g.detach().double().cpu() - r).abs().max().item()
        terr = (t.detach().double().cpu() - r).abs().max().item()
        out[name] = (err, 4.0 * max(terr, 2.0 ** -24 * r.abs().max().item()))
    return out
