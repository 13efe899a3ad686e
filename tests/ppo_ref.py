"""Checkers of the device PPO update (f16env_ppo_loss_head, f16env_ppo_adam_step, f16_jsb_amd.ppo):
the loss head in closed form in a given dtype, the same by torch autograd over the leaves (mean,
values, log_std), gradient clipping + Adam in fp64 and by torch on the CPU, the data generator with
planted ratios, and the project's 4 x torch rule on plain tensors. No test lives here."""
from __future__ import annotations

import math

import numpy as np
import torch

import policy_grad_ref as G

HYPER = ("lr", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "beta1", "beta2", "eps")
STATS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction")
RATIOS = (0.6, 0.75, 0.9, 1.0, 1.1, 1.25, 1.5)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def hyper(**kw):
    """The hyper-parameters as Python floats that are exact in float32 (the device array is float32:
    every reference then works from the very values the kernels read)."""
    h = dict(lr=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, beta1=0.9, beta2=0.999, eps=1e-5)
    assert set(kw) <= set(h)
    h.update(kw)
    return {key: float(np.float32(h[key])) for key in HYPER}


def hyper_tensor(h, device):
    return torch.tensor([h[key] for key in HYPER], dtype=torch.float32, device=device)


def log_prob64(mean, actions, log_std):
    m, a, ls = (t.double() for t in (mean, actions, log_std))
    return (-(a - m) ** 2 / (2.0 * torch.exp(2.0 * ls)) - ls - HALF_LOG_2PI).sum(dim=1)


def head_data(n, seed=0, clip_range=None):
    """n rows of float32 head inputs with a planted ratio per row: mean, values, actions, advantages,
    returns standard normal, log_std 0.1 N(0, 1), old_log_prob = lp64 - log(rho) with rho from RATIOS
    times (1 + u), |u| <= 0.01. No row is dropped or re-drawn. Asserts that every row's fp64 ratio
    (from the rounded old_log_prob) is at least 1e-3 from both clip edges, and for n >= 129 that the
    in-range class and all four (sign of the advantage) x (above / below the range) classes are
    populated, for the raw and for the normalised advantages."""
    c = hyper()["clip_range"] if clip_range is None else clip_range
    rng = np.random.default_rng(7000 + 13 * n + seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))  # noqa: E731
    d = {"mean": f32(rng.standard_normal((n, 4))), "values": f32(rng.standard_normal(n)),
         "actions": f32(rng.standard_normal((n, 4))), "advantages": f32(rng.standard_normal(n)),
         "returns": f32(rng.standard_normal(n)), "log_std": f32(0.1 * rng.standard_normal(4))}
    rho = rng.choice(RATIOS, n) * (1.0 + rng.uniform(-0.01, 0.01, n))
    lp64 = log_prob64(d["mean"], d["actions"], d["log_std"])
    d["old_log_prob"] = (lp64 - torch.from_numpy(np.log(rho))).float()
    ratio = torch.exp(lp64 - d["old_log_prob"].double())
    assert ((ratio - (1 - c)).abs() >= 1e-3).all() and ((ratio - (1 + c)).abs() >= 1e-3).all()
    if n >= 129:
        a = d["advantages"].double()
        for adv in (a, (a - a.mean()) / (a.std() + 1e-8)):
            assert ((ratio > 1 - c) & (ratio < 1 + c)).any()
            for pos in (True, False):
                for above in (True, False):
                    assert (((adv > 0) == pos) & ((ratio > 1 + c) if above else (ratio < 1 - c))).any(), (pos, above)
    d["ratio64"] = ratio
    return d


def _adv(a, normalize):
    return (a - a.mean()) / (a.std() + 1e-8) if normalize and a.numel() > 1 else a


def head_closed_form(d, h, normalize, dtype=torch.float64, clip_mask=True):
    """The loss head as include/f16env.h writes it, vectorised in `dtype`: {d_mean, d_values,
    d_log_std, clipped (bool rows), stats (6, STATS order)}. clip_mask=False: the surrogate's
    derivative is the advantage on every row (the negative control)."""
    c = lambda key: d[key].to(dtype)  # noqa: E731
    mean, values, actions, ls = c("mean"), c("values"), c("actions"), c("log_std")
    n, clip = values.numel(), h["clip_range"]
    sigma = torch.exp(ls)
    diff = actions - mean
    lp = (-(diff ** 2) / (2 * sigma ** 2) - ls - HALF_LOG_2PI).sum(dim=1)
    adv = _adv(c("advantages"), normalize)
    log_r = lp - c("old_log_prob")
    r = torch.exp(log_r)
    s1, s2 = adv * r, adv * torch.clamp(r, 1 - clip, 1 + clip)
    open_ = ((r >= 1 - clip) & (r <= 1 + clip)) | (s1 < s2)
    ds_dr = torch.where(open_, adv, torch.zeros_like(adv)) if clip_mask else adv
    g = -(1.0 / n) * ds_dr * r
    z = diff / sigma
    policy_loss, value_loss = -torch.min(s1, s2).mean(), ((values - c("returns")) ** 2).mean()
    entropy_loss = -(0.5 + HALF_LOG_2PI + ls).sum()
    stats = torch.stack([policy_loss, value_loss, entropy_loss,
                         policy_loss + h["ent_coef"] * entropy_loss + h["vf_coef"] * value_loss,
                         ((r - 1) - log_r).mean(), ((r - 1).abs() > clip).to(dtype).mean()])
    return {"d_mean": g[:, None] * diff / sigma ** 2, "d_values": h["vf_coef"] * 2 * (values - c("returns")) / n,
            "d_log_std": (g[:, None] * (z ** 2 - 1)).sum(dim=0) - h["ent_coef"], "clipped": ~open_, "stats": stats}


def head_autograd(d, h, normalize, dtype=torch.float64):
    """The same by torch autograd on the CPU in `dtype` over the leaves (mean, values, log_std):
    SB3's DiagGaussianDistribution and, where the advantages are normalised,
    policy_grad_ref.ppo_loss itself; with raw advantages (normalize off, or one row) its body with
    the advantage left as it is."""
    leaf = lambda key: d[key].detach().to(dtype).clone().requires_grad_(True)  # noqa: E731
    c = lambda key: d[key].to(dtype)  # noqa: E731
    mean, values, ls = leaf("mean"), leaf("values"), leaf("log_std")
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * ls.exp())
    lp, ent = dist.log_prob(c("actions")).sum(dim=1), dist.entropy().sum(dim=1)
    clip = h["clip_range"]
    if normalize and values.numel() > 1:
        loss, ratio = G.ppo_loss(values, lp, ent, c("advantages"), c("returns"), c("old_log_prob"), clip,
                                 h["ent_coef"], h["vf_coef"])
    else:
        adv = c("advantages")
        ratio = torch.exp(lp - c("old_log_prob"))
        loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean() \
            + h["ent_coef"] * (-ent.mean()) + h["vf_coef"] * torch.nn.functional.mse_loss(c("returns"), values)
    loss.backward()
    with torch.no_grad():
        adv = _adv(c("advantages"), normalize)
        log_r = lp - c("old_log_prob")
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
        value_loss = torch.nn.functional.mse_loss(c("returns"), values)
        stats = torch.stack([policy_loss, value_loss, -ent.mean(), loss.detach(), ((ratio - 1) - log_r).mean(),
                             ((ratio - 1).abs() > clip).to(dtype).mean()])
    return {"d_mean": mean.grad, "d_values": values.grad, "d_log_std": ls.grad, "stats": stats}


# ---------------------------------------------------------------------------------------------
def adam_ref64(blob, grads, h, m=None, v=None, step=0):
    """clip_grad_norm_(max_grad_norm) + torch.optim.Adam (no amsgrad, no weight decay) in fp64 from
    float32 inputs, one step per gradient in `grads`: [(blob, exp_avg, exp_avg_sq)] after each."""
    p = blob.detach().double().cpu().clone()
    m = torch.zeros_like(p) if m is None else m.detach().double().cpu().clone()
    v = torch.zeros_like(p) if v is None else v.detach().double().cpu().clone()
    out = []
    for g in grads:
        g = g.detach().double().cpu()
        step += 1
        g = g * min(1.0, h["max_grad_norm"] / (math.sqrt(float((g * g).sum())) + 1e-6))
        m = h["beta1"] * m + (1 - h["beta1"]) * g
        v = h["beta2"] * v + (1 - h["beta2"]) * g * g
        p = p - (h["lr"] / (1 - h["beta1"] ** step)) * m / (v.sqrt() / math.sqrt(1 - h["beta2"] ** step) + h["eps"])
        out.append((p.clone(), m.clone(), v.clone()))
    return out


def adam_torch32(blob, grads, h):
    """The same by torch on the CPU in float32: clip_grad_norm_ + torch.optim.Adam over [blob]."""
    p = blob.detach().float().cpu().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    out = []
    for g in grads:
        p.grad = g.detach().float().cpu().clone()
        torch.nn.utils.clip_grad_norm_([p], h["max_grad_norm"])
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return out


def adam_gradients(desc, k, d, pi_w, vf_w, h):
    """Three random gradients in blob layout (pads zero), scaled to norms of 0.5, 3 and 8 times
    max_grad_norm: the first is not clipped, the others are."""
    from f16_jsb_amd.policy import pack_blob
    out = []
    for step, scale in enumerate((0.5, 3.0, 8.0)):
        g = pack_blob(desc, *G.tanh_data(k, d, pi_w, vf_w, 1, seed=2 + step)[0])
        out.append((g * (scale * h["max_grad_norm"] / g.double().norm().item())).float())
    return out


# ---------------------------------------------------------------------------------------------
def rule(got, ref64, torch32):
    """policy_grad_ref.rule_of_four on one plain tensor: (err of got, allowance)."""
    nest = lambda x: ([], [], (x, x), (x, x), x)  # noqa: E731
    return G.rule_of_four(nest(got), nest(ref64), nest(torch32))["log_std"]


def check(label, got, ref64, torch32, bad):
    err, allow = rule(got, ref64, torch32)
    print("%s: kernel %.3e allowed %.3e ratio of torch's %.2f" % (label, err, allow, 4.0 * err / allow if allow else 0.0))
    if not err <= allow:
        bad.append((label, err, allow))
