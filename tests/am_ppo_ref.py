"""Checkers of device AM-PPO (f16env_ppo_dynago_update, f16env_ppo_loss_head_am, f16env_ppo_dag_step):
the reference's stable_baselines3/ppo/ppo.py:29-99, :327-388 and ppo/optim/sgd.py:219-344, :437-498
restated from their lines in torch on the CPU, in a given dtype -- float64 is the reference, float32
is "what torch would have computed" for the project's 4 x rule. The reference's Python cannot be
imported here, so tests/test_am_ppo_cpu.py pins this restatement by known
answers. `defect=` plants one named mistake (the checker's negative controls). No test lives here."""
from __future__ import annotations

import math
import statistics

import numpy as np
import torch

import policy_grad_ref as G

DYNAGO = ("tau", "p_star", "kappa_controller", "eta", "rho", "eps", "alpha_min", "alpha_max", "rho_sat", "kappa", "v_shift")
DAG = ("tau", "p_star", "kappa", "beta", "eta", "rho", "eps", "alpha_min", "alpha_max", "k_val", "lambda_rms", "s_min",
       "gamma", "ema_beta", "warmup_steps", "sat_every", "alpha")
BAND = 2.0 ** -20  # relative half-width around tau inside which a saturation count may differ


def _exact32(d, names):
    return {key: float(np.float32(d[key])) for key in names}


def dynago(**kw):
    """ppo.py:141-154's defaults as Python floats exact in float32 (the device array is float32)."""
    p = dict(tau=1.25, p_star=0.10, kappa_controller=2.0, eta=0.3, rho=0.1, eps=1e-5, alpha_min=1e-12, alpha_max=1e12,
             rho_sat=0.98, kappa=2.0, v_shift=0.0)
    assert set(kw) <= set(p)
    p.update(kw)
    return _exact32(p, DYNAGO)


def dag_constants(**kw):
    """sgd.py:118-132's defaults, kappa = tau / Phi^-1(1 - p_star / 2), exact in float32."""
    c = dict(tau=1.25, p_star=0.10, kappa=None, beta=1.0 / 3.0, eta=0.3, rho=0.1, eps=1e-5, alpha_min=1e-12, alpha_max=1e12,
             k_val=2.0, lambda_rms=0.3, s_min=0.1, gamma=1.0, ema_beta=0.98, warmup_steps=500, sat_every=10, alpha=0.0)
    assert set(kw) <= set(c)
    c.update(kw)
    if c["kappa"] is None:
        c["kappa"] = c["tau"] / statistics.NormalDist().inv_cdf(1.0 - c["p_star"] / 2.0)
    return _exact32(c, DAG)


def as_f32(x):
    """A scalar rounded to float32 and back: what a float32 store keeps."""
    return float(np.float32(float(x)))


# ---------------------------------------------------------------------------------------------
# ppo.py:29-99
def controller(adv, p, state, dtype=torch.float64, defect=None):
    """dynago_transform_advantages(update_ema=True) on `adv` (float32) in `dtype`; state = (alpha,
    sat) as Python floats of float32 values. Returns {"alpha", "sat": the new state as stored
    (float32 values), "N", "sigma", "count", "band": the elements whose |Z| lies within BAND of tau}.
    numel <= 1 returns the state unchanged (:40-41)."""
    a = adv.detach().to(dtype).reshape(-1)
    alpha, sat = (torch.tensor(float(v), dtype=torch.float32).to(dtype) for v in state)
    if a.numel() <= 1:
        return {"alpha": float(alpha), "sat": float(sat), "count": 0, "band": 0}
    eps = p["eps"]
    N = torch.linalg.norm(a)
    sigma = torch.std(a) + eps                                                      # :61
    a_hat = p["kappa_controller"] * (N + eps) / (sigma + (0.0 if defect == "eps_once" else eps)) \
        * (p["p_star"] / (sat + eps)) ** p["eta"]                                   # :69-73
    new = torch.clamp((1 - p["rho"]) * alpha + p["rho"] * a_hat, p["alpha_min"], p["alpha_max"])   # :80-81
    new = new.float().to(dtype)                                                     # :82, the float32 state
    z = (alpha if defect == "old_alpha_sat" else new) * (a / (N + eps))             # :87-88
    over = z.abs() > p["tau"]
    new_sat = ((1 - p["rho_sat"]) * sat + p["rho_sat"] * over.to(dtype).mean()).float()   # :91-94
    band = ((z.abs() - p["tau"]).abs() <= BAND * p["tau"]).sum().item()
    return {"alpha": float(new), "sat": float(new_sat), "N": float(N), "sigma": float(sigma), "count": int(over.sum()),
            "band": int(band)}


def modulate(adv, p, alpha, dtype=torch.float64):
    """dynago_transform_advantages(update_ema=False): (mod, N_mb) in `dtype`; numel <= 1: the input."""
    a = adv.detach().to(dtype)
    if a.numel() <= 1:
        return a.clone(), torch.linalg.norm(a) if a.numel() else torch.zeros((), dtype=dtype)
    N = torch.linalg.norm(a)
    z = torch.tensor(float(alpha), dtype=torch.float32).to(dtype) * (a / (N + p["eps"]))
    return a.abs() * (p["kappa"] * torch.tanh(z) + p["v_shift"]), N


def am_loss(values, log_prob, entropy, advantages, old_values, old_log_prob, p, alpha, h, normalize, defect=None):
    """ppo.py:327-388 with use_am_ppo in the dtype of `values`: (loss, ratio, parts) with parts =
    (policy_loss, value_loss, entropy_loss, mod, N_mb)."""
    dtype = values.dtype
    mod, N = modulate(advantages, p, alpha, dtype)
    adv = (mod - mod.mean()) / (mod.std() + 1e-8) if normalize and mod.numel() > 1 else mod          # :349-352
    ratio = torch.exp(log_prob - old_log_prob)
    clip = h["clip_range"]
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    target = (adv if defect == "normalized_target" else mod) + old_values.to(dtype)                  # :369
    value_loss = torch.nn.functional.mse_loss(target, values)
    entropy_loss = -entropy.mean()
    return policy_loss + h["ent_coef"] * entropy_loss + h["vf_coef"] * value_loss, ratio, \
        (policy_loss, value_loss, entropy_loss, mod, N)


def head_autograd(d, h, p, alpha, normalize, dtype=torch.float64, defect=None):
    """The AM head by torch autograd on the CPU in `dtype` over the leaves (mean, values, log_std) of
    ppo_ref.head_data's rows (its `returns` stands for old_values): {d_mean, d_values, d_log_std,
    stats (6, ppo_ref.STATS order), am_stats (4)}."""
    leaf = lambda key: d[key].detach().to(dtype).clone().requires_grad_(True)  # noqa: E731
    c = lambda key: d[key].to(dtype)  # noqa: E731
    mean, values, ls = leaf("mean"), leaf("values"), leaf("log_std")
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * ls.exp())
    lp, ent = dist.log_prob(c("actions")).sum(dim=1), dist.entropy().sum(dim=1)
    loss, ratio, (pl, vl, el, mod, N) = am_loss(values, lp, ent, d["advantages"], c("returns"), c("old_log_prob"), p, alpha,
                                                 h, normalize, defect)
    loss.backward()
    with torch.no_grad():
        log_r = lp - c("old_log_prob")
        stats = torch.stack([pl, vl, el, loss.detach(), ((ratio - 1) - log_r).mean(),
                             ((ratio - 1).abs() > h["clip_range"]).to(dtype).mean()])
        am_stats = torch.stack([c("advantages").mean(), mod.mean(), N, torch.tensor(as_f32(alpha), dtype=dtype)])
    return {"d_mean": mean.grad, "d_values": values.grad, "d_log_std": ls.grad, "stats": stats.detach(),
            "am_stats": am_stats.detach()}


# ---------------------------------------------------------------------------------------------
# ppo.py:399-400 with sgd.py:219-344 (DAG) or :437-498 (AlphaGrad), on a blob and its segment table
def dag_state(n_segments):
    """DAG's state before its first step (sgd.py:159-162, :170-171)."""
    return {"alpha": [1.0] * n_segments, "sat": [0.0] * n_segments, "s_t": 1.0, "rms_t": None, "rms0": None, "step": 0}


def dag_steps(blob, grads, h, c, segments, dtype=torch.float64, fixed_alpha=False, defect=None):
    """clip_grad_norm_(max_grad_norm) + the optimiser's step in `dtype`, one per gradient: a list of
    {"blob", "alpha", "sat" (float32 values per segment), "count", "s_t", "rms_t", "rms0", "step",
    "band" (elements of a sampled step whose |x| lies within BAND of tau), "norm", "coef"}. The
    tensors are the segments' padded slices: pads hold gradient 0, so they add nothing to a norm, to
    sum u^2 or to a count, and the saturation divides by the true count d_s."""
    p = blob.detach().to(dtype).cpu().clone()
    st = dag_state(len(segments))
    d_total = sum(count for _, _, count in segments)
    out = []
    for g in grads:
        g = g.detach().to(dtype).cpu()
        norms = torch.stack([torch.linalg.norm(g[o:o + n]) for o, n, _ in segments])
        total = torch.linalg.norm(norms)                                           # clip_grad_norm_
        coef = torch.clamp(h["max_grad_norm"] / (total + 1e-6), max=1.0)
        g = g * coef
        s_t, k_val = (1.0, 1.0) if fixed_alpha else (st["s_t"], c["k_val"])
        sampled = not fixed_alpha and st["step"] % max(1, int(c["sat_every"])) == 0
        total_sq, band, counts = 0.0, 0, [0] * len(segments)
        for i, (o, n, d_s) in enumerate(segments):
            gs = g[o:o + n]
            norm = torch.linalg.norm(gs)                                           # sgd.py:242
            if fixed_alpha:
                alpha = torch.tensor(c["alpha"], dtype=dtype)
            else:
                sigma = norm * (1.0 / math.sqrt(d_s))                              # :254-256
                sat = torch.tensor(st["sat"][i], dtype=dtype)
                a_hat = c["kappa"] * (norm + c["eps"]) / (sigma + c["eps"]) * (d_s / d_total) ** c["beta"] \
                    * (c["p_star"] / (sat + c["eps"])) ** c["eta"] * s_t           # :265-271
                alpha = torch.clamp((1 - c["rho"]) * torch.tensor(st["alpha"][i], dtype=dtype) + c["rho"] * a_hat,
                                    c["alpha_min"], c["alpha_max"]).float().to(dtype)   # :272-274, a float32 state
                st["alpha"][i] = float(alpha)
            x = (gs * (1.0 / (norm + c["eps"]))) * (alpha / s_t)                   # :277-282
            u = torch.tanh(x) * (k_val * s_t)                                      # :289
            if sampled:                                                            # :292-295
                counts[i] = int((x.abs() > c["tau"]).sum())
                st["sat"][i] = as_f32(counts[i] / (n if defect == "padded_sat" else d_s))
                band += int(((x.abs() - c["tau"]).abs() <= BAND * c["tau"]).sum())
            p[o:o + n] -= h["lr"] * u                                              # :320
            total_sq += float((u * u).sum())                                       # :322-323
        if not fixed_alpha:                                                        # :326-343
            rms_now, beta = math.sqrt(total_sq / d_total), c["ema_beta"]
            st["rms_t"] = rms_now if st["rms_t"] is None else beta * st["rms_t"] + (1 - beta) * rms_now
            if st["step"] < int(c["warmup_steps"]):
                st["rms0"] = st["rms_t"] if st["rms0"] is None else beta * st["rms0"] + (1 - beta) * st["rms_t"]
            else:
                if st["rms0"] is None:
                    st["rms0"] = st["rms_t"]
                den = c["lambda_rms"] * st["rms0"]
                ratio = max(0.0, min(1.0, st["rms_t"] / den)) if den else 1.0
                st["s_t"] = c["s_min"] + (1 - c["s_min"]) * ratio ** c["gamma"]
            st["step"] += 1
        out.append({"blob": p.clone(), "alpha": list(st["alpha"]), "sat": list(st["sat"]), "count": counts,
                    "s_t": st["s_t"], "rms_t": st["rms_t"], "rms0": st["rms0"], "step": st["step"], "band": band,
                    "norm": float(total), "coef": float(coef)})
    return out


def dag_gradients(desc, k, d, pi_w, vf_w, h, scales=(0.5, 3.0, 8.0, 1.5, 5.0, 0.7), seed=0):
    """ppo_ref.adam_gradients' construction, one gradient per scale: random gradients in blob layout
    (pads zero) with norms of `scales` times max_grad_norm."""
    from f16_jsb_amd.policy import pack_blob
    out = []
    for step, scale in enumerate(scales):
        g = pack_blob(desc, *G.tanh_data(k, d, pi_w, vf_w, 1, seed=20 + 10 * seed + step)[0])
        out.append((g * (scale * h["max_grad_norm"] / g.double().norm().item())).float())
    return out


def segment_views(segments, flat, names=None):
    """A flat blob-layout tensor cut into its segments, in policy_grad_ref.named_tensors' nesting
    shape for rule_of_four: a list of (name, slice)."""
    return [("seg%d" % i if names is None else names[i], flat[o:o + n]) for i, (o, n, _) in enumerate(segments)]


def rule(got, ref64, torch32):
    """The project's rule on plain tensors or scalars: (err of got, 4 max(err of torch32, 2^-24 max|ref|))."""
    t = lambda x: torch.as_tensor(x, dtype=torch.float64).reshape(-1)  # noqa: E731
    got, ref64, torch32 = t(got), t(ref64), t(torch32)
    err = (got - ref64).abs().max().item()
    return err, 4.0 * max((torch32 - ref64).abs().max().item(), 2.0 ** -24 * ref64.abs().max().item())


def check(label, got, ref64, torch32, bad):
    err, allow = rule(got, ref64, torch32)
    print("%s: kernel %.3e allowed %.3e ratio of torch's %.2f" % (label, err, allow, 4.0 * err / allow if allow else 0.0))
    if not err <= allow:
        bad.append((label, err, allow))
