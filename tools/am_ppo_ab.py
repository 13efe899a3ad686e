#!/usr/bin/env python3
"""Same-box A/B of device AM-PPO against the same arithmetic in torch.

    python tools/am_ppo_ab.py [--rounds 5] [--reps 20] [--out profiles/am_ppo_ab.json]

1. The DynAGO controller over a finished rollout's advantages (f16env_ppo_dynago_update), at
   --controller-sizes T x N (default 2048x4096 and 2048x32768):
   A = ppo.py:54-94 as torch ops on the device tensor, the state in a device tensor, no .item();
   B = DevicePPO.dynago_update (three launches, the array read twice).
   Reported: the median time and the fraction of the 8 TB/s HBM peak at 8 B per element.
2. One AM-PPO + DAG minibatch update, cases E and D of tests/policy_ref.py's MATRIX at --batches rows:
   A = pol.evaluate_actions + ppo.py:327-388's AM loss in torch + loss.backward() + clip_grad_norm_ +
       sgd.py:236-343's DAG.step in torch over views of the blob's parameter tensors, with the
       reference's .item() calls kept (ppo.py:329, :340, :362-386, sgd.py:323);
   B = DevicePPO(am_ppo={}, optimizer="dag").update;
   C = DevicePPO().update (standard PPO, Adam) -- B - C is what the feature costs per minibatch.
   Beside them the optimiser's step alone (step_from) for DAG and for Adam.
The method is tools/ppo_update_ab.py's: one process, interleaved rounds, host clock around --reps
repetitions ending in a device synchronise. Needs a GPU (no fallback).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12
COPY_RATE = 6.29e12  # the measured float4 copy rate of an MI355X


def parse_size(text):
    t, n = text.lower().split("x")
    return int(t), int(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--controller-sizes", type=parse_size, nargs="*", default=[(2048, 4096), (2048, 32768)])
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--cases", nargs="*", default=["E", "D"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "am_ppo_ab.json"))
    args = ap.parse_args()

    import torch
    import am_ppo_ref as A
    import policy_grad_ref as G
    import policy_ref
    import ppo_ref as P
    from f16_jsb_amd import abi
    from f16_jsb_amd.policy import DevicePolicy
    from f16_jsb_amd.ppo import DevicePPO
    if not torch.cuda.is_available():
        raise SystemExit("am_ppo_ab needs a GPU")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "controller": [],
              "update": []}
    p, h, c = A.dynago(), P.hyper(ent_coef=0.01), A.dag_constants()

    def timed(f):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e3

    def summary(rounds):
        med = {key: statistics.median(x[key] for x in rounds) for key in rounds[0]}
        return med, {key: [min(x[key] for x in rounds), max(x[key] for x in rounds)] for key in rounds[0]}

    def modulate(a, state):
        """ppo.py:54-99 with update_ema = False on the device in float32 (the reference forms sigma
        and alpha_hat in this mode too, :60-76, and drops them); state = device tensor (alpha, sat)."""
        eps = p["eps"]
        N = torch.linalg.norm(a)
        sigma = torch.std(a) + eps
        p["kappa_controller"] * (N + eps) / (sigma + eps) * (p["p_star"] / (state[1] + eps)) ** p["eta"]
        z = state[0] * (a / (N + eps))
        return a.abs() * (p["kappa"] * torch.tanh(z) + p["v_shift"])

    # ---- 1. the controller
    k, d, pi_w, vf_w, _ = policy_ref.MATRIX["E"]
    net = G.tanh_data(k, d, pi_w, vf_w, 1)[0]
    new_pol = lambda: DevicePolicy.from_layers(*G.as_params(net, torch.float32, dev), stack_k=k, frame_dim=d)  # noqa: E731
    for t_steps, n_envs in args.controller_sizes:
        n = t_steps * n_envs
        adv = torch.randn(t_steps, n_envs, generator=torch.Generator(device=dev).manual_seed(n), device=dev)
        ppo = DevicePPO(new_pol(), max_batch=1, am_ppo={}).reserve(1, rollout=n)
        state_a = ppo.am_state.clone()
        flat = adv.reshape(-1)

        def update_a():
            eps = p["eps"]  # (ppo.py:54-94; the modulated advantages the reference also forms there and drops are left out)
            N = torch.linalg.norm(flat)
            sigma = torch.std(flat) + eps
            a_hat = p["kappa_controller"] * (N + eps) / (sigma + eps) * (p["p_star"] / (state_a[1] + eps)) ** p["eta"]
            alpha = torch.clamp((1 - p["rho"]) * state_a[0] + p["rho"] * a_hat, p["alpha_min"], p["alpha_max"])
            z = alpha * (flat / (N + eps))
            state_a[1] = (1 - p["rho_sat"]) * state_a[1] + p["rho_sat"] * (z.abs() > p["tau"]).float().mean()
            state_a[0] = alpha

        def update_b():
            ppo.dynago_update(adv)

        rounds = [{"controller_ms_a": timed(update_a), "controller_ms_b": timed(update_b)} for _ in range(args.rounds)]
        med, spread = summary(rounds)
        rate = 8.0 * n / (med["controller_ms_b"] * 1e-3)
        result["controller"].append({
            "n_steps": t_steps, "n_envs": n_envs, "elements": n, "rounds": rounds, "median": med, "min_max": spread,
            "speedup_b_over_a_median": med["controller_ms_a"] / med["controller_ms_b"],
            "b_faster_than_a_every_round": all(x["controller_ms_b"] < x["controller_ms_a"] for x in rounds),
            "b_bytes_per_s_at_8_per_element": rate, "b_fraction_of_hbm_peak": rate / HBM_PEAK,
            "b_fraction_of_copy_rate": rate / COPY_RATE,
            "state_a": state_a.tolist(), "state_b": ppo.am_state.tolist()})
        print(json.dumps(result["controller"][-1]), flush=True)
        del adv, flat, ppo

    # ---- 2. the minibatch update
    def blob_views(desc, blob):
        """The parameter tensors as views of a blob-layout tensor (policy.unpack_blob without the
        copies): a weight as (tiles, rows of the tile, fan_in), its pads cut off."""
        off, _ = abi.policy_blob_layout(desc)
        out = []

        def piece(slot, rows, outs, fan_in):
            nks = (fan_in + 1) // 2
            w = blob[off[slot]:off[slot] + (rows // 32) * nks * 64].view(rows // 32, nks, 2, 32)
            w = w.permute(0, 3, 1, 2).flatten(2)[:, :min(outs, 32), :fan_in]
            assert w.untyped_storage().data_ptr() == blob.untyped_storage().data_ptr() and w.numel() == outs * fan_in
            out.append(w)
            out.append(blob[off[slot + 1]:off[slot + 1] + outs])
        for b, (widths, n) in enumerate(((desc.pi_width, desc.n_pi), (desc.vf_width, desc.n_vf))):
            fan_in = desc.K * desc.D
            for l in range(n):
                piece(6 * b + 2 * l, widths[l], widths[l], fan_in)
                fan_in = widths[l]
        piece(abi.F16_POLICY_OFF_ACT_W, 32, 4, desc.pi_width[desc.n_pi - 1])
        piece(abi.F16_POLICY_OFF_VAL_W, 32, 1, desc.vf_width[desc.n_vf - 1])
        ls = off[abi.F16_POLICY_OFF_LOG_STD]
        return out + [blob[ls:ls + 4]]

    for case in args.cases:
        k, d, pi_w, vf_w, _ = policy_ref.MATRIX[case]
        net = G.tanh_data(k, d, pi_w, vf_w, 1)[0]
        new_pol = lambda: DevicePolicy.from_layers(*G.as_params(net, torch.float32, dev), stack_k=k, frame_dim=d)  # noqa: E731
        for batch in args.batches:
            g = torch.Generator(device="cpu").manual_seed(batch)
            rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
            obs, actions, adv, ret, old_v = rnd(batch, k, d), rnd(batch, 4), rnd(batch), rnd(batch), rnd(batch)
            pol_a, pol_b, pol_c = new_pol().requires_grad_(), new_pol(), new_pol()
            with torch.no_grad():
                old_lp = pol_b.evaluate_actions(obs, actions)[1].clone()
            ppo_b = DevicePPO(pol_b, ent_coef=0.01, max_batch=batch, am_ppo={}, optimizer="dag")
            ppo_c = DevicePPO(pol_c, ent_coef=0.01, max_batch=batch)
            mb = (obs, actions, old_v, old_lp, adv, ret)
            state_a = ppo_b.am_state.clone()
            params = blob_views(pol_a.desc, pol_a.blob)
            counts = [t.numel() for t in params]
            d_total, dL = sum(counts), torch.tensor([float(x) for x in counts], device=dev)
            inv_sqrt_d = [1.0 / math.sqrt(x) for x in counts]
            dag = {"alpha": torch.ones(len(params), device=dev), "sat": torch.zeros(len(params), device=dev), "s_t": 1.0,
                   "rms_t": None, "rms0": None, "step": 0}

            def dag_step(grads):
                """sgd.py:236-343 as PPO._setup_model builds it, in torch on the device."""
                norms = torch._foreach_norm(grads, 2)
                sigma_cat = torch.stack(torch._foreach_mul(norms, inv_sqrt_d))
                norm_cat = torch.stack(norms)
                a_hat = c["kappa"] * (norm_cat + c["eps"]) / (sigma_cat + c["eps"]) * (dL / d_total) ** c["beta"] \
                    * (c["p_star"] / (dag["sat"] + c["eps"])) ** c["eta"] * dag["s_t"]
                alpha = ((1 - c["rho"]) * dag["alpha"] + c["rho"] * a_hat).clamp_(c["alpha_min"], c["alpha_max"])
                dag["alpha"] = alpha
                g_norm = torch._foreach_mul(grads, torch._foreach_reciprocal(torch._foreach_add(norms, c["eps"])))
                scaled = torch._foreach_mul(g_norm, torch._foreach_div(list(alpha.unbind()), dag["s_t"]))
                updates = torch._foreach_mul(torch._foreach_tanh(scaled), c["k_val"] * dag["s_t"])
                if dag["step"] % int(c["sat_every"]) == 0:
                    dag["sat"] = torch.stack([t.abs().gt(c["tau"]).float().mean() for t in scaled])
                torch._foreach_add_(params, updates, alpha=-h["lr"])
                total_sq = sum(t.sum() for t in torch._foreach_mul(updates, updates)).item()
                rms_now, beta = math.sqrt(total_sq / d_total), c["ema_beta"]
                dag["rms_t"] = rms_now if dag["rms_t"] is None else beta * dag["rms_t"] + (1 - beta) * rms_now
                if dag["step"] < int(c["warmup_steps"]):
                    dag["rms0"] = dag["rms_t"] if dag["rms0"] is None else beta * dag["rms0"] + (1 - beta) * dag["rms_t"]
                else:
                    dag["rms0"] = dag["rms_t"] if dag["rms0"] is None else dag["rms0"]
                    ratio = max(0.0, min(1.0, dag["rms_t"] / (c["lambda_rms"] * dag["rms0"])))
                    dag["s_t"] = c["s_min"] + (1 - c["s_min"]) * ratio ** c["gamma"]
                dag["step"] += 1

            def update_a():
                v, lp, ent = pol_a.evaluate_actions(obs, actions)
                adv.mean().item()                                                      # ppo.py:329
                mod = modulate(adv, state_a)
                mod.mean().item()                                                      # :340
                a_pol = (mod - mod.mean()) / (mod.std() + 1e-8)
                ratio = torch.exp(lp - old_lp)
                clip = h["clip_range"]
                policy_loss = -torch.min(a_pol * ratio, a_pol * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
                policy_loss.item()                                                     # :362
                torch.mean((torch.abs(ratio - 1) > clip).float()).item()               # :364
                value_loss = torch.nn.functional.mse_loss(mod + old_v, v)
                value_loss.item()                                                      # :382
                entropy_loss = -torch.mean(ent)
                entropy_loss.item()                                                    # :386
                loss = policy_loss + h["ent_coef"] * entropy_loss + h["vf_coef"] * value_loss
                with torch.no_grad():
                    log_ratio = lp - old_lp
                    torch.mean((torch.exp(log_ratio) - 1) - log_ratio).cpu().numpy()   # :392
                pol_a.blob.grad = None
                loss.backward()
                torch.nn.utils.clip_grad_norm_(pol_a.parameters(), h["max_grad_norm"])
                with torch.no_grad():
                    dag_step(blob_views(pol_a.desc, pol_a.blob.grad))

            def update_b():
                ppo_b.update(*mb)

            def update_c():
                ppo_c.update(*mb)

            update_a(), update_b(), update_c()
            grad_b, grad_c = ppo_b.grad.clone(), ppo_c.grad.clone()
            rounds = [{"update_ms_a": timed(update_a), "update_ms_b": timed(update_b), "update_ms_c": timed(update_c),
                       "step_ms_dag": timed(lambda: ppo_b.step_from(grad_b)),
                       "step_ms_adam": timed(lambda: ppo_c.step_from(grad_c))} for _ in range(args.rounds)]
            torch.cuda.synchronize()
            med, spread = summary(rounds)
            result["update"].append({
                "case": case, "batch": batch, "rounds": rounds, "median": med, "min_max": spread,
                "speedup_b_over_a_median": med["update_ms_a"] / med["update_ms_b"],
                "b_faster_than_a_every_round": all(x["update_ms_b"] < x["update_ms_a"] for x in rounds),
                "feature_cost_ms_b_minus_c_median": med["update_ms_b"] - med["update_ms_c"],
                "dag_step_over_adam_step_median": med["step_ms_dag"] / med["step_ms_adam"],
                "blob_finite": bool(torch.isfinite(pol_a.blob).all() and torch.isfinite(pol_b.blob).all())})
            print(json.dumps(result["update"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
