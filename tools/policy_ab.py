#!/usr/bin/env python3
"""Same-box A/B of the policy in the rollout loop: torch (HIP-graphed) vs the device policy kernel.

    python tools/policy_ab.py [--envs 32768] [--stack 4] [--rounds 5] [--steps 256]
                              [--out profiles/policy_forward_ab.json]

A = bench.GraphedPolicy(bench.MlpActorCritic): SB3's MlpPolicy shape in torch, forward and value
    each captured once as a HIP graph on a static input (bench.py's policy-in-the-loop leg);
B = DevicePolicy.from_layers on the SAME weights: one f16env_policy_forward launch.
Two nets: pi=[64,64] vf=[64,64] (SB3's default) and pi=[64,64] vf=[128,64] (the reference's
train.py heads). Per net, in one process, interleaved A B A B ... for --rounds rounds:
  forward  -- the forward alone on the windowed observation, by graph replay of its launches
              (A: the copy into the static input + its graph; B: its launch captured in a graph),
              device events around `--reps` replays;
  rollout  -- collect_rollout over --steps steps (windowed layout, fused rollout-step launches,
              deferred bootstrap), host clock around it ending in a device synchronise.
Every round's numbers are kept; `b_faster_every_round` says whether B beat A in each of them.
Needs a GPU (no fallback).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def graph_of(fn, dev):
    import torch
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def time_replays(fn, reps):
    import torch
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


class WideVf:
    """bench.MlpActorCritic with another vf branch (same init rule)."""

    def __new__(cls, bench, obs_dim, dev, vf_widths, seed):
        import torch
        net = bench.MlpActorCritic(obs_dim, dev, seed=seed)
        g = torch.Generator(device="cpu").manual_seed(seed + 1)
        layers, fan_in = [], obs_dim
        for w in vf_widths:
            layers.append(((torch.randn(w, fan_in, generator=g) * (2 ** 0.5 / fan_in ** 0.5)).to(dev),
                           torch.zeros(w, device=dev)))
            fan_in = w
        net.vf = layers
        net.val_w = ((torch.randn(1, fan_in, generator=g) / fan_in ** 0.5).to(dev), torch.zeros(1, device=dev))
        return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--stack", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_forward_ab.json"))
    args = ap.parse_args()

    import torch
    import bench
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.policy import DevicePolicy
    from f16_jsb_amd.rollout import DeviceRolloutBuffer, collect_rollout
    if not torch.cuda.is_available():
        raise SystemExit("policy_ab needs a GPU")
    dev = torch.device("cuda", 0)
    n, k, T = args.envs, args.stack, args.steps
    envs = F16Envs(n, stack_k=k, device=dev, seed=7, obs_layout="window")
    envs.reset()
    for t in range(20):
        envs.step(envs.sample_actions(3, t))
    buf = DeviceRolloutBuffer(T, n, k, dev)
    result = {"envs": n, "stack_k": k, "rollout_steps": T, "rounds": args.rounds, "forward_reps": args.reps,
              "device": torch.cuda.get_device_name(0), "nets": []}
    for name, vf_widths in (("pi64x64_vf64x64", None), ("pi64x64_vf128x64", [128, 64])):
        net = bench.MlpActorCritic(k * 15, dev, seed=0) if vf_widths is None else WideVf(bench, k * 15, dev, vf_widths, 0)
        A = bench.GraphedPolicy(net, n, k, dev)
        B = DevicePolicy.from_layers(net.pi, net.vf, net.act_w, net.val_w, net.log_std, stack_k=k, seed=1)
        obs = envs.obs
        # the same function: values agree to float32 rounding (the noise differs by design)
        va, vb = A.value(obs).clone(), B.value(obs)
        value_diff = float((va - vb).abs().max())
        outs = (torch.empty((n, 4), device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev))
        gB = graph_of(lambda: B.forward_into(obs, 0, *outs), dev)
        fwd_a, fwd_b = (lambda: A(obs)), gB.replay
        for pol in (A, B):  # warm both rollouts (the stash, the views)
            collect_rollout(envs, DeviceRolloutBuffer(8, n, k, dev), 11, 0, policy_fn=pol,
                            value_fn=pol.value, persistent=False)
        rounds = []
        for r in range(args.rounds):
            row = {}
            for tag, fwd, pol in (("a", fwd_a, A), ("b", fwd_b, B)):
                row["forward_ms_" + tag] = time_replays(fwd, args.reps)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                collect_rollout(envs, buf, 11 + r, 1000 * r, policy_fn=pol, value_fn=pol.value, persistent=False)
                torch.cuda.synchronize()
                row["rollout_step_ms_" + tag] = (time.perf_counter() - t0) / T * 1e3
            rounds.append(row)
        med = {key: statistics.median(x[key] for x in rounds) for key in rounds[0]}
        result["nets"].append({
            "net": name, "value_max_abs_diff_a_vs_b": value_diff, "rounds": rounds, "median": med,
            "forward_speedup_median": med["forward_ms_a"] / med["forward_ms_b"],
            "rollout_step_speedup_median": med["rollout_step_ms_a"] / med["rollout_step_ms_b"],
            "env_steps_per_s_a": n / med["rollout_step_ms_a"] * 1e3,
            "env_steps_per_s_b": n / med["rollout_step_ms_b"] * 1e3,
            "b_faster_every_round": all(x["forward_ms_b"] < x["forward_ms_a"]
                                        and x["rollout_step_ms_b"] < x["rollout_step_ms_a"] for x in rounds)})
    envs.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "nets": [{key: x[key] for key in ("net", "forward_speedup_median",
                                                                         "rollout_step_speedup_median",
                                                                         "b_faster_every_round", "median")}
                                               for x in result["nets"]]}))


if __name__ == "__main__":
    main()
