#!/usr/bin/env python3
"""Same-box A/B of the reference's LMA policy in the rollout loop: torch (HIP-graphed) vs the
device LMA policy kernel, in the protocol of tools/policy_ab.py.

    python tools/lma_ab.py [--envs 32768] [--small 256] [--rounds 5] [--steps 256]
                           [--out profiles/lma_forward_ab.json]

The net is case R of tests/lma_ref.py: K = 10 raw frames, the extractor with 2 blocks and ff 128,
pi = [64, 64], vf = [128, 64], tanh, random weights.
A = bench.GraphedPolicy(TorchLMA): the same network in torch, eval mode, float32 on the GPU (the
    15 -> 17 transform, nn.functional.linear / layer_norm / scaled_dot_product_attention / gelu),
    forward and value each captured once as a HIP graph on a static input;
B = DeviceLMAPolicy.from_layers on the SAME weights: one f16env_policy_lma_forward launch.
Per row, in one process, interleaved A B A B ... for --rounds rounds:
  forward  -- the forward alone on the windowed observation at --small and --envs rows, by graph
              replay (A: the copy into the static input + its graph; B: its launch captured in a
              graph), device events around --reps replays;
  rollout  -- collect_rollout over --steps steps at --envs envs (windowed layout, fused
              rollout-step launches, deferred bootstrap), host clock ending in a device synchronise.
Every round is kept; `b_faster_every_round` says whether B beat A in each of them. From the same
run, the MLP-only DevicePolicy rows ("mlp_only": the same pi / vf MLPs without the extractor --
the forward on the (n, K, 17) feature window, DESIGN's case D; the rollout on the raw frames,
which is what collect_rollout hands a policy), so the extractor's cost per step can be read off.
Needs a GPU (no fallback).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

K, EMBED, D_NEW, HEADS, FF, BLOCKS = 10, 64, 32, 4, 128, 2
PI, VF = [64, 64], [128, 64]


class TorchLMA:
    """The reference's policy network in torch, eval mode: __call__(obs) -> (actions, values,
    log_probs), value(obs) -> values, as bench.MlpActorCritic."""

    def __init__(self, dev, seed=0):
        import torch
        from f16_jsb_amd.abi import lma_new_dims
        from f16_jsb_amd.lma_policy import positional_encoding
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.L, self.C = lma_new_dims(K, EMBED)

        def lin(o, i):
            return (torch.randn(o, i, generator=g) * math.sqrt(2.0 / i)).to(dev), (0.1 * torch.randn(o, generator=g)).to(dev)

        def ln():
            return (1.0 + 0.1 * torch.randn(D_NEW, generator=g)).to(dev), (0.1 * torch.randn(D_NEW, generator=g)).to(dev)

        def branch(widths):
            out, fan_in = [], self.L * D_NEW
            for w in widths:
                out.append(lin(w, fan_in))
                fan_in = w
            return out
        self.ext = {"embed": lin(EMBED, 17), "embed2": lin(D_NEW, self.C), "blocks": [
            {"ln_1": ln(), "attn.c_attn": lin(3 * D_NEW, D_NEW), "attn.c_proj": lin(D_NEW, D_NEW), "ln_2": ln(),
             "mlp.c_fc": lin(FF, D_NEW), "mlp.c_proj": lin(D_NEW, FF)} for _ in range(BLOCKS)]}
        self.pi, self.vf = branch(PI), branch(VF)
        self.act_w, self.val_w = lin(4, PI[-1]), lin(1, VF[-1])
        self.log_std = torch.zeros(4, device=dev)
        self.pe = positional_encoding(K, EMBED).to(dev)

    def features(self, o):
        import torch
        import torch.nn.functional as F
        n = o.shape[0]
        dx, dy, dz = o[..., 12] - o[..., 0], o[..., 13] - o[..., 1], o[..., 14] - o[..., 2]
        rel = torch.atan2(dy, dx) - o[..., 11]
        x = torch.stack([1.0 / (1.0 + torch.sqrt(dx * dx + dy * dy) * 1e-3), dz / 15000.0, o[..., 2] / 15000.0, o[..., 3],
                         o[..., 6], o[..., 7], o[..., 8], torch.cos(o[..., 4]), torch.cos(o[..., 5]), torch.sin(o[..., 4]),
                         torch.sin(o[..., 5]), torch.cos(o[..., 9]), torch.cos(o[..., 10]), torch.sin(o[..., 9]),
                         torch.sin(o[..., 10]), torch.cos(rel), torch.sin(rel)], -1)
        y = torch.relu(F.linear(x, *self.ext["embed"])) + self.pe
        z = torch.cat(torch.split(y, EMBED // 4, dim=2), dim=1).reshape(n, self.L, self.C)
        z = torch.relu(F.linear(z, *self.ext["embed2"]))
        for b in self.ext["blocks"]:
            h = F.layer_norm(z, (D_NEW,), *b["ln_1"], 1e-5)
            q, k, v = (a.view(n, self.L, HEADS, D_NEW // HEADS).transpose(1, 2)
                       for a in F.linear(h, *b["attn.c_attn"]).split(D_NEW, dim=2))
            a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(n, self.L, D_NEW)
            z = z + F.linear(a, *b["attn.c_proj"])
            h = F.layer_norm(z, (D_NEW,), *b["ln_2"], 1e-5)
            z = z + F.linear(F.gelu(F.linear(h, *b["mlp.c_fc"])), *b["mlp.c_proj"])
        return z.reshape(n, -1)

    @staticmethod
    def _mlp(x, layers):
        import torch
        for w, b in layers:
            x = torch.tanh(torch.nn.functional.linear(x, w, b))
        return x

    def value(self, obs):
        import torch
        return torch.nn.functional.linear(self._mlp(self.features(obs), self.vf), *self.val_w).reshape(-1)

    def __call__(self, obs):
        import torch
        f = self.features(obs)
        mean = torch.nn.functional.linear(self._mlp(f, self.pi), *self.act_w)
        eps = torch.randn_like(mean)
        act = mean + self.log_std.exp() * eps
        logp = (-0.5 * eps * eps - self.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
        return act, torch.nn.functional.linear(self._mlp(f, self.vf), *self.val_w).reshape(-1), logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--small", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lma_forward_ab.json"))
    args = ap.parse_args()

    import torch
    import bench
    from policy_ab import graph_of, time_replays
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.features import features
    from f16_jsb_amd.lma_policy import DeviceLMAPolicy
    from f16_jsb_amd.policy import DevicePolicy
    from f16_jsb_amd.rollout import DeviceRolloutBuffer, collect_rollout
    if not torch.cuda.is_available():
        raise SystemExit("lma_ab needs a GPU")
    dev = torch.device("cuda", 0)
    n, T = args.envs, args.steps
    envs = F16Envs(n, stack_k=K, device=dev, seed=7, obs_layout="window")
    envs.reset()
    for t in range(20):
        envs.step(envs.sample_actions(3, t))
    net = TorchLMA(dev, seed=0)
    B = DeviceLMAPolicy.from_layers(net.ext, net.pi, net.vf, net.act_w, net.val_w, net.log_std, stack_k=K, seed=1)
    g = torch.Generator(device="cpu").manual_seed(5)

    def mlp_only(d):  # the same widths without the extractor
        def lin(o, i):
            return (torch.randn(o, i, generator=g) * math.sqrt(2.0 / i)).to(dev), torch.zeros(o, device=dev)
        return DevicePolicy.from_layers([lin(64, K * d), lin(64, 64)], [lin(128, K * d), lin(64, 128)], lin(4, 64),
                                        lin(1, 64), torch.zeros(4, device=dev), stack_k=K, frame_dim=d, seed=1)
    M17, M15 = mlp_only(17), mlp_only(15)
    result = {"net": "case R: K 10, D 15, 2 blocks, ff 128, pi [64, 64], vf [128, 64], tanh", "rollout_steps": T,
              "rounds": args.rounds, "forward_reps": args.reps, "device": torch.cuda.get_device_name(0), "rows": []}
    obs_all = envs.obs
    result["value_max_abs_diff_a_vs_b"] = float((net.value(obs_all[:4096]) - B.value(obs_all[:4096])).abs().max())

    def forward_row(rows):
        obs = obs_all[:rows]
        feat = features(obs)
        A = bench.GraphedPolicy(net, rows, K, dev)
        outs = (torch.empty((rows, 4), device=dev), torch.empty(rows, device=dev), torch.empty(rows, device=dev))
        gB = graph_of(lambda: B.forward_into(obs, 0, *outs), dev)
        gM = graph_of(lambda: M17.forward_into(feat, 0, *outs), dev)
        rounds = []
        for _ in range(args.rounds):
            rounds.append({"ms_a": time_replays(lambda: A(obs), args.reps), "ms_b": time_replays(gB.replay, args.reps),
                           "ms_mlp_only": time_replays(gM.replay, args.reps)})
        return rounds

    def rollout_row():
        A = bench.GraphedPolicy(net, n, K, dev)
        buf = DeviceRolloutBuffer(T, n, K, dev)
        for pol in (A, B, M15):  # warm (the stash, the views)
            collect_rollout(envs, DeviceRolloutBuffer(8, n, K, dev), 11, 0, policy_fn=pol, value_fn=pol.value, persistent=False)
        rounds = []
        for r in range(args.rounds):
            row = {}
            for tag, pol in (("a", A), ("b", B), ("mlp_only", M15)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                collect_rollout(envs, buf, 11 + r, 1000 * r, policy_fn=pol, value_fn=pol.value, persistent=False)
                torch.cuda.synchronize()
                row["ms_" + tag] = (time.perf_counter() - t0) / T * 1e3
            rounds.append(row)
        return rounds

    for what, rows, rounds in (("forward", args.small, None), ("forward", n, None), ("rollout_step", n, None)):
        rounds = forward_row(rows) if what == "forward" else rollout_row()
        med = {key: statistics.median(x[key] for x in rounds) for key in rounds[0]}
        result["rows"].append({"what": what, "rows": rows, "rounds": rounds, "median": med,
                               "speedup_median": med["ms_a"] / med["ms_b"],
                               "extractor_cost_ms_median": med["ms_b"] - med["ms_mlp_only"],
                               "b_faster_every_round": all(x["ms_b"] < x["ms_a"] for x in rounds)})
    result["b_faster_every_round_of_every_row"] = all(x["b_faster_every_round"] for x in result["rows"])
    envs.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "b_faster": result["b_faster_every_round_of_every_row"],
                      "rows": [{key: x[key] for key in ("what", "rows", "median", "speedup_median")} for x in result["rows"]]}))


if __name__ == "__main__":
    main()
