#!/usr/bin/env python3
"""Same-box A/B/C of one PPO minibatch update on the blob: torch's loss and optimiser vs DevicePPO.

    python tools/ppo_update_ab.py [--rounds 5] [--reps 20] [--out profiles/ppo_update_ab.json]

One update = the forward on the minibatch, the PPO loss (tests/policy_grad_ref.py: ppo_loss, clip
0.2, ent_coef 0.01, vf_coef 0.5), its gradient, clip_grad_norm_(0.5) and an Adam step (lr 3e-4,
eps 1e-5), on a fixed synthetic minibatch.
A = DevicePolicy.evaluate_actions + the loss in torch + loss.backward() (f16env_policy_backward
    under autograd) + clip_grad_norm_ + torch.optim.Adam([pol.blob]): the update as it was before
    DevicePPO (B of tools/policy_backward_ab.py);
B = DevicePPO.update, eager: forward, loss head, backward, clip + Adam as HIP launches;
C = the same update captured in a HIP graph once and replayed.
Architectures: cases E and D of tests/policy_ref.py's MATRIX; batch sizes 256, 4 096 and 65 536.
Per (case, batch), in one process, interleaved A B C A B C ... for --rounds rounds: host clock
around --reps updates ending in a device synchronise. Needs a GPU (no fallback).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--cases", nargs="+", default=["E", "D"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update_ab.json"))
    args = ap.parse_args()

    import torch
    import policy_grad_ref as G
    import policy_ref
    from f16_jsb_amd.policy import DevicePolicy
    from f16_jsb_amd.ppo import DevicePPO
    if not torch.cuda.is_available():
        raise SystemExit("ppo_update_ab needs a GPU")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "runs": []}

    def timed(update):
        for _ in range(3):
            update()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            update()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e3

    for case in args.cases:
        k, d, pi_w, vf_w, _ = policy_ref.MATRIX[case]
        net = G.tanh_data(k, d, pi_w, vf_w, 1)[0]
        for batch in args.batches:
            g = torch.Generator(device="cpu").manual_seed(batch)
            rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
            obs, actions, adv, ret, old_v = rnd(batch, k, d), rnd(batch, 4), rnd(batch), rnd(batch), rnd(batch)
            new = lambda: DevicePolicy.from_layers(*G.as_params(net, torch.float32, dev), stack_k=k, frame_dim=d)  # noqa: E731
            pol_a, pol_b, pol_c = new().requires_grad_(), new(), new()
            with torch.no_grad():
                old_lp = pol_b.evaluate_actions(obs, actions)[1].clone()
            opt_a = torch.optim.Adam(pol_a.parameters(), lr=3e-4, eps=1e-5)
            ppo_b = DevicePPO(pol_b, ent_coef=0.01, max_batch=batch)
            ppo_c = DevicePPO(pol_c, ent_coef=0.01, max_batch=batch)
            mb = (obs, actions, old_v, old_lp, adv, ret)

            def update_a():
                v, lp, ent = pol_a.evaluate_actions(obs, actions)
                loss = G.ppo_loss(v, lp, ent, adv, ret, old_lp)[0]
                opt_a.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(pol_a.parameters(), 0.5)
                opt_a.step()

            def update_b():
                ppo_b.update(*mb)

            # one eager update ahead of the capture (every kernel has run), mirrored on A and B so
            # that the three paths have taken the same number of steps when they are compared
            update_a(), update_b(), ppo_c.update(*mb)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                ppo_c.update(*mb)
            graph.replay()  # (the capture ran nothing: one replay keeps C level with A and B below)
            update_a(), update_b()

            rounds = [{"update_ms_a": timed(update_a), "update_ms_b": timed(update_b), "update_ms_c": timed(graph.replay)}
                      for _ in range(args.rounds)]
            torch.cuda.synchronize()
            med = {key: statistics.median(x[key] for x in rounds) for key in rounds[0]}
            spread = {key: [min(x[key] for x in rounds), max(x[key] for x in rounds)] for key in rounds[0]}
            result["runs"].append({
                "case": case, "batch": batch, "rounds": rounds, "median": med, "min_max": spread,
                "speedup_b_over_a_median": med["update_ms_a"] / med["update_ms_b"],
                "speedup_c_over_a_median": med["update_ms_a"] / med["update_ms_c"],
                "b_faster_than_a_every_round": all(x["update_ms_b"] < x["update_ms_a"] for x in rounds),
                "c_no_slower_than_b_every_round": all(x["update_ms_c"] <= x["update_ms_b"] for x in rounds),
                "c_no_slower_than_b_median": med["update_ms_c"] <= med["update_ms_b"],
                # the three paths took the same steps from the same start: B and C agree bit for bit,
                # A (torch's loss arithmetic) to rounding amplified by Adam's normalised step
                "blob_bits_equal_b_vs_c": bool(torch.equal(pol_b.blob, pol_c.blob)),
                "blob_max_abs_diff_a_vs_b": float((pol_a.blob.detach() - pol_b.blob).abs().max()),
                "steps": int(ppo_b.step.item())})
            print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
