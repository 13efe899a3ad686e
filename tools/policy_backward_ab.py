#!/usr/bin/env python3
"""Same-box A/B of one PPO minibatch update: a torch copy of the net vs the blob path.

    python tools/policy_backward_ab.py [--rounds 5] [--reps 20] [--out profiles/policy_backward_ab.json]

One update = evaluate_actions, the PPO loss (tests/policy_grad_ref.py: ppo_loss), backward,
clip_grad_norm_(0.5) and an Adam step (lr 3e-4, eps 1e-5), on a fixed synthetic minibatch.
A = the net as torch leaves under SB3's key names, torch autograd, Adam over those leaves, then
    pol.load_state_dict(...) -- the repack a caller without the backward kernel does per update;
B = DevicePolicy.evaluate_actions on the blob, f16env_policy_backward, Adam over [pol.blob].
Architectures: cases E and D of tests/policy_ref.py's MATRIX; batch sizes 256, 4 096 and 65 536.
Per (case, batch), in one process, interleaved A B A B ... for --rounds rounds: host clock around
--reps updates ending in a device synchronise. The backward kernel alone (both launches) is timed
by device events around --reps calls. Needs a GPU (no fallback).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_backward_ab.json"))
    args = ap.parse_args()

    import torch
    import policy_grad_ref as G
    import policy_ref
    from f16_jsb_amd.policy import DevicePolicy, layers_from_state_dict, state_dict_from_layers
    if not torch.cuda.is_available():
        raise SystemExit("policy_backward_ab needs a GPU")
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
            obs, actions, adv, ret = rnd(batch, k, d), rnd(batch, 4), rnd(batch), rnd(batch)
            pol_a = DevicePolicy.from_layers(*G.as_params(net, torch.float32, dev), stack_k=k, frame_dim=d)
            pol_b = DevicePolicy.from_layers(*G.as_params(net, torch.float32, dev), stack_k=k, frame_dim=d).requires_grad_()
            with torch.no_grad():
                old_lp = pol_b.evaluate_actions(obs, actions)[1].clone()
            sd = state_dict_from_layers(*G.as_params(net, torch.float32, dev))  # A's copy of the net: leaves
            opt_a = torch.optim.Adam(list(sd.values()), lr=3e-4, eps=1e-5)
            opt_b = torch.optim.Adam(pol_b.parameters(), lr=3e-4, eps=1e-5)

            def update_a():
                v, lp, ent = G.evaluate_actions(obs, actions, *layers_from_state_dict(sd), "tanh")
                loss = G.ppo_loss(v, lp, ent, adv, ret, old_lp)[0]
                opt_a.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(list(sd.values()), 0.5)
                opt_a.step()
                pol_a.load_state_dict(sd)

            def update_b():
                v, lp, ent = pol_b.evaluate_actions(obs, actions)
                loss = G.ppo_loss(v, lp, ent, adv, ret, old_lp)[0]
                opt_b.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(pol_b.parameters(), 0.5)
                opt_b.step()

            rounds = [{"update_ms_a": timed(update_a), "update_ms_b": timed(update_b)} for _ in range(args.rounds)]
            # the two paths took the same steps from the same start: the blobs agree to rounding
            drift = float((pol_a.blob - pol_b.blob.detach()).abs().max())
            d_mean, d_values, out = rnd(batch, 4), rnd(batch), torch.empty_like(pol_b.blob.detach())
            for _ in range(3):
                pol_b.backward_blob(obs, d_mean, d_values, out=out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                pol_b.backward_blob(obs, d_mean, d_values, out=out)
            e1.record()
            torch.cuda.synchronize()
            med = {key: statistics.median(x[key] for x in rounds) for key in rounds[0]}
            result["runs"].append({"case": case, "batch": batch, "rounds": rounds, "median": med,
                                   "speedup_median": med["update_ms_a"] / med["update_ms_b"],
                                   "b_faster_every_round": all(x["update_ms_b"] < x["update_ms_a"] for x in rounds),
                                   "backward_kernel_ms": e0.elapsed_time(e1) / args.reps,
                                   "blob_max_abs_diff_a_vs_b": drift})
            print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
