#!/usr/bin/env python3
"""Same-box A/B of one minibatch gradient of the LMA policy into blob layout, and the precision record.

    python tools/lma_backward_ab.py [--rounds 5] [--reps 10] [--out profiles/lma_backward_ab.json]
    python tools/lma_backward_ab.py --precision [--out profiles/lma_backward_precision.json]

A = what a caller has without the backward kernel: the network restated in torch float32 on the
    same GPU (tests/lma_grad_ref.py: forward), autograd's backward of sum d_mean . mean +
    d_values value, and the repack of the gradients into a blob (pack_lma_blob);
B = DeviceLMATrainPolicy.backward_blob (f16env_policy_lma_backward: two launches).
Shapes: case R at 256 rows (the reference's minibatch), 4 096 and 65 536, and case S at 256. Per
shape, in one process, interleaved A B A B ... for --rounds rounds: host clock around --reps
gradients ending in a device synchronise; medians. B alone is also timed by device events.
--precision: per matrix case at 257 rows and per stress input, r, F and the kernel's largest error
ratio to the allowance base per tensor (the rule of tests/lma_grad_ref.py). Needs a GPU (no fallback).
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", nargs="+", default=["R:256", "R:4096", "R:65536", "S:256"])
    ap.add_argument("--precision", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import lma_grad_ref as G
    import lma_ref
    from f16_jsb_amd.lma_policy import DeviceLMATrainPolicy
    if not torch.cuda.is_available():
        raise SystemExit("lma_backward_ab needs a GPU")
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)  # noqa: E731
    pair = lambda wb: (t(wb[0]), t(wb[1]))  # noqa: E731

    def policy(net, k, d, act, hs):
        ext = {"embed": pair(net["embed"]), "embed2": pair(net["embed2"]),
               "blocks": [{key: pair(v) for key, v in blk.items()} for blk in net["blocks"]]}
        return DeviceLMATrainPolicy.from_layers(ext, [pair(l) for l in net["pi"]], [pair(l) for l in net["vf"]],
                                                pair(net["act"]), pair(net["val"]), t(net["log_std"]), stack_k=k,
                                                frame_dim=d, activation=act, heads_stacking=hs)

    result = {"device": torch.cuda.get_device_name(0)}
    if args.precision:
        out_path = args.out or os.path.join(ROOT, "profiles", "lma_backward_precision.json")
        result["rule"] = "allowance = F x max(torch float32 error, 2^-24 max|ref|), F = max(4, 2 r); ratios are error / base"
        result["inputs"] = []
        inputs = [(name, G.case_input(name), G.case_rule(name), lma_ref.MATRIX[name][:2]) for name in lma_ref.MATRIX]
        inputs += [(kind, G.stress_input(kind), G.stress_rule(kind), lma_ref.MATRIX[lma_ref.STRESS_CASE][:2])
                   for kind in lma_ref.STRESS]
        for label, (net, obs, dm, dv, act, hs), rule, (k, d) in inputs:
            pol = policy(net, k, d, act, hs)
            got = pol.backward_blob(t(obs), t(dm), t(dv))
            ratios = rule.ratios(G.unpack(pol.desc, pol.lma, got))
            worst = max(ratios, key=ratios.get)
            result["inputs"].append({"input": label, "rows": int(len(obs)), "r": rule.r, "F": rule.F,
                                     "kernel_max_ratio": ratios[worst], "kernel_worst_tensor": worst,
                                     "within_allowance": ratios[worst] <= rule.F,
                                     "finite": bool(torch.isfinite(got).all()), "kernel_ratios": ratios})
            print(json.dumps({key: v for key, v in result["inputs"][-1].items() if key != "kernel_ratios"}), flush=True)
    else:
        out_path = args.out or os.path.join(ROOT, "profiles", "lma_backward_ab.json")
        result.update(rounds=args.rounds, reps=args.reps, runs=[])

        def timed(fn):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.reps * 1e3

        for shape in args.shapes:
            case, batch = shape.split(":")
            batch = int(batch)
            k, d, nl, ff, pi_w, vf_w, act, hs, _ = lma_ref.MATRIX[case]
            net = lma_ref.random_net(case)
            pol = policy(net, k, d, act, hs)
            g = torch.Generator(device="cpu").manual_seed(batch)
            obs = torch.randn(batch, k, d, generator=g).to(dev)
            dm, dv = (torch.randn(batch, 4, generator=g) / batch).to(dev), (torch.randn(batch, generator=g) / batch).to(dev)
            out_b = torch.empty(pol.n_floats, device=dev)
            pol.reserve_backward(batch)
            leaves = G.leaves(net, torch.float32, dev)
            holder = {}

            def grad_a():
                for _, p in G.named_tensors(leaves):
                    p.grad = None
                _, mean, values = G.forward(leaves, obs, torch.float32, act, hs)
                ((mean * dm).sum() + (values * dv).sum()).backward()
                grads = {"embed": tuple(p.grad for p in leaves["embed"]), "embed2": tuple(p.grad for p in leaves["embed2"]),
                         "blocks": [{piece: tuple(p.grad for p in blk[piece]) for piece in lma_ref.BLOCK_PIECES}
                                    for blk in leaves["blocks"]],
                         "pi": [tuple(p.grad for p in l) for l in leaves["pi"]],
                         "vf": [tuple(p.grad for p in l) for l in leaves["vf"]],
                         "act": tuple(p.grad for p in leaves["act"]), "val": tuple(p.grad for p in leaves["val"])}
                holder["a"] = G.pack(pol.desc, pol.lma, grads, device=dev)

            def grad_b():
                pol.backward_blob(obs, dm, dv, out=out_b)

            rounds = [{"grad_ms_a": timed(grad_a), "grad_ms_b": timed(grad_b)} for _ in range(args.rounds)]
            diff = float((holder["a"] - out_b).abs().max())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                grad_b()
            e1.record()
            torch.cuda.synchronize()
            med = {key: statistics.median(x[key] for x in rounds) for key in rounds[0]}
            result["runs"].append({"case": case, "batch": batch, "rounds": rounds, "median": med,
                                   "speedup_median": med["grad_ms_a"] / med["grad_ms_b"],
                                   "b_faster_every_round": all(x["grad_ms_b"] < x["grad_ms_a"] for x in rounds),
                                   "backward_device_ms": e0.elapsed_time(e1) / args.reps,
                                   "grad_max_abs": float(out_b.abs().max()), "grad_max_abs_diff_a_vs_b": diff})
            print(json.dumps(result["runs"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": out_path}))


if __name__ == "__main__":
    main()
