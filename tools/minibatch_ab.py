#!/usr/bin/env python3
"""Same-box A/B of the PPO update's minibatch gather: materialise-then-index vs the device sampler.

    python tools/minibatch_ab.py [--envs 32768] [--steps 2048] [--stacks 4,10]
                                 [--batches 256,65536,1048576] [--rounds 5]
                                 [--out profiles/minibatch_gather_ab.json]

The buffer is filled by collect_rollout (the one-launch random-policy rollout, then GAE) at
cfg4's per-GPU share. Per stack depth K, in one process:
  A = the only route before the sampler existed, from functions that predate it:
      buf.observations() once (rebuild_observations: every stacked observation), swap_and_flatten
      of the six fields, then per minibatch six torch fancy-indexing gathers on a permutation.
      The one-off materialisation (time, peak memory) is reported apart from the per-epoch
      indexing. If the materialisation does not fit in free device memory at the full n_steps,
      A runs on the first T_a steps, the largest halving of n_steps that fits (`a_steps`), and B
      is timed on those T_a steps as well (`b_same_steps_*`) next to its full-size figures.
  B = DeviceRolloutBuffer.get(batch_size): one f16env_rollout_minibatch launch per minibatch.
Per minibatch size, --rounds rounds interleaved A B A B ..., device events around a whole epoch
of minibatches over one device permutation per round, the same for both sides and drawn outside
the events (torch.randperm's own time and transient memory are recorded apart: `randperm_ms`,
`randperm_peak_bytes`); medians reported with every round kept.
B's bytes per sample are the algorithm's (read 60 K + 4 (K-1) + 8 + 16 + 16, written 60 K + 32),
its rate is set against the 6.29 TB/s achievable copy rate the README uses.
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

COPY_RATE = 6.29e12  # B/s, README's achievable HBM copy rate
A_FIELDS = ("actions", "values", "log_probs", "advantages", "returns")


def swap_and_flatten(x):
    """buffers.py:36-50 on a device tensor."""
    return x.transpose(0, 1).reshape((x.shape[0] * x.shape[1],) + tuple(x.shape[2:]))


def epoch_a(flat, perm, bs):
    last = None
    for i in range(0, perm.numel(), bs):
        idx = perm[i:i + bs]
        last = tuple(x[idx] for x in flat)
    return last


def epoch_b(source, bs):
    last = None
    for mb in source(bs):
        last = mb
    return last


def timed(fn):
    """(device ms between events around fn, host ms around fn ending in a synchronise)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def timed_value(fn):
    """(fn's value, host ms around it ending in a synchronise)."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def peak_of(fn, dev):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated(dev) - base


def materialise(buf, k, steps):
    """A's one-off: the stacked observations of the first `steps` steps, flattened with the other
    five fields."""
    from f16_jsb_amd.rollout import rebuild_observations
    obs = rebuild_observations(buf.frames[:steps], buf.obs0, buf.episode_starts[:steps], k)
    flat_obs = swap_and_flatten(obs)
    del obs
    return (flat_obs,) + tuple(swap_and_flatten(getattr(buf, f)[:steps]) for f in A_FIELDS)


def save(result, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path + ".part", "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    os.replace(path + ".part", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--stacks", default="4,10")
    ap.add_argument("--batches", default="256,65536,1048576")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minibatch_gather_ab.json"))
    args = ap.parse_args()

    import torch
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.rollout import DeviceRolloutBuffer, collect_rollout, minibatches
    if not torch.cuda.is_available():
        raise SystemExit("minibatch_ab needs a GPU")
    dev = torch.device("cuda", 0)
    n, T = args.envs, args.steps
    batches = [int(b) for b in args.batches.split(",")]
    result = {"envs": n, "steps": T, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
              "copy_rate_bytes_per_s": COPY_RATE, "stacks": []}
    for k in (int(s) for s in args.stacks.split(",")):
        envs = F16Envs(n, stack_k=k, device=dev, seed=7, obs_layout="window")
        envs.reset()
        buf = DeviceRolloutBuffer(T, n, k, dev)
        last_v, last_d = collect_rollout(envs, buf, seed=11)
        buf.compute_returns_and_advantage(last_v, last_d)
        envs.close()
        del envs
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0, total_mem = torch.cuda.mem_get_info(dev)
        entry = {"stack_k": k, "episode_start_fraction": float(buf.episode_starts.mean()),
                 "buffer_bytes": sum(x.numel() * 4 for x in buf.state_dict().values()),
                 "free_bytes_before_a": free0, "device_bytes": total_mem, "a_attempts": []}
        # A's one-off materialisation, at the largest halving of T that fits
        flat, ta = None, T
        while flat is None and ta >= 1:
            try:
                t0 = time.perf_counter()
                flat, peak = peak_of(lambda: materialise(buf, k, ta), dev)
                entry.update(a_steps=ta, a_materialise_ms=(time.perf_counter() - t0) * 1e3, a_materialise_peak_bytes=peak,
                             a_resident_bytes=sum(x.numel() * 4 for x in flat))
            except torch.cuda.OutOfMemoryError:
                entry["a_attempts"].append({"steps": ta, "fits": False})
                flat = None
                torch.cuda.empty_cache()
                ta //= 2
        if flat is None:
            raise SystemExit("A does not fit at any n_steps")
        # a second, timed materialisation now that the allocator holds the blocks (steady state)
        del flat
        t0 = time.perf_counter()
        flat = materialise(buf, k, ta)
        torch.cuda.synchronize()
        entry["a_materialise_ms_second"] = (time.perf_counter() - t0) * 1e3
        same = {f: x[:ta] if f != "obs0" else x for f, x in buf.state_dict().items()}
        read_b, written_b = 60 * k + 4 * (k - 1) + 8 + 16 + 16, 60 * k + 32
        entry.update(b_bytes_read_per_sample=read_b, b_bytes_written_per_sample=written_b, rows=[])
        for bs in batches:
            # per side: (epoch over a given device permutation, its number of transitions)
            sides = {"a": (lambda p: epoch_a(flat, p, bs), ta * n),
                     "b": (lambda p: epoch_b(lambda s: buf.get(s, indices=p), bs), T * n)}
            if ta != T:
                sides["b_same_steps"] = (lambda p: epoch_b(lambda s: minibatches(same, k, s, indices=p), bs), ta * n)
            # one untimed epoch per side warms every shape; its peak memory (the permutation already
            # drawn, so not in it) is the side's epoch peak
            perms = {m: torch.randperm(m, device=dev) for m in {m for _, m in sides.values()}}
            peaks = {tag: peak_of(lambda: fn(perms[m]), dev)[1] for tag, (fn, m) in sides.items()}
            rounds = []
            for r in range(args.rounds):
                row = {}
                for m in perms:  # a fresh permutation per round, drawn outside the epochs' events
                    perms[m] = None
                    (perms[m], peak), ms = timed_value(lambda: peak_of(lambda: torch.randperm(m, device=dev), dev))
                    if m == T * n:
                        row["randperm_ms"], row["randperm_peak_bytes"] = ms, peak
                for tag, (fn, m) in sides.items():
                    row[tag + "_epoch_ms"], row[tag + "_epoch_host_ms"] = timed(lambda: fn(perms[m]))
                rounds.append(row)
            del perms
            med = {key: statistics.median(x[key] for x in rounds) for key in rounds[0]}
            out = {"batch_size": bs, "rounds": rounds, "median": med,
                   "epoch_peak_bytes": peaks}
            for tag, (_, samples) in sides.items():
                out[tag + "_samples"] = samples
                out[tag + "_minibatches"] = -(-samples // bs)
                out[tag + "_ns_per_sample"] = med[tag + "_epoch_ms"] * 1e6 / samples
            rate = T * n * (read_b + written_b) / (med["b_epoch_ms"] * 1e-3)
            out.update(b_bytes_per_s=rate, b_fraction_of_copy_rate=rate / COPY_RATE,
                       b_over_a_per_sample=out["b_ns_per_sample"] / out["a_ns_per_sample"])
            entry["rows"].append(out)
            save(dict(result, stacks=result["stacks"] + [entry], complete=False), args.out)  # keep what is measured
            print(json.dumps({"stack_k": k, "batch_size": bs, "a_steps": ta,
                              **{key: round(v, 3) for key, v in out.items() if key.endswith("_ns_per_sample")},
                              "b_fraction_of_copy_rate": round(out["b_fraction_of_copy_rate"], 4)}), flush=True)
        result["stacks"].append(entry)
        save(result, args.out)
        del flat, same, buf
        torch.cuda.empty_cache()
    save(result, args.out)
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
