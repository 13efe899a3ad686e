#!/usr/bin/env python3
"""Same-box A/B of two builds of the four policy kernels: the bits they produce and the time they
take, each library in its own fresh process (F16ENV_LIB), parent and head alternating.

    python tools/policy_ab_builds.py build-parent [REV]   # REV (default HEAD) -> f16_jsb_amd/libf16env_ab_parent.so
    python tools/policy_ab_builds.py run [--rounds 5] [--reps 100] [--out-dir profiles]

build-parent checks REV out into a temporary git worktree and builds ITS sources with its own
build.py (as tools/ab_builds.py build does for flag variants); head is the product library.

Bits, per library and round: for every case of tests/policy_ref.MATRIX (a random net by lma_ref's
rule, 257 standard-normal rows and a fixed eps from a fixed seed) and of tests/lma_ref.MATRIX
(random_net, shared_inputs), sha256 of the raw bytes of
  actions, values, log_probs (and features for LMA) of the forward with the fixed eps, with the
  Philox stream at one (seed, step), and of the VALUE_ONLY forward (values; features for LMA);
  backward_blob's result with both upstream gradients, d_mean only and d_values only, at
  max_blocks 0, 1 and 3 (257 rows: a partial last tile, more tiles than slots at 1 and 3).
Every hash of head must equal the parent's: no tolerance. -> profiles/policy_refactor_bits.json

Time, in the same processes: device events around --reps replays of a captured graph of
  the MLP forward (policy_ref case E, the net of tools/policy_ab.py) and the LMA forward (case R) at 32 768 rows,
  the MLP backward (case E) and the LMA backward (case R) at 4 096 rows.
Accepted when head's median over the rounds <= the parent's median + the parent's own max - min
spread over its rounds in this run. -> profiles/policy_refactor_ab.json
Exit status 1 when a hash differs or a time is not accepted. Needs a GPU (no fallback).
"""
from __future__ import annotations

import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PARENT = os.path.join(ROOT, "f16_jsb_amd", "libf16env_ab_parent.so")
HEAD = os.path.join(ROOT, "f16_jsb_amd", "libf16env.so")
MLP_TIMED, LMA_TIMED, FWD_ROWS, BWD_ROWS = "E", "R", 32768, 4096


def build_parent(rev):
    tree = tempfile.mkdtemp(prefix="f16_parent_")
    subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", tree, rev], check=True)
    try:
        subprocess.run([sys.executable, "-c", "from f16_jsb_amd.build import build; build(force=True, out=%r)" % PARENT],
                       cwd=tree, check=True)
    finally:
        subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", tree], check=True)
    print("built", PARENT, "from", rev)


def run_one(reps):
    import numpy as np
    import torch
    import lma_ref
    import policy_ref
    from f16_jsb_amd.lma_policy import DeviceLMATrainPolicy
    from f16_jsb_amd.policy import DevicePolicy
    from policy_ab import graph_of, time_replays
    if not torch.cuda.is_available():
        raise SystemExit("policy_ab_builds needs a GPU")
    dev = torch.device("cuda", 0)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)  # noqa: E731
    pair = lambda wb: (t(wb[0]), t(wb[1]))  # noqa: E731
    digest = lambda *xs: hashlib.sha256(b"".join(x.detach().cpu().numpy().tobytes() for x in xs)).hexdigest()  # noqa: E731

    def mlp(name):
        k, d, pi_w, vf_w, _ = policy_ref.MATRIX[name]
        rng = np.random.default_rng(31000 + sum(map(ord, name)))
        lin = lambda o, i: (rng.standard_normal((o, i)) * (2.0 / i) ** 0.5, rng.standard_normal(o) * 0.1)  # noqa: E731

        def branch(widths):
            out, fan_in = [], k * d
            for w in widths:
                out.append(pair(lin(w, fan_in)))
                fan_in = w
            return out
        pol = DevicePolicy.from_layers(branch(pi_w), branch(vf_w), pair(lin(4, pi_w[-1])), pair(lin(1, vf_w[-1])),
                                       t([-0.5, 0.0, 0.25, 0.5]), stack_k=k, frame_dim=d, device=dev)
        return pol, rng.standard_normal((lma_ref.N_ROWS, k, d)), rng.standard_normal((lma_ref.N_ROWS, 4))

    def lma(name):
        k, d, _, _, _, _, act, hs, _ = lma_ref.MATRIX[name]
        net = lma_ref.random_net(name)
        ext = {"embed": pair(net["embed"]), "embed2": pair(net["embed2"]),
               "blocks": [{key: pair(v) for key, v in blk.items()} for blk in net["blocks"]]}
        pol = DeviceLMATrainPolicy.from_layers(ext, [pair(l) for l in net["pi"]], [pair(l) for l in net["vf"]],
                                               pair(net["act"]), pair(net["val"]), t(net["log_std"]), stack_k=k,
                                               frame_dim=d, activation=act, heads_stacking=hs, device=dev)
        return (pol,) + lma_ref.shared_inputs(name)

    def upstream(n):
        g = torch.Generator(device="cpu").manual_seed(n)
        return (torch.randn(n, 4, generator=g) / n).to(dev), (torch.randn(n, generator=g) / n).to(dev)

    bits = {}
    for kind, make, names in (("mlp", mlp, policy_ref.MATRIX), ("lma", lma, lma_ref.MATRIX)):
        for name in names:
            pol, obs, eps = make(name)
            obs, eps = t(obs), t(eps)
            pol.seed, h = 0x1234567, {}
            if kind == "lma":
                h["forward_eps"] = digest(*pol.forward_with_features(obs, 0, eps=eps))
                h["forward_philox"] = digest(*pol.forward_with_features(obs, 77))
                h["value_only"] = digest(pol.value(obs), pol.extract_features(obs))
            else:
                h["forward_eps"] = digest(*pol(obs, step=0, eps=eps))
                h["forward_philox"] = digest(*pol(obs, step=77))
                h["value_only"] = digest(pol.value(obs))
            dm, dv = upstream(obs.shape[0])
            for mb in (0, 1, 3):
                for tag, a, b in (("both", dm, dv), ("d_mean", dm, None), ("d_values", None, dv)):
                    h["backward_%s_mb%d" % (tag, mb)] = digest(pol.backward_blob(obs, a, b, max_blocks=mb))
            bits["%s_%s" % (kind, name)] = h

    times = {}
    for kind, make, name in (("mlp", mlp, MLP_TIMED), ("lma", lma, LMA_TIMED)):
        pol = make(name)[0]
        g = torch.Generator(device="cpu").manual_seed(5)
        obs = torch.randn(FWD_ROWS, pol.k, pol.d, generator=g).to(dev)
        outs = (torch.empty((FWD_ROWS, 4), device=dev), torch.empty(FWD_ROWS, device=dev), torch.empty(FWD_ROWS, device=dev))
        times["%s_forward_ms" % kind] = time_replays(graph_of(lambda: pol.forward_into(obs, 0, *outs), dev).replay, reps)
        obs_b, (dm, dv) = obs[:BWD_ROWS].contiguous(), upstream(BWD_ROWS)
        grad = torch.empty(pol.n_floats, device=dev)
        pol.reserve_backward(BWD_ROWS)
        times["%s_backward_ms" % kind] = time_replays(
            graph_of(lambda: pol.backward_blob(obs_b, dm, dv, out=grad), dev).replay, reps)
    print(json.dumps({"bits": bits, "times": times, "device": torch.cuda.get_device_name(0)}), flush=True)


def run(rounds, reps, out_dir):
    libs = (("parent", PARENT), ("head", HEAD))
    for _, path in libs:
        if not os.path.exists(path):
            raise SystemExit("%s is missing (build-parent / python -m f16_jsb_amd.build)" % path)
    out = {name: [] for name, _ in libs}
    for r in range(rounds):
        for name, path in libs:
            p = subprocess.run([sys.executable, __file__, "one", "--reps", str(reps)], env=dict(os.environ, F16ENV_LIB=path),
                               capture_output=True, text=True, timeout=280)
            if p.returncode != 0:  # (a fault is a finding: nothing more is started on the device)
                raise SystemExit("%s round %d FAILED rc %d\n%s" % (name, r, p.returncode, p.stderr[-3000:]))
            out[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("round %d %-6s %s" % (r, name, json.dumps(out[name][-1]["times"])), flush=True)
    device = out["head"][0]["device"]
    for name in out:  # a library's own rounds agree with one another (the kernels are deterministic)
        assert all(x["bits"] == out[name][0]["bits"] for x in out[name]), "%s: hashes differ between rounds" % name
    pb, hb = out["parent"][0]["bits"], out["head"][0]["bits"]
    differing = sorted("%s.%s" % (c, k) for c in pb for k in pb[c] if hb[c][k] != pb[c][k])
    with open(os.path.join(out_dir, "policy_refactor_bits.json"), "w") as f:
        json.dump({"device": device, "rows": 257, "hashes_compared": sum(len(v) for v in pb.values()),
                   "identical": not differing, "differing": differing, "parent": pb, "head": hb}, f, indent=1)
        f.write("\n")
    ab, ok = {"device": device, "rounds": rounds, "reps": reps, "forward_rows": FWD_ROWS, "backward_rows": BWD_ROWS,
              "mlp_case": MLP_TIMED, "lma_case": LMA_TIMED, "kernels": {}}, not differing
    for key in out["head"][0]["times"]:
        pt, ht = [x["times"][key] for x in out["parent"]], [x["times"][key] for x in out["head"]]
        row = {"parent_ms": pt, "head_ms": ht, "parent_median": statistics.median(pt), "head_median": statistics.median(ht),
               "parent_spread": max(pt) - min(pt), "head_spread": max(ht) - min(ht)}
        row["accepted"] = row["head_median"] <= row["parent_median"] + row["parent_spread"]
        ok = ok and row["accepted"]
        ab["kernels"][key] = row
    with open(os.path.join(out_dir, "policy_refactor_ab.json"), "w") as f:
        json.dump(ab, f, indent=1)
        f.write("\n")
    print(json.dumps({"identical": not differing, "differing": differing,
                      "times": {k: {x: v[x] for x in ("parent_median", "head_median", "parent_spread", "accepted")}
                                for k, v in ab["kernels"].items()}}, indent=1), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    arg = lambda flag, default: int(sys.argv[sys.argv.index(flag) + 1]) if flag in sys.argv else default  # noqa: E731
    cmd = sys.argv[1] if len(sys.argv) > 1 else "run"
    if cmd == "build-parent":
        build_parent(sys.argv[2] if len(sys.argv) > 2 else "HEAD")
    elif cmd == "one":
        run_one(arg("--reps", 100))
    else:
        out_dir = sys.argv[sys.argv.index("--out-dir") + 1] if "--out-dir" in sys.argv else os.path.join(ROOT, "profiles")
        os.makedirs(out_dir, exist_ok=True)
        sys.exit(run(arg("--rounds", 5), arg("--reps", 100), out_dir))
