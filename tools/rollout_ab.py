#!/usr/bin/env python3
"""Same-box A/B of two Python trees of the package on ONE libf16env.so: the bits its host-side code
leaves and the host time a step of it takes, each tree in its own fresh process, parent and head
alternating (tools/policy_ab_builds.py's pattern with the roles swapped: there the library changed
and the Python stayed). --suite rollout (default): the rollout collector
(f16_jsb_amd.rollout.collect_rollout); --suite facades: the drop-in boundary (F16VecEnv,
F16GymVectorEnv, F16GymEnv). The driver is one; a suite is the body of a child and two file names.

    python tools/rollout_ab.py export-parent DIR [REV]     # REV's tree (default HEAD) -> DIR
    python tools/rollout_ab.py run [--suite rollout|facades] [--parent-tree DIR | --rev REV] [--rounds 5]
                                   [--out-dir profiles]

The parent's tree is REV checked out into a temporary git worktree for the run, or a directory
export-parent made earlier (for a machine that has the files and no history). Both sides load the
product library through F16ENV_LIB; nothing is started after a child that failed. Every hash of head
must equal the parent's: no tolerance. A time is accepted when head's median over the rounds <= the
parent's median + the parent's own max - min spread over its rounds in this run. Exit status 1 when
a hash differs or a time is not accepted. Needs a GPU (no fallback).

--suite rollout.
Bits, per tree and round: N = 257 envs (one full 256-lane block and one lane) and N = 260 (at 257 a
frame row is no multiple of 16 bytes, so the contiguous layout collects on the generic path: 260 is
the nearest count at which it takes the fused ones), K = 4, T = 12, max_steps = 5 (every lane
truncates inside the rollout), two consecutive rollouts on one handle (the second starts from the
carried episode starts), both layouts, for
  the random policy persistent, fused (persistent=False) and generic (fused=False),
  a closure policy and a DevicePolicy, each with bootstrap "deferred" and "per_step",
  the closure on the generic path, and one cfg5 handle on the windowed layout (random persistent,
  random fused, DevicePolicy deferred):
sha256 of the raw bytes of every FIELDS tensor (after GAE), obs0, last_values, last_dones and the
env's final observation. -> profiles/rollout_refactor_bits.json

Time, in the same processes: the host clock around collect_rollout plus a synchronise, over T = 256
steps, per step, the median of --reps rollouts after a warm one; at 256 envs (the launch path sets
the time, not the kernel) and at bench.py's default --rollout-envs (32 768), for the windowed and
the contiguous layout fused with the random policy and the windowed layout with a DevicePolicy and
the deferred bootstrap. -> profiles/rollout_refactor_ab.json

--suite facades, through f16_jsb_amd.make / make_vec / F16GymEnv alone (what both trees have). Bits:
N = 257, K = 4 and 10, max_steps = 7, history = max(16, 2K), 140 steps of default_rng(1) Box actions
(past the host mirror's default ring of max(128, 4K) positions: one host restart), for F16VecEnv in
numpy mode, with copy_obs=True and in device mode on both layouts, F16GymVectorEnv in numpy and
device mode, and F16GymEnv (30 steps); seed(100) / reset(seed=100) first, env_method("reset",
indices=[0, 3]) once at step 50 and get_attr of goal, current_step and state at the end on the
F16VecEnv variants. One sha256 per output over the raw bytes of all steps: obs, rewards, dones /
terminated / truncated; of finished lanes terminal_observation, TimeLimit.truncated and episode r, l
(final_obs, _final_obs, episode r, l); the wall-clock "t" alone is left out.
-> profiles/facade_refactor_bits.json
Time: the host clock around step() -- the outputs are on the host, or a synchronise follows in
device mode -- per step, the median of --reps blocks of 50 steps after a warm block: F16VecEnv numpy
mode at 256 envs, K = 4 (the Python path sets the time) and at 65 536 envs, K = 10 (bench.py's
sb3_compat_bench shape), F16GymVectorEnv numpy mode and F16VecEnv device mode at 256 envs.
-> profiles/facade_refactor_ab.json
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "f16_jsb_amd", "libf16env.so")
N_ENVS, K, T, MAX_STEPS, SEED, STEP0 = (257, 260), 4, 12, 5, 21, 1000
TIMED_T, TIMED_ENVS = 256, (256, 32768)
FACADE_N, FACADE_K, FACADE_STEPS, FACADE_MAX_STEPS, FACADE_BLOCK = 257, (4, 10), 140, 7, 50


def export_parent(dest, rev):
    """REV's package sources into DEST (git archive: tracked files only, no build products)."""
    os.makedirs(dest, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "f16_jsb_amd"], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", dest], input=tar, check=True)
    print("exported", rev, "to", dest)


def enter_tree(tree):
    """A child's start: the package of `tree` and no other, and a GPU."""
    sys.path.insert(0, tree)
    import torch
    import f16_jsb_amd
    assert os.path.dirname(os.path.abspath(f16_jsb_amd.__file__)) == os.path.join(os.path.abspath(tree), "f16_jsb_amd")
    if not torch.cuda.is_available():
        raise SystemExit("rollout_ab needs a GPU")
    return torch, torch.device("cuda", 0)


def one_rollout(tree, reps):
    torch, dev = enter_tree(tree)
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.policy import DevicePolicy
    from f16_jsb_amd.rollout import FIELDS, DeviceRolloutBuffer, collect_rollout
    digest = lambda x: hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest()  # noqa: E731

    def policy():  # SB3's default MlpPolicy shape, random weights; log_std = 1: samples leave the action Box
        g = torch.Generator(device="cpu").manual_seed(2)
        lin = lambda i, o: ((torch.randn(o, i, generator=g) * (2.0 / i) ** 0.5).to(dev),  # noqa: E731
                            (torch.randn(o, generator=g) * 0.1).to(dev))
        return DevicePolicy.from_layers([lin(K * 15, 64), lin(64, 64)], [lin(K * 15, 64), lin(64, 64)], lin(64, 4),
                                        lin(64, 1), torch.ones(4, device=dev), stack_k=K, seed=SEED)
    pol = policy()

    def collect(envs, buf, kind, step0, **kw):
        if kind == "random":
            return collect_rollout(envs, buf, SEED, step0, **kw)
        if kind == "device":
            return collect_rollout(envs, buf, SEED, step0, policy_fn=pol, **kw)
        calls = []

        def closure(obs):
            calls.append(1)
            return pol(obs, step=step0 + len(calls) - 1)
        return collect_rollout(envs, buf, SEED, step0, policy_fn=closure, value_fn=pol.value, **kw)

    cases = [("random_persistent", "random", {}), ("random_fused", "random", {"persistent": False}),
             ("random_generic", "random", {"fused": False}), ("closure_generic", "closure", {"fused": False})]
    cases += [("%s_%s" % (kind, b), kind, {"bootstrap": b}) for kind in ("closure", "device") for b in ("deferred", "per_step")]
    cfg5_cases = [c for c in cases if c[0] in ("random_persistent", "random_fused", "device_deferred")]
    bits = {}
    for n, (tag, layout, env_kw, todo) in itertools.product(N_ENVS, (
            ("contiguous", "contiguous", {}, cases), ("window", "window", {}, cases),
            ("window_cfg5", "window", {"cfg5": True}, cfg5_cases))):
        for name, kind, kw in todo:
            envs = F16Envs(n, stack_k=K, device=dev, seed=5, obs_layout=layout, max_steps=MAX_STEPS, **env_kw)
            envs.reset()
            buf, h = DeviceRolloutBuffer(T, n, K, dev), {}
            for r in range(2):
                last_v, last_d = collect(envs, buf, kind, STEP0 + r * T, **kw)
                buf.compute_returns_and_advantage(last_v, last_d)
                for f in FIELDS + ("obs0",):
                    h["rollout%d.%s" % (r, f)] = digest(getattr(buf, f))
                h["rollout%d.last_values" % r], h["rollout%d.last_dones" % r] = digest(last_v), digest(last_d)
                h["rollout%d.final_obs" % r] = digest(envs.obs)
            envs.close()
            bits["n%d.%s.%s" % (n, tag, name)] = h

    times = {}
    for n in TIMED_ENVS:
        for name, layout, kind, kw in (("window_random_fused", "window", "random", {"persistent": False}),
                                       ("contiguous_random_fused", "contiguous", "random", {"persistent": False}),
                                       ("window_device_deferred", "window", "device", {"bootstrap": "deferred"})):
            envs = F16Envs(n, stack_k=K, device=dev, seed=5, obs_layout=layout)
            envs.reset()
            buf, per_step = DeviceRolloutBuffer(TIMED_T, n, K, dev), []
            for r in range(reps + 1):  # (the first is the warm one)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                collect(envs, buf, kind, r * TIMED_T, **kw)
                torch.cuda.synchronize(dev)
                per_step.append((time.perf_counter() - t0) / TIMED_T * 1e6)
            envs.close()
            times["%s_n%d_us_per_step" % (name, n)] = statistics.median(per_step[1:])
    print(json.dumps({"bits": bits, "times": times, "device": torch.cuda.get_device_name(0)}), flush=True)


def one_facades(tree, reps):
    torch, dev = enter_tree(tree)
    import numpy as np
    import f16_jsb_amd
    from f16_jsb_amd import F16GymEnv

    class Hashes(dict):  # one running sha256 per named output
        def add(self, name, x):
            x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
            self.setdefault(name, hashlib.sha256()).update(np.ascontiguousarray(x).tobytes())

        def done(self):
            return {k: v.hexdigest() for k, v in self.items()}

    box = lambda rng, n: rng.uniform([-1, -1, -1, 0], [1, 1, 1, 1], (n, 4)).astype(np.float32)  # noqa: E731

    def vec_run(h, k, **kw):
        numpy_mode = kw.get("return_numpy", True)
        env = f16_jsb_amd.make(num_envs=FACADE_N, stack_k=k, device=dev, seed=3, max_steps=FACADE_MAX_STEPS,
                               history=max(16, 2 * k), **kw)
        env.seed(100)
        h.add("reset", env.reset())
        rng = np.random.default_rng(1)
        for t in range(FACADE_STEPS):
            if t == 50:
                for o, _ in env.env_method("reset", indices=[0, 3]):
                    h.add("masked_reset", o)
            act = box(rng, FACADE_N)
            obs, rew, dones, infos = env.step(act if numpy_mode else torch.as_tensor(act, device=dev))
            h.add("obs", obs), h.add("rew", rew), h.add("dones", dones)
            for i in (np.flatnonzero(dones) if numpy_mode else ()):
                h.add("terminal_observation", infos[i]["terminal_observation"])
                h.add("TimeLimit.truncated", infos[i]["TimeLimit.truncated"])
                h.add("episode.r", infos[i]["episode"]["r"]), h.add("episode.l", infos[i]["episode"]["l"])
        for attr in ("goal", "current_step", "state"):
            h.add("get_attr." + attr, np.stack(env.get_attr(attr)))
        env.close()

    def gymvec_run(h, k, **kw):
        numpy_mode = kw.get("return_numpy", True)
        env = f16_jsb_amd.make_vec(num_envs=FACADE_N, stack_k=k, device=dev, seed=3, max_steps=FACADE_MAX_STEPS,
                                   history=max(16, 2 * k), **kw)
        h.add("reset", env.reset(seed=100)[0])
        rng = np.random.default_rng(1)
        for t in range(FACADE_STEPS):
            act = box(rng, FACADE_N)
            obs, rew, term, trunc, infos = env.step(act if numpy_mode else torch.as_tensor(act, device=dev))
            h.add("obs", obs), h.add("rew", rew), h.add("terminated", term), h.add("truncated", trunc)
            if infos:
                h.add("final_obs", infos["final_obs"]), h.add("_final_obs", infos["_final_obs"])
                h.add("episode.r", infos["episode"]["r"]), h.add("episode.l", infos["episode"]["l"])
        env.close()

    def gymenv_run(h, k):
        env = F16GymEnv(stack_k=k, device=dev, seed=3, max_steps=FACADE_MAX_STEPS)
        h.add("reset", env.reset(seed=100)[0])
        rng = np.random.default_rng(1)
        for t in range(30):
            obs, rew, term, trunc, _ = env.step(box(rng, 1)[0])
            h.add("obs", obs), h.add("rew", rew), h.add("terminated", term), h.add("truncated", trunc)
            if term or trunc:  # (no auto-reset: the caller resets, as with the reference)
                h.add("reset", env.reset(seed=100 + t)[0])
        env.close()

    bits = {}
    for k in FACADE_K:
        for name, fn, kw in (("vec_numpy", vec_run, {}), ("vec_copy_obs", vec_run, {"copy_obs": True}),
                             ("vec_device_contiguous", vec_run, {"return_numpy": False}),
                             ("vec_device_window", vec_run, {"return_numpy": False, "obs_layout": "window"}),
                             ("gymvec_numpy", gymvec_run, {}), ("gymvec_device", gymvec_run, {"return_numpy": False}),
                             ("gymenv", gymenv_run, {})):
            h = Hashes()
            fn(h, k, **kw)
            bits["k%d.%s" % (k, name)] = h.done()

    times = {}
    for name, make, n, k, kw in (("vec_numpy", f16_jsb_amd.make, 256, 4, {}), ("vec_numpy", f16_jsb_amd.make, 65536, 10, {}),
                                 ("gymvec_numpy", f16_jsb_amd.make_vec, 256, 4, {}),
                                 ("vec_device", f16_jsb_amd.make, 256, 4, {"return_numpy": False})):
        env = make(num_envs=n, stack_k=k, device=dev, seed=5, **kw)
        env.reset()
        act = box(np.random.default_rng(2), n)
        act = act if kw.get("return_numpy", True) else torch.as_tensor(act, device=dev)
        per_step = []
        for r in range(reps + 1):  # (the first is the warm one)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(FACADE_BLOCK):
                env.step(act)
            torch.cuda.synchronize(dev)
            per_step.append((time.perf_counter() - t0) / FACADE_BLOCK * 1e6)
        env.close()
        times["%s_n%d_k%d_us_per_step" % (name, n, k)] = statistics.median(per_step[1:])
    print(json.dumps({"bits": bits, "times": times, "device": torch.cuda.get_device_name(0)}), flush=True)


# a suite: the body of a child, the two output names, what its two files say of its settings
SUITES = {
    "rollout": (one_rollout, "rollout_refactor_bits.json", "rollout_refactor_ab.json",
                {"n_envs": N_ENVS, "stack_k": K, "n_steps": T, "max_steps": MAX_STEPS}, {"n_steps": TIMED_T}),
    "facades": (one_facades, "facade_refactor_bits.json", "facade_refactor_ab.json",
                {"n_envs": FACADE_N, "stack_k": FACADE_K, "n_steps": FACADE_STEPS, "max_steps": FACADE_MAX_STEPS},
                {"n_steps": FACADE_BLOCK}),
}


def run(parent_tree, rounds, reps, out_dir, suite):
    if not os.path.exists(LIB):
        raise SystemExit("%s is missing (python -m f16_jsb_amd.build)" % LIB)
    _, bits_name, ab_name, bits_meta, ab_meta = SUITES[suite]
    trees = (("parent", parent_tree), ("head", ROOT))
    out = {name: [] for name, _ in trees}
    for r in range(rounds):
        for name, tree in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "one", "--suite", suite, "--tree", tree,
                                "--reps", str(reps)],
                               env=dict(os.environ, F16ENV_LIB=LIB), cwd=tree, capture_output=True, text=True, timeout=280)
            if p.returncode != 0:  # (a fault is a finding: nothing more is started on the device)
                raise SystemExit("%s round %d FAILED rc %d\n%s" % (name, r, p.returncode, p.stderr[-3000:]))
            out[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("round %d %-6s %s" % (r, name, json.dumps(out[name][-1]["times"])), flush=True)
    device = out["head"][0]["device"]
    for name in out:  # a tree's own rounds agree with one another (the kernels are deterministic)
        assert all(x["bits"] == out[name][0]["bits"] for x in out[name]), "%s: hashes differ between rounds" % name
    pb, hb = out["parent"][0]["bits"], out["head"][0]["bits"]
    differing = sorted("%s.%s" % (c, k) for c in pb for k in pb[c] if hb[c][k] != pb[c][k])
    with open(os.path.join(out_dir, bits_name), "w") as f:
        json.dump({"device": device, **bits_meta, "hashes_compared": sum(len(v) for v in pb.values()), "identical": not differing,
                   "differing": differing, "parent": pb, "head": hb}, f, indent=1)
        f.write("\n")
    ab, ok = {"device": device, "rounds": rounds, "reps": reps, **ab_meta, "unit": "us of host time per step",
              "cases": {}}, not differing
    for key in out["head"][0]["times"]:
        pt, ht = [x["times"][key] for x in out["parent"]], [x["times"][key] for x in out["head"]]
        row = {"parent_us": pt, "head_us": ht, "parent_median": statistics.median(pt), "head_median": statistics.median(ht),
               "parent_spread": max(pt) - min(pt), "head_spread": max(ht) - min(ht)}
        row["accepted"] = row["head_median"] <= row["parent_median"] + row["parent_spread"]
        ok = ok and row["accepted"]
        ab["cases"][key] = row
    with open(os.path.join(out_dir, ab_name), "w") as f:
        json.dump(ab, f, indent=1)
        f.write("\n")
    print(json.dumps({"identical": not differing, "differing": differing, "hashes_compared": sum(len(v) for v in pb.values()),
                      "times": {k: {x: round(v[x], 3) if x != "accepted" else v[x]
                                    for x in ("parent_median", "head_median", "parent_spread", "accepted")}
                                for k, v in ab["cases"].items()}}, indent=1), flush=True)
    return 0 if ok else 1


def main(argv):
    opt = lambda flag, default: argv[argv.index(flag) + 1] if flag in argv else default  # noqa: E731
    cmd = argv[1] if len(argv) > 1 else "run"
    if cmd == "export-parent":
        return export_parent(argv[2], argv[3] if len(argv) > 3 else "HEAD")
    suite = opt("--suite", "rollout")
    if suite not in SUITES:
        raise SystemExit("--suite is one of %s" % ", ".join(SUITES))
    if cmd == "one":
        return SUITES[suite][0](opt("--tree", ROOT), int(opt("--reps", 5)))
    out_dir = opt("--out-dir", os.path.join(ROOT, "profiles"))
    os.makedirs(out_dir, exist_ok=True)
    parent_tree, made = opt("--parent-tree", None), None
    if parent_tree is None:
        parent_tree = made = tempfile.mkdtemp(prefix="f16_parent_")
        subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", made, opt("--rev", "HEAD")], check=True)
    try:
        return run(os.path.abspath(parent_tree), int(opt("--rounds", 5)), int(opt("--reps", 5)), out_dir, suite)
    finally:
        if made:
            subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", made], check=True)
            shutil.rmtree(made, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
