"""The observation layouts of F16Envs agree through every mutating operation: a contiguous
handle, a position-major and an env-major windowed handle (and, in a second run, windowed handles
with fused_features / fused_poses against a plain one) are driven through one fixed interleaving
of reset, masked reset, every form of step, the rollout-slot step, the one-launch rollout,
set_obs, get_state -> set_state and enough plain steps to restart the short histories several
times; after each operation their observations, step outputs, policy features and poses must be
bit-identical. N = 70 (one full and one partial wave), K = 3, history 6 = 2K (a restart every 4
steps; rollout_random meets both a window that fits beside the current one and one that does
not), max_steps 5 (every lane truncates and auto-resets at a known step).

The windowed handles' feature_window_calls after each operation are compared with CALLS, which
was recorded on an MI355X from the commit before the layout classes existed (this same test with
F16_LAYOUT_RECORD=<file> set, which writes the counts instead of asserting them): the rule for
when the feature windows are current is measured against the old code, not the code under test."""
from __future__ import annotations

import json
import os

import pytest

pytestmark = pytest.mark.gpu

N, K, HIST, MAX_STEPS, SEED = 70, 3, 6, 5, 13
OPS = ["reset", "step", "step", "step_done", "step_none", "step_feat", "slot", "slot_policy", "masked_reset", "step",
       "rollout", "rollout", "step", "rollout", "step", "step", "rollout", "set_obs", "step", "state", "step",
       "step_pair", "step", "slot", "slot", "step_none", "step", "step", "masked_reset", "step_pair", "step", "step",
       "step", "step", "reset", "step_feat", "step", "step", "step", "step"]
# (incremental, full, fused) of feature_window_calls after each op of OPS, recorded at the parent
CALLS = {
    "plain": [[0, 1, 0], [0, 2, 0], [1, 2, 0], [2, 2, 0], [3, 2, 0], [3, 2, 1], [3, 2, 2], [3, 2, 3], [3, 3, 3], [3, 4, 3],
              [3, 5, 3], [3, 6, 3], [3, 7, 3], [3, 8, 3], [3, 9, 3], [4, 9, 3], [4, 10, 3], [4, 11, 3], [4, 12, 3],
              [4, 13, 3], [4, 14, 3], [4, 15, 3], [5, 15, 3], [5, 15, 4], [5, 15, 5], [6, 15, 5], [7, 15, 5], [8, 15, 5],
              [8, 16, 5], [8, 17, 5], [9, 17, 5], [10, 17, 5], [11, 17, 5], [12, 17, 5], [12, 18, 5], [12, 19, 5],
              [13, 19, 5], [14, 19, 5], [15, 19, 5], [16, 19, 5]],
    "fused": [[0, 1, 0], [0, 2, 0], [0, 2, 1], [1, 2, 1], [1, 2, 2], [1, 2, 3], [1, 2, 4], [1, 2, 5], [1, 3, 5], [1, 4, 5],
              [1, 5, 5], [1, 6, 5], [1, 7, 5], [1, 8, 5], [1, 9, 5], [1, 9, 6], [1, 10, 6], [1, 11, 6], [1, 12, 6],
              [1, 13, 6], [1, 14, 6], [1, 14, 8], [1, 14, 9], [1, 14, 10], [1, 14, 11], [1, 14, 12], [1, 14, 13],
              [1, 14, 14], [1, 15, 14], [1, 16, 15], [1, 16, 16], [1, 16, 17], [1, 16, 18], [1, 16, 19], [1, 17, 19],
              [1, 18, 19], [1, 18, 20], [1, 18, 21], [1, 18, 22], [1, 18, 23]],
}


def _apply(e, op, i, torch):
    """One operation on one handle; returns the extra tensors it filled (compared across handles)."""
    f32 = dict(dtype=torch.float32, device=e.device)
    if op == "reset":
        e.reset()
    elif op == "masked_reset":
        e.reset(mask=torch.arange(N, device=e.device) % 3 == i % 3)
    elif op == "step":
        e.step(e.sample_actions(3, i))
    elif op == "step_pair":  # a step whose features nobody asks for, then another
        e.step(e.sample_actions(3, i))
        e.step(e.sample_actions(4, i))
    elif op == "step_done":
        idx, cnt = torch.zeros(N, dtype=torch.int32, device=e.device), torch.zeros(1, dtype=torch.int32, device=e.device)
        e.step(e.sample_actions(3, i), done_idx=idx, n_done=cnt)
        return [idx[:int(cnt.item())].sort().values]
    elif op == "step_none":
        e.step(None, seed=3, step=i)
    elif op == "step_feat":
        feat = torch.zeros((N, K, 17), **f32)
        e.step(e.sample_actions(3, i), features=feat)
        return [feat]
    elif op in ("slot", "slot_policy"):
        ac, rw, ns = torch.zeros((N, 4), **f32), torch.zeros(N, **f32), torch.zeros(N, **f32)
        fr = torch.zeros((N, 15), **f32)
        pol = e.sample_actions(5, i) * 1.5 if op == "slot_policy" else None
        e.step_rollout(3, i, actions=ac, rewards=rw, next_start=ns, policy_actions=pol, clip=pol is not None,
                       **({"next_frame": fr} if e.window else {"frame": fr}))
        return [ac, rw, ns]
    elif op == "rollout":
        bufs = [torch.zeros(s, **f32) for s in ((4, N, 15), (4, N, 4), (4, N), (3, N), (N,))]
        e.rollout_random(7, 100 * i, 4, *bufs)
        return bufs
    elif op == "set_obs":
        e.set_obs(e.obs.clone() * 0.5)
    elif op == "state":
        e.set_state(e.get_state())
    else:
        raise AssertionError(op)
    return []


def _drive(torch, kws, kinds):
    """Drive one handle per kws entry through OPS; kinds[j] names handle j's CALLS list (None: the
    contiguous handle has no feature windows). Handle 0 is the reference of the comparisons."""
    from f16_jsb_amd.env import F16Envs
    es = [F16Envs(N, stack_k=K, seed=SEED, max_steps=MAX_STEPS, **kw) for kw in kws]
    record = os.environ.get("F16_LAYOUT_RECORD")
    seen = {kind: [] for kind in kinds if kind}
    bad, terminal, finished = [], False, 0

    def same(what, i, xs):
        for j, x in enumerate(xs[1:], 1):
            if not (x.shape == xs[0].shape and torch.equal(x, xs[0])):
                bad.append("op %d (%s): %s of handle %d differs" % (i, OPS[i], what, j))

    for i, op in enumerate(OPS):
        extras = [_apply(e, op, i, torch) for e in es]
        for m in range(len(extras[0])):
            same("output %d" % m, i, [x[m] for x in extras])
        same("obs", i, [e.obs for e in es])
        for f in ("rew", "term", "trunc", "ep_len"):
            same(f, i, [getattr(e, f) for e in es])
        same("obs_features", i, [e.obs_features() for e in es])
        same("poses", i, [e.poses() for e in es])
        # the terminal observations of the lanes the last step finished: kept until an op rewrites
        # both windows (set_obs; rollout_random keeps none in the windowed layout) up to the next step
        if op in ("rollout", "set_obs"):
            terminal = False
        elif op not in ("reset", "masked_reset", "state"):
            terminal = True
        if terminal:
            done = (es[0].term | es[0].trunc) != 0
            same("terminal_obs", i, [e.terminal_obs[done] for e in es])
            finished += int(done.sum())
        for e, kind in zip(es, kinds):
            if kind:
                c = e.feature_window_calls
                got = [c["incremental"], c["full"], c["fused"]]
                if len(seen[kind]) == i:
                    seen[kind].append(got)
                elif seen[kind][i] != got:
                    bad.append("op %d (%s): feature_window_calls %s vs %s within kind %s" % (i, op, got, seen[kind][i], kind))
    for e in es:
        e.close()
    if record:
        prior = json.load(open(record)) if os.path.exists(record) else {}
        prior.update(seen)
        prior.setdefault("mismatches", []).extend(bad)
        with open(record, "w") as f:
            json.dump(prior, f)
        return
    assert not bad, "\n".join(bad)
    assert finished >= N, "every lane should have truncated and auto-reset at least once"
    for kind, got in seen.items():
        assert got == CALLS[kind], "feature_window_calls (%s) after each op:\n%s\nrecorded:\n%s" % (kind, got, CALLS[kind])


def test_layouts_agree_through_every_operation(gpu):
    import torch
    _drive(torch, [dict(obs_layout="contiguous"), dict(obs_layout="window", history=HIST, window_order="position"),
                   dict(obs_layout="window", history=HIST, window_order="env")], [None, "plain", "plain"])


def test_fused_handles_agree_with_plain_window(gpu):
    import torch
    w = dict(obs_layout="window", history=HIST)
    fused = dict(fused_features=True, fused_poses=True)
    _drive(torch, [dict(w, window_order="position"), dict(w, window_order="position", **fused),
                   dict(w, window_order="env", **fused)], ["plain", "fused", "fused"])
