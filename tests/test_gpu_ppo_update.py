"""GPU checks of the device PPO update (f16env_ppo_loss_head, f16env_ppo_adam_step, DevicePPO): the
loss head against fp64 and torch's float32 autograd by the project's 4 x torch rule over the row
counts, grid limits and both advantage modes; the clipped Adam step alone on the smallest and the
largest blob; one whole update on a minibatch of a real rollout; a captured sampler + update
against eager updates bit for bit; and the edges. Measured on an MI355X: DESIGN.md section 4."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import policy_grad_ref as G
import policy_ref
import ppo_ref as P
from f16_jsb_amd import abi

pytestmark = pytest.mark.gpu

MATRIX = policy_ref.MATRIX
GUARD = 8  # doubles past the head's workspace that must stay as they were


def _policy(net, gpu, k, d, activation="tanh", **kw):
    from f16_jsb_amd.policy import DevicePolicy
    pi, vf, act, val, ls = net
    t = lambda x: x.to(gpu)  # noqa: E731
    return DevicePolicy.from_layers([(t(w), t(b)) for w, b in pi], [(t(w), t(b)) for w, b in vf], (t(act[0]), t(act[1])),
                                    (t(val[0]), t(val[1])), t(ls), stack_k=k, frame_dim=d, activation=activation, **kw)


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# 1. the head
HEAD_H = P.hyper(ent_coef=0.01, lr=0.0)


@functools.lru_cache(maxsize=None)
def _head_case(n, normalize):
    """The generator's rows and their references, made once, shared, not changed."""
    d = P.head_data(n)
    return d, P.head_autograd(d, HEAD_H, normalize, torch.float64), P.head_autograd(d, HEAD_H, normalize, torch.float32), \
        P.head_closed_form(d, HEAD_H, normalize)["clipped"]


def _run_head(gpu, d, max_blocks, normalize):
    """f16env_ppo_loss_head on the rows, then f16env_ppo_adam_step with lr = 0 over a blob of eight
    floats whose last four are log_std: (d_mean, d_values, d_log_std read from the gradient,
    stats[8])."""
    from f16_jsb_amd._lib import check, lib
    L = lib()
    n = d["values"].numel()
    t = {key: d[key].to(gpu) for key in ("mean", "values", "actions", "old_log_prob", "advantages", "returns")}
    blob = torch.zeros(8, device=gpu)
    blob[4:] = d["log_std"].to(gpu)
    before = blob.clone()
    hyper = P.hyper_tensor(HEAD_H, gpu)
    need, blocks = ctypes.c_int64(0), ctypes.c_int32(0)
    check(L.f16env_ppo_workspace(n, max_blocks, ctypes.byref(need)), "f16env_ppo_workspace")
    check(L.f16env_ppo_head_blocks(n, max_blocks, ctypes.byref(blocks)), "f16env_ppo_head_blocks")
    assert need.value == 8 * (4 + 8 * blocks.value) and blocks.value == min(-(-n // 256), max_blocks or 256)
    ws = torch.full((need.value // 8 + GUARD,), -7.0, dtype=torch.float64, device=gpu)
    d_mean, d_values = torch.full((n, 4), float("nan"), device=gpu), torch.full((n,), float("nan"), device=gpu)
    grad, m, v = torch.zeros(8, device=gpu), torch.zeros(8, device=gpu), torch.zeros(8, device=gpu)
    step, stats = torch.zeros(1, dtype=torch.int32, device=gpu), torch.full((8,), float("nan"), device=gpu)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    check(L.f16env_ppo_loss_head(stream, n, t["mean"].data_ptr(), t["values"].data_ptr(), t["actions"].data_ptr(),
                                 t["old_log_prob"].data_ptr(), t["advantages"].data_ptr(), t["returns"].data_ptr(),
                                 blob.data_ptr() + 16, hyper.data_ptr(), abi.F16_PPO_NORMALIZE_ADV if normalize else 0,
                                 max_blocks, ws.data_ptr(), need.value, d_mean.data_ptr(), d_values.data_ptr()),
          "f16env_ppo_loss_head")
    check(L.f16env_ppo_adam_step(stream, 8, blob.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(),
                                 hyper.data_ptr(), 4, ws.data_ptr(), blocks.value, stats.data_ptr()),
          "f16env_ppo_adam_step")
    torch.cuda.synchronize()
    assert (ws[-GUARD:] == -7.0).all() and ws[2].item() == n
    assert _same(blob, before) and int(step.item()) == 1 and (grad[:4] == 0).all()   # lr = 0: only the state moved
    return d_mean.cpu(), d_values.cpu(), grad[4:].cpu(), stats.cpu()


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("n", [1, 2, 129, 257, 1031])
def test_head_against_fp64_and_torch(gpu, n, normalize):
    """n = 1 (normalisation skipped), 2 (the smallest std), 129 (one block), 257 (one row into a
    second block), 1031 (a partial last block; with max_blocks 1 and 2 the blocks stride over the
    rows), each with max_blocks 0, 1, 2 and ent_coef 0.01: d_mean, d_values, d_log_std and every
    statistic within 4 x torch CPU float32 autograd's error against fp64 autograd; the clipped rows'
    d_mean equal to 0 and no other row's; clip_fraction equal to the reference's; two calls give
    the same bits."""
    d, ref64, t32, clipped = _head_case(n, normalize)
    bad = []
    for max_blocks in (0, 1, 2):
        d_mean, d_values, d_log_std, stats = _run_head(gpu, d, max_blocks, normalize)
        label = "n %d %s max_blocks %d " % (n, "normalized" if normalize else "raw", max_blocks)
        assert torch.isfinite(d_mean).all() and torch.isfinite(d_values).all() and torch.isfinite(stats).all()
        P.check(label + "d_mean", d_mean, ref64["d_mean"], t32["d_mean"], bad)
        P.check(label + "d_values", d_values, ref64["d_values"], t32["d_values"], bad)
        P.check(label + "d_log_std", d_log_std, ref64["d_log_std"], t32["d_log_std"], bad)
        for i, name in enumerate(P.STATS):
            P.check(label + name, stats[i:i + 1], ref64["stats"][i:i + 1], t32["stats"][i:i + 1], bad)
        assert (d_mean[clipped] == 0).all() and (d_mean[~clipped] != 0).all(dim=1).all()
        assert stats[5].item() == ref64["stats"][5].float().item()
        assert round(stats[5].item() * n) == int(((d["ratio64"] - 1).abs() > HEAD_H["clip_range"]).sum())
        norm = d_log_std.double().norm().item()
        assert abs(stats[6].item() - norm) <= 2.0 ** -23 * norm
        coef = min(1.0, HEAD_H["max_grad_norm"] / (stats[6].item() + 1e-6))
        assert abs(stats[7].item() - coef) <= 2.0 ** -22 * coef  # (one float32 sum and one division)
        again = _run_head(gpu, d, max_blocks, normalize)
        assert all(_same(a, b) for a, b in zip((d_mean, d_values, d_log_std, stats), again)), label
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 2. the step alone
@pytest.mark.parametrize("case", ["G", "F"])
def test_clipped_adam_step_alone(gpu, case):
    """The smallest and the largest blob of the matrix, three steps on random gradients (pads zero)
    whose norm is once below and twice above max_grad_norm: blob, exp_avg and exp_avg_sq per
    parameter tensor within 4 x torch CPU Adam's error against the fp64 reference fed the same
    gradients; the pads of all three all-bits zero; the gradient untouched; the step counter 3."""
    from f16_jsb_amd.policy import unpack_blob
    from f16_jsb_amd.ppo import DevicePPO
    k, d, pi_w, vf_w, _ = MATRIX[case]
    h = P.hyper()
    pol = _policy(G.tanh_data(k, d, pi_w, vf_w, 1, seed=1)[0], gpu, k, d)
    start = pol.blob.detach().cpu().clone()
    grads = P.adam_gradients(pol.desc, k, d, pi_w, vf_w, h)
    ref, t32 = P.adam_ref64(start, grads, h), P.adam_torch32(start, grads, h)
    zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, start.numpy())["zero"]
    ppo = DevicePPO(pol, max_batch=1)
    assert torch.equal(ppo.hyper.cpu(), P.hyper_tensor(h, "cpu"))
    bad = []
    for step, g in enumerate(grads):
        dev_g = g.to(gpu)
        version = pol.blob._version
        ppo.step_from(dev_g)
        assert pol.blob._version > version and _same(dev_g, g)
        stats = ppo.stats.cpu()
        norm = g.double().norm().item()
        assert abs(stats[6].item() - norm) <= 2.0 ** -23 * norm
        assert (stats[7].item() == 1.0) == (step == 0) and 0 < stats[7].item() <= 1.0
        for which, (name, got) in enumerate((("blob", pol.blob), ("exp_avg", ppo.exp_avg), ("exp_avg_sq", ppo.exp_avg_sq))):
            got = got.detach().cpu()
            assert torch.isfinite(got).all() and np.all(_bits(got)[zero] == 0), (step, name)
            rules = G.rule_of_four(unpack_blob(pol.desc, got), unpack_blob(pol.desc, ref[step][which]),
                                   unpack_blob(pol.desc, t32[step][which]))
            for tensor, (err, allow) in rules.items():
                print("case %s step %d %s %s: kernel %.3e allowed %.3e ratio of torch's %.2f"
                      % (case, step, name, tensor, err, allow, 4.0 * err / allow if allow else 0.0))
                if not err <= allow:
                    bad.append((step, name, tensor, err, allow))
    assert int(ppo.step.item()) == 3
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 3, 4. on a rollout
T_STEPS, N_ENVS, B = 8, 64, 129


def _rollout(gpu, pol, k):
    """A tiny rollout collected by the policy itself, with GAE: the full DeviceRolloutBuffer."""
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.rollout import DeviceRolloutBuffer, collect_rollout
    envs = F16Envs(N_ENVS, stack_k=k, device=gpu, seed=5, obs_layout="window")
    try:
        envs.reset()
        buf = DeviceRolloutBuffer(T_STEPS, N_ENVS, k, gpu)
        last_v, last_d = collect_rollout(envs, buf, 7, 0, policy_fn=pol)
        buf.compute_returns_and_advantage(last_v, last_d)
        torch.cuda.synchronize()
    finally:
        envs.close()
    return buf


def test_one_update_end_to_end(gpu):
    """Case E, a minibatch of 129 from a tiny rollout. ppo.grad (log_std slots included) is within
    the 4 x rule of the fp64 autograd of the whole loss; the new blob is within the rule of the fp64
    clip + Adam reference fed the kernel's own gradient; the blob's version advanced; the policy's
    output moved and is finite."""
    from f16_jsb_amd.policy import unpack_blob
    from f16_jsb_amd.ppo import DevicePPO
    k, d, pi_w, vf_w, _ = MATRIX["E"]
    net = G.tanh_data(k, d, pi_w, vf_w, 1, seed=3)[0]
    pol = _policy(net, gpu, k, d, seed=11)
    buf = _rollout(gpu, pol, k)
    mb = next(iter(buf.get(B, generator=torch.Generator(device=gpu).manual_seed(1))))
    assert tuple(mb.observations.shape) == (B, k, d)
    h = P.hyper(ent_coef=0.01)

    def loss_of(dtype):
        p = G.as_params(net, dtype, "cpu")
        c = lambda t: t.to(device="cpu", dtype=dtype)  # noqa: E731
        v, lp, ent = G.evaluate_actions(c(mb.observations), c(mb.actions), *p, "tanh")
        loss, ratio = G.ppo_loss(v, lp, ent, c(mb.advantages), c(mb.returns), c(mb.old_log_prob), h["clip_range"],
                                 h["ent_coef"], h["vf_coef"])
        loss.backward()
        return G.grads_of(p), ratio.detach(), loss.item()

    ref64, ratio, loss64 = loss_of(torch.float64)
    # the clip is discontinuous in the ratio: no row may sit at an edge (at unchanged weights it is 1)
    assert ((ratio - 0.8).abs() > 1e-4).all() and ((ratio - 1.2).abs() > 1e-4).all() and (ratio - 1).abs().max() < 1e-3
    t32, _, loss32 = loss_of(torch.float32)

    ppo = DevicePPO(pol, ent_coef=0.01, max_batch=B)
    start, version = pol.blob.detach().clone(), pol.blob._version
    a0, v0, _ = pol(mb.observations, step=0)
    ppo.update(mb)
    assert pol.blob._version > version and int(ppo.step.item()) == 1
    grad = ppo.grad.clone()
    assert torch.isfinite(grad).all()
    got = unpack_blob(pol.desc, grad)
    assert got[4].abs().max() > 0  # log_std's gradient was written by the step's prologue
    bad = []
    for name, (err, allow) in G.rule_of_four(got, ref64, t32).items():
        print("ppo.grad %s: kernel %.3e allowed %.3e ratio of torch's %.2f" % (name, err, allow, 4.0 * err / allow if allow else 0.0))
        if not err <= allow:
            bad.append(("grad", name, err, allow))
    stats = ppo.stats.cpu()
    print("loss: kernel %.9g torch float32 %.9g fp64 %.12g" % (stats[3].item(), loss32, loss64))
    # every ratio is within 1e-3 of 1: nothing is clipped, and approx_kl <= (1e-3)^2 / 2 plus the ratio's rounding
    assert stats[5].item() == 0.0 and abs(stats[4].item()) < 1e-6 and torch.isfinite(stats).all()
    ref, t32a = P.adam_ref64(start, [grad], h)[0], P.adam_torch32(start, [grad], h)[0]
    for which, (name, now) in enumerate((("blob", pol.blob), ("exp_avg", ppo.exp_avg), ("exp_avg_sq", ppo.exp_avg_sq))):
        rules = G.rule_of_four(unpack_blob(pol.desc, now.detach()), unpack_blob(pol.desc, ref[which]),
                               unpack_blob(pol.desc, t32a[which]))
        for tensor, (err, allow) in rules.items():
            print("%s %s: kernel %.3e allowed %.3e ratio of torch's %.2f" % (name, tensor, err, allow, 4.0 * err / allow if allow else 0.0))
            if not err <= allow:
                bad.append((name, tensor, err, allow))
    assert not bad, bad
    zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, np.zeros(pol.n_floats, np.float32))["zero"]
    assert np.all(_bits(pol.blob)[zero] == 0) and not torch.equal(pol.blob.detach(), start)
    a1, v1, _ = pol(mb.observations, step=0)
    assert torch.isfinite(a1).all() and torch.isfinite(v1).all() and not torch.equal(v1, v0) and not torch.equal(a1, a0)
    # the six tensors instead of the tuple, and train()'s loops: two passes of four minibatches
    ppo.update(*mb)
    assert int(ppo.step.item()) == 2
    assert ppo.train(buf, 2, 128, generator=torch.Generator(device=gpu).manual_seed(2)) == 8
    assert int(ppo.step.item()) == 10 and torch.isfinite(pol.blob).all() and torch.isfinite(ppo.stats).all()
    sd = ppo.state_dict()
    other = DevicePPO(_policy(net, gpu, k, d), max_batch=1).load_state_dict(sd)
    assert all(_same(getattr(other, key), getattr(ppo, key)) for key in ("exp_avg", "exp_avg_sq", "step", "hyper"))


def test_captured_sampler_and_update_equal_eager_updates(gpu):
    """rollout_minibatch(view, idx, out=samples) + ppo.update(samples) captured once and replayed
    three times with idx overwritten in place equals three eager updates from the same start bit for
    bit, in blob, moments, step counter and stats. After set_hyper(lr=0) a replay leaves the blob
    as it is while the moments and the step counter still move."""
    from f16_jsb_amd.ppo import DevicePPO
    from f16_jsb_amd.rollout import RolloutSamples, _View, rollout_minibatch
    k, d, pi_w, vf_w, _ = MATRIX["E"]
    net = G.tanh_data(k, d, pi_w, vf_w, 1, seed=3)[0]
    buf = _rollout(gpu, _policy(net, gpu, k, d, seed=11), k)
    view = _View(buf)
    perm = torch.randperm(T_STEPS * N_ENVS, generator=torch.Generator().manual_seed(4))
    batches = [perm[i * B:(i + 1) * B].to(gpu) for i in range(3)]
    e = lambda *s: torch.empty(s, dtype=torch.float32, device=gpu)  # noqa: E731
    new_samples = lambda: RolloutSamples(e(B, k, d), e(B, 4), e(B), e(B), e(B), e(B))  # noqa: E731
    state = lambda pol, ppo: [x.detach().clone() for x in (pol.blob, ppo.exp_avg, ppo.exp_avg_sq, ppo.step, ppo.stats)]  # noqa: E731

    pol_e = _policy(net, gpu, k, d)
    ppo_e = DevicePPO(pol_e, ent_coef=0.01, max_batch=B)
    samples_e, eager = new_samples(), []
    for idx in batches:
        rollout_minibatch(view, idx, out=samples_e)
        ppo_e.update(samples_e)
        eager.append(state(pol_e, ppo_e))
    torch.cuda.synchronize()
    assert not _same(eager[0][0], eager[1][0]) and not _same(eager[1][0], eager[2][0])

    pol_g = _policy(net, gpu, k, d)
    ppo_g = DevicePPO(pol_g, ent_coef=0.01, max_batch=B)
    samples_g, idx = new_samples(), batches[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rollout_minibatch(view, idx, out=samples_g)
        ppo_g.update(samples_g)
    assert int(ppo_g.step.item()) == 0  # (the capture ran nothing)
    for i, batch in enumerate(batches):
        idx.copy_(batch)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(("blob", "exp_avg", "exp_avg_sq", "step", "stats"), state(pol_g, ppo_g), eager[i]):
            assert _same(a, b), (i, name)
    ppo_g.set_hyper(lr=0.0)
    before = state(pol_g, ppo_g)
    graph.replay()
    torch.cuda.synchronize()
    after = state(pol_g, ppo_g)
    assert _same(after[0], before[0]) and not _same(after[1], before[1]) and not _same(after[2], before[2])
    assert int(after[3].item()) == 4


# ---------------------------------------------------------------------------------------------
# 5. edges
def test_edges(gpu):
    from f16_jsb_amd.ppo import DevicePPO
    k, d, pi_w, vf_w, _ = MATRIX["G"]
    net, obs = G.tanh_data(k, d, pi_w, vf_w, 8)[:2]
    pol = _policy(net, gpu, k, d)
    ppo = DevicePPO(pol, max_batch=4)
    hd = P.head_data(8)
    x = obs.to(gpu)
    good = [x] + [hd[key].to(gpu) for key in ("actions", "values", "old_log_prob", "advantages", "returns")]

    def swapped(i, t):
        a = list(good)
        a[i] = t
        return a
    with pytest.raises(ValueError):
        ppo.update(*swapped(1, hd["actions"]))                        # a CPU tensor
    with pytest.raises(ValueError):
        ppo.update(*swapped(4, good[4].half()))                       # float16
    shifted = torch.zeros(8 * 4 + 1, device=gpu)[1:].reshape(8, 4)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    with pytest.raises(ValueError):
        ppo.update(*swapped(1, shifted))                              # misaligned actions
    with pytest.raises(ValueError):
        ppo.update(*swapped(5, good[5][:7]))                          # a short tensor
    with pytest.raises(ValueError):
        ppo.step_from(torch.zeros(pol.n_floats - 1, device=gpu))
    with pytest.raises(ValueError):
        ppo.set_hyper(learning_rate=1.0)
    start = pol.blob.detach().clone()
    ppo.update(*[t[:0] for t in good])                                # n == 0: nothing moves
    torch.cuda.synchronize()
    assert int(ppo.step.item()) == 0 and _same(pol.blob, start) and (ppo.exp_avg == 0).all() and ppo.max_batch == 4
    # inside a capture the buffers cannot grow: 8 rows where 4 are reserved raise, 4 rows are captured
    ppo.update(*[t[:4] for t in good])                                # (outside: every kernel has run once)
    torch.cuda.synchronize()
    four = [t[:4].clone() for t in good]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ppo.update(*four)
        with pytest.raises(RuntimeError, match="stream capture"):
            ppo.update(*good)
    graph.replay()
    torch.cuda.synchronize()
    assert int(ppo.step.item()) == 2 and ppo.max_batch == 4
    ppo.update(*good)                                                 # outside a capture they grow
    torch.cuda.synchronize()
    assert ppo.max_batch == 8 and int(ppo.step.item()) == 3 and torch.isfinite(pol.blob).all()
