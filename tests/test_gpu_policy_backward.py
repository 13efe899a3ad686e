"""GPU checks of the device policy's backward (f16env_policy_backward, DevicePolicy.backward_blob /
mean_and_value / evaluate_actions): exact integer gradients over the architecture matrix, tanh
nets against fp64 by the project's 4 x torch rule, determinism and graph replay, in-place inputs,
one PPO minibatch through autograd with an Adam step on the blob, and the edges."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import policy_grad_ref as G
import policy_ref
from f16_jsb_amd import abi

pytestmark = pytest.mark.gpu

MATRIX = policy_ref.MATRIX
N = 257


def _policy(net, gpu, k, d, activation="tanh", **kw):
    from f16_jsb_amd.policy import DevicePolicy
    pi, vf, act, val, ls = net
    t = lambda x: x.to(gpu)  # noqa: E731
    return DevicePolicy.from_layers([(t(w), t(b)) for w, b in pi], [(t(w), t(b)) for w, b in vf], (t(act[0]), t(act[1])),
                                    (t(val[0]), t(val[1])), t(ls), stack_k=k, frame_dim=d, activation=activation, **kw)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------
# 1. exact
@functools.lru_cache(maxsize=None)
def _int_case(name):
    """Case `name`'s integer data at n = 257 (rows [0, n) of it serve the smaller n) and, per n,
    the exact gradient packed into blob layout: made once, shared, not changed."""
    k, d, pi_w, vf_w, _ = MATRIX[name]
    net, obs, d_mean, d_values = G.int_data(k, d, pi_w, vf_w, N)
    desc = abi.policy_desc(k, d, pi_w, vf_w, "relu")
    refs = {}
    for n in (1, 129, 257):
        for which in ("both", "mean", "values"):
            dm = d_mean[:n].numpy() if which != "values" else None
            dv = d_values[:n].numpy() if which != "mean" else None
            refs[n, which] = G.pack(desc, G.int_vjp(net, obs[:n].numpy(), dm, dv)[0]).numpy()
    return net, obs, d_mean, d_values, refs


@pytest.mark.parametrize("name", list(MATRIX))
def test_exact_integer_gradient_over_the_matrix(gpu, name):
    """ReLU nets on integer data whose every float32 partial sum is exact in any order: grad_blob
    equals the integer reference element for element for n in {1, 129, 257} and max_blocks in
    {0, 1, 2} (1 and 2 at n = 257 send a wave through several row tiles and, by the case's waves per
    block, leave the last tile partial), pads and log_std slots have all bits zero, and a NULL
    d_mean / d_values zeroes exactly its branch."""
    k, d, pi_w, vf_w, _ = MATRIX[name]
    net, obs, d_mean, d_values, refs = _int_case(name)
    pol = _policy(net, gpu, k, d, "relu")
    u = policy_ref.unpack_blob(k, d, pi_w, vf_w, np.zeros(pol.n_floats, np.float32))
    ls = pol.offsets[abi.F16_POLICY_OFF_LOG_STD]
    pads = np.concatenate([u["zero"], np.arange(ls, ls + 4)])
    x, dm, dv = obs.to(gpu), d_mean.to(gpu), d_values.to(gpu)
    for n in (1, 129, 257):
        assert np.abs(refs[n, "both"]).max() > 0
        for max_blocks in (0, 1, 2):
            got = pol.backward_blob(x[:n], dm[:n], dv[:n], max_blocks=max_blocks).cpu().numpy()
            assert not np.isnan(got).any()
            assert np.array_equal(got, refs[n, "both"]), (n, max_blocks, int((got != refs[n, "both"]).sum()))
            assert np.all(got[pads].view(np.uint32) == 0), (n, max_blocks)
        only_mean = pol.backward_blob(x[:n], dm[:n], None, max_blocks=2).cpu().numpy()
        only_values = pol.backward_blob(x[:n], None, dv[:n], max_blocks=2).cpu().numpy()
        assert np.array_equal(only_mean, refs[n, "mean"]) and np.array_equal(only_values, refs[n, "values"])
        # exactly its branch: the other branch's pieces are all-bits zero, and the two add up
        assert np.all(only_mean.view(np.uint32)[refs[n, "mean"] == 0] == 0)
        assert np.all(only_values.view(np.uint32)[refs[n, "values"] == 0] == 0)
        assert np.array_equal(only_mean + only_values, refs[n, "both"])


# ---------------------------------------------------------------------------------------------
# 2. precision
@functools.lru_cache(maxsize=None)
def _tanh_case(name, seed=0):
    k, d, pi_w, vf_w, _ = MATRIX[name]
    net, obs, d_mean, d_values = G.tanh_data(k, d, pi_w, vf_w, N, seed)
    return net, obs, d_mean, d_values, G.vjp(net, obs, d_mean, d_values, "tanh"), \
        G.vjp(net, obs, d_mean, d_values, "tanh", torch.float32)


def _check_rule(label, got, ref64, t32):
    bad = []
    for name, (err, allow) in G.rule_of_four(got, ref64, t32).items():
        print("%s %s: kernel %.3e allowed %.3e ratio of torch's %.2f" % (label, name, err, allow, 4.0 * err / allow if allow else 0.0))
        if not err <= allow:
            bad.append((name, err, allow))
    return bad


@pytest.mark.parametrize("name", list(MATRIX))
def test_tanh_gradient_against_fp64_over_the_matrix(gpu, name):
    """Per parameter tensor, the kernel's max abs error against the fp64 vjp is at most 4 x that of
    torch CPU float32 autograd (floor 2^-24 max|reference|). Measured on an MI355X: DESIGN.md
    section 4."""
    from f16_jsb_amd.policy import unpack_blob
    k, d, pi_w, vf_w, _ = MATRIX[name]
    net, obs, d_mean, d_values, ref64, t32 = _tanh_case(name)
    pol = _policy(net, gpu, k, d)
    grad = pol.backward_blob(obs.to(gpu), d_mean.to(gpu), d_values.to(gpu))
    assert torch.isfinite(grad).all()
    bad = _check_rule("case " + name, unpack_blob(pol.desc, grad), ref64, t32)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 3. determinism
def test_same_bits_eager_graph_and_after_load(gpu):
    """Case C at n = 257 over the windowed observation of a stepped F16Envs: two calls give the
    same bits, a captured call replayed twice the same again, and after pol.load() of other
    weights the replay equals a fresh policy's gradient."""
    from f16_jsb_amd.env import F16Envs
    k, d, pi_w, vf_w, _ = MATRIX["C"]
    first, second = _tanh_case("C")[0], _tanh_case("C", 1)[0]
    _, _, d_mean, d_values = _tanh_case("C")[:4]
    dm, dv = d_mean.to(gpu), d_values.to(gpu)
    envs = F16Envs(N, stack_k=k, device=gpu, seed=3, obs_layout="window")
    try:
        envs.reset()
        for t in range(6):
            envs.step(envs.sample_actions(9, t))
        obs = envs.obs
        assert tuple(obs.shape) == (N, k, d) and not obs.is_contiguous()
        pol = _policy(first, gpu, k, d)
        a, b = pol.backward_blob(obs, dm, dv), pol.backward_blob(obs, dm, dv)
        assert np.array_equal(_bits(a), _bits(b)) and a.abs().max() > 0
        assert np.array_equal(_bits(a), _bits(pol.backward_blob(obs.contiguous(), dm, dv)))
        out = torch.zeros_like(a)
        pol.reserve_backward(N)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pol.backward_blob(obs, dm, dv, out=out)
        for _ in range(2):
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(_bits(out), _bits(a))
        pol.load(*_load_args(second, gpu))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        fresh = _policy(second, gpu, k, d).backward_blob(obs, dm, dv)
        assert np.array_equal(_bits(out), _bits(fresh)) and not np.array_equal(_bits(out), _bits(a))
    finally:
        envs.close()


def _load_args(net, gpu):
    pi, vf, act, val, ls = net
    t = lambda x: x.to(gpu)  # noqa: E731
    return ([(t(w), t(b)) for w, b in pi], [(t(w), t(b)) for w, b in vf], (t(act[0]), t(act[1])), (t(val[0]), t(val[1])),
            t(ls))


# ---------------------------------------------------------------------------------------------
# 4. in-place inputs
def test_feature_window_and_frame_broadcast_read_in_place(gpu):
    """Case G on the (n, K, 17) feature window of a stepped fused-features F16Envs and on a
    frame-broadcast (stride 0) view: each gives the bits of its contiguous copy."""
    from f16_jsb_amd.env import F16Envs
    k, d, pi_w, vf_w, _ = MATRIX["G"]
    net, obs, d_mean, d_values = _tanh_case("G")[:4]
    dm, dv = d_mean.to(gpu), d_values.to(gpu)
    pol = _policy(net, gpu, k, d)
    envs = F16Envs(N, stack_k=k, device=gpu, seed=3, obs_layout="window", fused_features=True)
    try:
        envs.reset()
        for t in range(6):
            envs.step(envs.sample_actions(9, t))
        feat = envs.obs_features()
        assert tuple(feat.shape) == (N, k, d) and not feat.is_contiguous() and feat.stride(2) == 1
        a, b = pol.backward_blob(feat, dm, dv), pol.backward_blob(feat.contiguous(), dm, dv)
        assert np.array_equal(_bits(a), _bits(b)) and torch.isfinite(a).all() and a.abs().max() > 0
    finally:
        envs.close()
    x = obs.to(gpu)
    frames = x[:, :1].expand(N, k, d)
    assert frames.stride(1) == 0
    c, e = pol.backward_blob(frames, dm, dv), pol.backward_blob(frames.contiguous(), dm, dv)
    assert np.array_equal(_bits(c), _bits(e)) and not np.array_equal(_bits(c), _bits(pol.backward_blob(x, dm, dv)))


# ---------------------------------------------------------------------------------------------
# 5. through autograd
def test_ppo_minibatch_through_autograd_and_one_adam_step(gpu):
    """Case E: a tiny rollout collected by the policy itself, GAE, one minibatch of 129, the PPO
    loss in the caller's torch. loss.backward() fills pol.blob.grad (log_std slots included), held
    to the 4 x rule against the fp64 autograd of the same loss on the same rows; then one clipped
    Adam step on the blob."""
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.policy import unpack_blob
    from f16_jsb_amd.rollout import DeviceRolloutBuffer, collect_rollout
    k, d, pi_w, vf_w, _ = MATRIX["E"]
    T, n_envs, B = 8, 64, 129
    net = G.tanh_data(k, d, pi_w, vf_w, 1, seed=3)[0]
    pol = _policy(net, gpu, k, d, seed=11)
    envs = F16Envs(n_envs, stack_k=k, device=gpu, seed=5, obs_layout="window")
    try:
        envs.reset()
        buf = DeviceRolloutBuffer(T, n_envs, k, gpu)
        last_v, last_d = collect_rollout(envs, buf, 7, 0, policy_fn=pol)
        buf.compute_returns_and_advantage(last_v, last_d)
        mb = next(iter(buf.get(B, generator=torch.Generator(device=gpu).manual_seed(1))))
    finally:
        envs.close()
    assert tuple(mb.observations.shape) == (B, k, d)

    def loss_of(dtype, device):
        p = G.as_params(net, dtype, device)
        c = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
        v, lp, ent = G.evaluate_actions(c(mb.observations), c(mb.actions), *p, "tanh")
        loss, ratio = G.ppo_loss(v, lp, ent, c(mb.advantages), c(mb.returns), c(mb.old_log_prob))
        loss.backward()
        return G.grads_of(p), ratio.detach()

    ref64, ratio = loss_of(torch.float64, "cpu")
    # the clip is discontinuous in the ratio: no row may sit at an edge (at unchanged weights it is 1)
    assert ((ratio - 0.8).abs() > 1e-4).all() and ((ratio - 1.2).abs() > 1e-4).all() and (ratio - 1).abs().max() < 1e-3
    t32, _ = loss_of(torch.float32, "cpu")

    pol.requires_grad_()
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4, eps=1e-5)
    v, lp, ent = pol.evaluate_actions(mb.observations, mb.actions)
    assert tuple(v.shape) == tuple(lp.shape) == tuple(ent.shape) == (B,)
    loss, _ = G.ppo_loss(v, lp, ent, mb.advantages, mb.returns, mb.old_log_prob)
    opt.zero_grad()
    loss.backward(retain_graph=True)
    grad = pol.blob.grad
    assert grad is not None and torch.isfinite(grad).all()
    got = unpack_blob(pol.desc, grad)
    assert got[4].abs().max() > 0  # log_std's gradient arrived through the slice
    bad = _check_rule("ppo loss", got, ref64, t32)
    assert not bad, bad

    zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, np.zeros(pol.n_floats, np.float32))["zero"]
    before = {key: t.clone() for key, t in pol.state_dict().items()}
    torch.nn.utils.clip_grad_norm_(pol.parameters(), 0.5)
    opt.step()
    after = pol.state_dict()
    assert set(after) == set(before) and all(not torch.equal(after[key], before[key]) for key in before)
    assert np.all(_bits(pol.blob)[zero] == 0)
    a, vals, lps = pol(mb.observations)
    assert torch.isfinite(a).all() and torch.isfinite(vals).all() and not torch.equal(vals, v.detach())
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()  # the blob moved under the graph: torch's version check, not a stale gradient


# ---------------------------------------------------------------------------------------------
# 6. edges
def test_edges(gpu):
    k, d, pi_w, vf_w, _ = MATRIX["G"]
    net, obs, d_mean, d_values = _tanh_case("G")[:4]
    pol = _policy(net, gpu, k, d)
    x, dm, dv = obs.to(gpu), d_mean.to(gpu), d_values.to(gpu)
    empty = pol.backward_blob(x[:0], dm[:0], dv[:0])
    assert tuple(empty.shape) == (pol.n_floats,) and np.all(_bits(empty) == 0)
    with pytest.raises(ValueError):
        pol.backward_blob(x, d_mean, dv)                       # a CPU d_mean
    with pytest.raises(ValueError):
        pol.backward_blob(x, dm.half(), dv)                    # float16
    shifted = torch.zeros(N * 4 + 1, device=gpu)[1:].reshape(N, 4)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    with pytest.raises(ValueError):
        pol.backward_blob(x, shifted, dv)                      # misaligned
    with pytest.raises(ValueError):
        pol.backward_blob(x, None, None)
    with pytest.raises(ValueError):
        pol.backward_blob(x.clone().requires_grad_(True), dm, dv)
    pol.requires_grad_()
    with pytest.raises(ValueError):
        pol.mean_and_value(x.clone().requires_grad_(True))
    # without grad mode it is just the forward; with it, an unused output's branch gets zero gradient
    with torch.no_grad():
        mean, values = pol.mean_and_value(x)
    assert not mean.requires_grad and torch.equal(mean, pol.predict(x)) and torch.equal(values, pol.value(x))
    mean, values = pol.mean_and_value(x)
    assert mean.requires_grad and values.requires_grad
    (values * dv).sum().backward()
    assert np.array_equal(_bits(pol.blob.grad), _bits(pol.backward_blob(x, None, dv)))
    torch.cuda.synchronize()
