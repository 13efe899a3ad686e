"""GPU checks of the device policy kernel (f16env_policy_forward / DevicePolicy): the operand
maps on exact integer data, the tanh net's error against fp64 next to torch's own float32
error, layout / batch invariance, the noise stream, bounds, validation and graph capture."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import policy_ref

pytestmark = pytest.mark.gpu


def _np_layers(layers):
    return [(w.detach().cpu().numpy(), b.detach().cpu().numpy()) for w, b in layers]


# ---------------------------------------------------------------------------------------------
# exact layout check: integer data, ReLU, eps = 0
def _int_net(rng, in_dim, pi_w, vf_w):
    def lin(o, i, density, lo, hi):
        w = rng.integers(lo, hi + 1, (o, i)) * (rng.random((o, i)) < density)
        return w.astype(np.int64), rng.integers(-3, 4, o).astype(np.int64)

    def branch(widths):
        out, fan_in = [], in_dim
        for l, w in enumerate(widths):
            out.append(lin(w, fan_in, 0.5 if l == 0 else 0.25, -1, 1))
            fan_in = w
        return out
    pi, vf = branch(pi_w), branch(vf_w)
    return pi, vf, lin(4, pi_w[-1], 1.0, -2, 2), lin(1, vf_w[-1], 1.0, -2, 2)


def _int_forward(x, layers, head):
    """Integer reference, and the largest sum of |terms| any output forms (every partial sum of
    any summation order is bounded by it)."""
    bound = 0
    for w, b in layers + [head]:
        bound = max(bound, int((np.abs(x) @ np.abs(w).T + np.abs(b)).max()))
        x = x @ w.T + b
        if w is not head[0]:
            x = np.maximum(x, 0)
    return x, bound


EXACT_CASES = [(n, k, 15, [64, 64], [64, 64]) for k in (1, 4) for n in (1, 31, 33, 64, 1000)] \
    + [(161, 10, 17, [32, 96, 64], [128, 64])]


@pytest.mark.parametrize("n,k,d,pi_w,vf_w", EXACT_CASES,
                         ids=["n%d-K%d-D%d-pi%d" % (c[0], c[1], c[2], len(c[3])) for c in EXACT_CASES])
def test_exact_integer_layout(gpu, n, k, d, pi_w, vf_w):
    """Asymmetric integer weights and inputs, every sum exact in float32: actions (= the mean at
    eps = 0) and values equal the integer reference bit for bit. A transposed operand, a wrong k
    permutation, a wrong accumulator row map or a mis-handled pad input fails here."""
    from f16_jsb_amd.policy import DevicePolicy
    rng = np.random.default_rng(1000 * k + n)
    pi, vf, act, val = _int_net(rng, k * d, pi_w, vf_w)
    x = rng.integers(-2, 3, (n, k, d)).astype(np.int64)
    mean, b1 = _int_forward(x.reshape(n, -1), pi, act)
    value, b2 = _int_forward(x.reshape(n, -1), vf, val)
    assert max(b1, b2) < 2 ** 24, "test data: a sum may not be exact in float32"
    assert np.abs(mean).max() > 0 and np.abs(value).max() > 0 and len(np.unique(mean)) >= min(4, n)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=gpu)  # noqa: E731
    pol = DevicePolicy.from_layers([(t(w), t(b)) for w, b in pi], [(t(w), t(b)) for w, b in vf],
                                   (t(act[0]), t(act[1])), (t(val[0]), t(val[1])), torch.zeros(4, device=gpu),
                                   stack_k=k, frame_dim=d, activation="relu")
    a, v, lp = pol(t(x), eps=torch.zeros((n, 4), device=gpu))
    assert np.array_equal(a.cpu().numpy(), mean.astype(np.float32))
    assert np.array_equal(v.cpu().numpy(), value[:, 0].astype(np.float32))
    assert np.abs(lp.cpu().numpy() - 4 * -0.9189385332046727).max() < 1e-6  # eps = 0, log_std = 0


# ---------------------------------------------------------------------------------------------
# the tanh net on stepped observations
N_ENVS, K = 1000, 4


@pytest.fixture(scope="module")
def world(gpu):
    """A stepped windowed F16Envs, bench.py's MlpActorCritic weights (CPU), the DevicePolicy on
    them, a fixed eps, and the fp64 reference: computed once, shared, left unchanged."""
    import bench
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.policy import DevicePolicy
    envs = F16Envs(N_ENVS, stack_k=K, device=gpu, seed=3, obs_layout="window")
    envs.reset()
    for t in range(6):
        envs.step(envs.sample_actions(9, t))
    obs = envs.obs
    assert not obs.is_contiguous() and obs.stride(2) == 1
    net = bench.MlpActorCritic(K * 15, "cpu", seed=1)
    net.log_std = torch.tensor([-0.5, 0.0, 0.25, 0.5])
    dev = lambda layers: [(w.to(gpu), b.to(gpu)) for w, b in layers]  # noqa: E731
    pol = DevicePolicy.from_layers(dev(net.pi), dev(net.vf), dev([net.act_w])[0], dev([net.val_w])[0],
                                   net.log_std.to(gpu), stack_k=K, seed=77)
    eps = torch.from_numpy(np.random.default_rng(8).standard_normal((N_ENVS, 4)).astype(np.float32))
    obs_cpu = obs.cpu()
    ref = policy_ref.forward(obs_cpu.numpy(), _np_layers(net.pi), _np_layers(net.vf), _np_layers([net.act_w])[0],
                             _np_layers([net.val_w])[0], net.log_std.numpy(), eps.numpy())
    yield {"envs": envs, "obs": obs, "obs_cpu": obs_cpu, "net": net, "pol": pol, "eps": eps.to(gpu),
           "eps_cpu": eps, "ref": ref, "out": tuple(x.clone() for x in pol(obs, eps=eps.to(gpu)))}
    envs.close()


@pytest.mark.parametrize("inputs", ["stepped", "unit"])
def test_tanh_net_error_against_fp64_within_4x_torch(world, inputs):
    """Kernel and torch are both float32 chains that differ in summation order and tanh; the
    kernel's max abs error against the fp64 reference is at most 4 x torch's (CPU float32), per
    output kind. "stepped": the observations of the stepped envs (positions of 1e3..1e4 saturate
    most first-layer units, and what is left is rounded on the grid of those large partial sums by
    both); "unit": standard-normal observations, where every tanh is in its curved range.
    Measured on an MI355X (kernel / torch): DESIGN.md section 4."""
    import math
    net, eps = world["net"], world["eps_cpu"]
    if inputs == "stepped":
        x, ref, out = world["obs_cpu"], world["ref"], world["out"]
    else:
        x = torch.from_numpy(np.random.default_rng(21).standard_normal((N_ENVS, K, 15)).astype(np.float32))
        ref = policy_ref.forward(x.numpy(), _np_layers(net.pi), _np_layers(net.vf), _np_layers([net.act_w])[0],
                                 _np_layers([net.val_w])[0], net.log_std.numpy(), eps.numpy())
        out = world["pol"](x.to(world["eps"].device), eps=world["eps"])
    flat = x.reshape(N_ENVS, -1)
    mean = torch.nn.functional.linear(net._mlp(flat, net.pi), *net.act_w)
    t_act = mean + net.log_std.exp() * eps
    t_val = net.value(x)
    t_lp = (-0.5 * eps * eps - net.log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    ref_a, ref_v, ref_lp, _ = ref
    got = [o.cpu().numpy().astype(np.float64) for o in out]
    bad = []
    for name, g, tt, r in (("actions", got[0], t_act, ref_a), ("values", got[1], t_val, ref_v),
                           ("log_probs", got[2], t_lp, ref_lp)):
        e_k = np.abs(g - r).max()
        e_t = np.abs(tt.numpy().astype(np.float64) - r).max()
        print("%s %s: kernel %.3e torch %.3e ratio %.2f" % (inputs, name, e_k, e_t, e_k / e_t if e_t else float("inf")))
        assert np.all(np.isfinite(g))
        if not e_k <= 4.0 * e_t:
            bad.append((name, e_k, e_t))
    assert not bad, bad


def test_in_place_window_equals_contiguous_copy(world):
    pol, obs = world["pol"], world["obs"]
    for kw in ({"eps": world["eps"]}, {"step": 3}):
        a = pol(obs, **kw)
        b = pol(obs.contiguous(), **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(pol(obs, eps=world["eps"]), world["out"]))


def test_batch_invariance(world):
    """Row i alone, in a batch of 33 and in the full batch: the same bits (the deferred and
    per-step bootstraps, and SB3's batch-of-one bootstrap, agree through this)."""
    pol, obs, eps, full = world["pol"], world["obs"], world["eps"], world["out"]
    for i in (0, 5, 31, 32, 500, N_ENVS - 1):
        one = pol(obs[i:i + 1], eps=eps[i:i + 1])
        assert all(torch.equal(o[0], f[i]) for o, f in zip(one, full)), i
        assert torch.equal(pol.value(obs[i:i + 1])[0], full[1][i])
        for s in {max(0, i - 32), max(0, min(i - 7, N_ENVS - 33)), min(i, N_ENVS - 33)}:
            part = pol(obs[s:s + 33], eps=eps[s:s + 33])
            assert all(torch.equal(o[i - s], f[i]) for o, f in zip(part, full)), (i, s)


def test_value_only_equals_full_forward(world):
    pol, obs = world["pol"], world["obs"]
    assert torch.equal(pol.value(obs), world["out"][1])
    assert torch.equal(pol.value(obs.contiguous()), world["out"][1])
    out = torch.empty(N_ENVS, device=obs.device)
    assert pol.value(obs, out=out) is out and torch.equal(out, world["out"][1])


def test_philox_normals(world, gpu):
    """Zero action head and log_std: the actions ARE eps. Within 1e-5 of the fp64 stream
    (|eps| <= 5.9 by construction: about 20 ulp), another draw per step and seed, and two shards
    with env_id_base 0 and n/2 reproduce the single run's rows."""
    from f16_jsb_amd.policy import DevicePolicy
    net, obs = world["net"], world["obs"]
    dev = lambda layers: [(w.to(gpu), b.to(gpu)) for w, b in layers]  # noqa: E731
    zero_head = (torch.zeros((4, 64), device=gpu), torch.zeros(4, device=gpu))

    def make(seed, base=0):
        return DevicePolicy.from_layers(dev(net.pi), dev(net.vf), zero_head, dev([net.val_w])[0],
                                        torch.zeros(4, device=gpu), stack_k=K, seed=seed, env_id_base=base)
    pol = make(1234)
    a, v, lp = pol(obs, step=7)
    want = policy_ref.policy_normals(1234, np.arange(N_ENVS), 7)
    got = a.cpu().numpy().astype(np.float64)
    assert np.abs(got - want).max() < 1e-5
    assert np.abs(lp.cpu().numpy() - policy_ref.log_prob_eps(want, np.zeros(4))).max() < 1e-4
    assert torch.equal(v, world["out"][1])
    a8 = pol(obs, step=8)[0]
    assert np.abs(a8.cpu().numpy() - policy_ref.policy_normals(1234, np.arange(N_ENVS), 8)).max() < 1e-5
    assert not torch.equal(a8, a) and not torch.equal(make(1235)(obs, step=7)[0], a)
    assert np.abs(pol(obs, step=(1 << 40) + 3)[0].cpu().numpy()
                  - policy_ref.policy_normals(1234, np.arange(N_ENVS), (1 << 40) + 3)).max() < 1e-5
    # the call counter is the default step
    p2 = make(1234)
    assert torch.equal(p2(obs)[0], pol(obs, step=0)[0]) and torch.equal(p2(obs)[0], pol(obs, step=1)[0])
    # shards
    h = N_ENVS // 2
    lo, hi = make(1234, 0)(obs[:h], step=7), make(1234, h)(obs[h:], step=7)
    for x, y, f in zip(lo, hi, (a, v, lp)):
        assert torch.equal(torch.cat([x, y]), f)


def test_deterministic_flag(world):
    pol, obs = world["pol"], world["obs"]
    zero = pol(obs, eps=torch.zeros_like(world["eps"]))
    det = pol(obs, deterministic=True)
    assert all(torch.equal(x, y) for x, y in zip(zero, det))
    assert torch.equal(pol.predict(obs), det[0]) and not torch.equal(det[0], world["out"][0])
    mean = world["ref"][3]
    assert np.abs(det[0].cpu().numpy() - mean).max() < 1e-5


def test_nothing_outside_the_rows_is_written(world, gpu):
    pol, n, pad, canary = world["pol"], 33, 8, -777.25
    acts = torch.full((n + 2 * pad, 4), canary, device=gpu)
    vals = torch.full((n + 2 * pad,), canary, device=gpu)
    lps = torch.full((n + 2 * pad,), canary, device=gpu)
    pol.forward_into(world["obs"][:n], 0, acts[pad:pad + n], vals[pad:pad + n], lps[pad:pad + n],
                     eps=world["eps"][:n])
    for buf, f in ((acts, world["out"][0]), (vals, world["out"][1]), (lps, world["out"][2])):
        assert torch.all(buf[:pad] == canary) and torch.all(buf[pad + n:] == canary)
        assert torch.equal(buf[pad:pad + n], f[:n])
    vals.fill_(canary)
    pol.value(world["obs"][:n], out=vals[pad:pad + n])
    assert torch.all(vals[:pad] == canary) and torch.all(vals[pad + n:] == canary)
    assert torch.equal(vals[pad:pad + n], world["out"][1][:n])


def test_validation(world, gpu):
    pol, obs = world["pol"], world["obs"]
    for bad in (world["obs_cpu"], obs.contiguous().half(), torch.zeros((8, K + 1, 15), device=gpu),
                torch.zeros((8, K, 30), device=gpu)[:, :, ::2], torch.zeros((8, K * 15), device=gpu), None):
        with pytest.raises(ValueError):
            pol(bad)
        with pytest.raises(ValueError):
            pol.value(bad)
    with pytest.raises(ValueError):
        pol(obs, eps=world["eps"][:5])
    with pytest.raises(ValueError):
        pol.forward_into(obs, 0, torch.zeros((N_ENVS, 4), device=gpu), torch.zeros(N_ENVS + 1, device=gpu),
                         torch.zeros(N_ENVS, device=gpu))


def test_graph_capture_replays_the_eager_result(world, gpu):
    pol, obs = world["pol"], world["obs"]
    eager = pol(obs, step=5)
    outs = (torch.zeros((N_ENVS, 4), device=gpu), torch.zeros(N_ENVS, device=gpu), torch.zeros(N_ENVS, device=gpu))
    vout = torch.zeros(N_ENVS, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pol.forward_into(obs, 5, *outs)
        pol.value(obs, out=vout)
    for o in outs + (vout,):
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(outs, eager))
    assert torch.equal(vout, eager[1])
