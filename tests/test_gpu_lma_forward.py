"""GPU checks of the device LMA policy (f16env_policy_lma_forward / DeviceLMAPolicy) over the case
matrix of tests/lma_ref.py: the exact integer layout, every case against the fp64 restatement by
the project's 4 x torch rule, batch invariance, non-finite rows, the flags, the noise stream,
graphs and streams, and collect_rollout's fast path with the deferred bootstrap.
Measured ratios: profiles/lma_forward_precision.json, DESIGN.md section 4."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import lma_ref

pytestmark = pytest.mark.gpu

MATRIX = lma_ref.MATRIX
N_ROWS = 257
RPB = lma_ref.ROWS_PER_BLOCK   # (the block's four waves share its 32 rows: a wave's rows are the block's)
KINDS = ("features", "actions", "values", "log_probs")


def _reaches(name, matrix=MATRIX):
    """The case, after asserting the kernel instance DESIGN section 4's rule gives it."""
    k, d, nl, ff, pi_w, vf_w, act, hs, inst = matrix[name]
    assert lma_ref.kernel_instance(k, d, nl, ff, pi_w, vf_w) == inst, name
    return k, d, act, hs


def _args(net, gpu):
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=gpu)  # noqa: E731
    pair = lambda wb: (t(wb[0]), t(wb[1]))  # noqa: E731
    ext = {"embed": pair(net["embed"]), "embed2": pair(net["embed2"]),
           "blocks": [{k: pair(v) for k, v in blk.items()} for blk in net["blocks"]]}
    return ext, [pair(l) for l in net["pi"]], [pair(l) for l in net["vf"]], pair(net["act"]), pair(net["val"]), t(net["log_std"])


def _policy(net, gpu, k, d, act="tanh", hs=4, **kw):
    from f16_jsb_amd.lma_policy import DeviceLMAPolicy
    return DeviceLMAPolicy.from_layers(*_args(net, gpu), stack_k=k, frame_dim=d, activation=act, heads_stacking=hs, **kw)


def _cpu(out):
    return [o.cpu().numpy() for o in out]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """257 standard-normal rows and a fixed eps for a case: made once, shared, not changed."""
    k, d = MATRIX[name][:2]
    rng = np.random.default_rng(900 + sum(map(ord, name)))
    return rng.standard_normal((N_ROWS, k, d)).astype(np.float32), rng.standard_normal((N_ROWS, 4)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _net(name, seed=0):
    return lma_ref.random_net(name, seed)


# ---------------------------------------------------------------------------------------------
# (a) exact integer layout: stages 2-4, the k-step map of W_2 and the MLP fan-in
EXACT = {"W3": (3, 17, 0, 128, [64], [64], "relu", 4, (17, 79488)),
         "W10": (10, 17, 0, 128, [64], [64], "relu", 4, (17, 95872))}


def _int_case(name):
    k = EXACT[name][0]
    rng = np.random.default_rng(40 + k)
    L, C = lma_ref.new_dims(k)

    def sparse(o, i, keep):
        return (rng.integers(-1, 2, (o, i)) * (rng.random((o, i)) < keep)).astype(np.int64)
    net = {"embed": (sparse(64, 17, 0.5), rng.integers(-2, 3, 64)), "embed2": (sparse(32, C, 0.2), rng.integers(-2, 3, 32)),
           "blocks": [], "pi": [(sparse(64, L * 32, 0.2), rng.integers(-2, 3, 64))],
           "vf": [(sparse(64, L * 32, 0.2), rng.integers(-2, 3, 64))], "act": (sparse(4, 64, 0.3), rng.integers(-2, 3, 4)),
           "val": (sparse(1, 64, 0.3), rng.integers(-2, 3, 1)), "log_std": np.zeros(4)}
    pe = rng.integers(-2, 3, (k, 64))
    return net, pe


def _int_forward(net, pe, x, hs=4):
    """The integer network in int64, and the largest sum of magnitudes any output met."""
    n, k, _ = x.shape
    L, C = lma_ref.new_dims(k)
    bound = [0]

    def lin(h, wb):
        bound[0] = max(bound[0], int((np.abs(h) @ np.abs(wb[0]).T + np.abs(wb[1])).max()))
        return h @ wb[0].T + wb[1]
    y = np.maximum(lin(x, net["embed"]), 0) + pe
    flat = np.zeros((n, k * 64), np.int64)
    flat[:, lma_ref.flat_index(k, 64, hs).reshape(-1)] = y.reshape(n, -1)
    f = np.maximum(lin(flat.reshape(n, L, C), net["embed2"]), 0).reshape(n, -1)
    mean = lin(np.maximum(lin(f, net["pi"][0]), 0), net["act"])
    value = lin(np.maximum(lin(f, net["vf"][0]), 0), net["val"])[:, 0]
    return f, mean, value, bound[0]


@pytest.mark.parametrize("n", [1, RPB + 1, 2 * RPB + 1])
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_integer_layout(gpu, name, n):
    """Integer weights, an integer PE table and integer (K, 17) inputs under ReLU, no block: every
    sum is exact in float32, so features, means and values equal the integer reference bit for
    bit. n = 1; one row alone in a second block; a third block whose waves have one live row."""
    k, d, act, hs = _reaches(name, EXACT)
    net, pe = _int_case(name)
    x = np.random.default_rng(n).integers(-2, 3, (n, k, d)).astype(np.int64)
    f, mean, value, bound = _int_forward(net, pe, x)
    assert bound < 2 ** 24, "test data: a sum may not be exact in float32"
    assert np.abs(f).max() > 0 and np.abs(mean).max() > 0 and np.abs(value).max() > 0
    pol = _policy(net, gpu, k, d, act, hs, pe=torch.as_tensor(pe.astype(np.float32)))
    a, v, lp, feats = pol.forward_with_features(torch.as_tensor(x.astype(np.float32), device=gpu), 0,
                                                eps=torch.zeros((n, 4), device=gpu))
    assert np.array_equal(feats.cpu().numpy(), f.astype(np.float32))
    assert np.array_equal(a.cpu().numpy(), mean.astype(np.float32))
    assert np.array_equal(v.cpu().numpy(), value.astype(np.float32))
    assert torch.equal(pol.extract_features(torch.as_tensor(x.astype(np.float32), device=gpu)), feats)


# ---------------------------------------------------------------------------------------------
# (b) precision: every case against fp64 by the 4 x torch rule
def precision(label, got, net, x, eps, act, hs, rows=None):
    """Per output kind (kernel error, torch CPU float32 error, floor, ratio) against the fp64
    restatement, and the kinds beyond 4 x max(torch, 2^-24 max|reference|). Prints every figure."""
    ref = lma_ref.forward(net, x, eps, torch.float64, act, hs)
    t32 = lma_ref.forward(net, x, eps, torch.float32, act, hs)
    figures, bad = {}, []
    for kind, g, tt, r in zip(KINDS, got, t32, ref):
        g, tt = np.asarray(g, np.float64), np.asarray(tt, np.float64)
        if rows is not None:
            g, tt, r = g[rows], tt[rows], r[rows]
        e_k, e_t, floor = np.abs(g - r).max(), np.abs(tt - r).max(), 2.0 ** -24 * np.abs(r).max()
        ratio = e_k / max(e_t, floor)
        figures[kind] = {"kernel": float(e_k), "torch": float(e_t), "floor": float(floor), "ratio": float(ratio)}
        print("%s %s: kernel %.3e torch %.3e floor %.3e ratio %.2f" % (label, kind, e_k, e_t, floor, ratio))
        if not (np.all(np.isfinite(g)) and e_k <= 4.0 * max(e_t, floor)):
            bad.append((kind, e_k, e_t, floor))
    return figures, bad


def run_case(name, gpu, x=None):
    """The case's kernel outputs (features, actions, values, log_probs) on its shared inputs."""
    k, d, act, hs = _reaches(name)
    xs, eps = _inputs(name)
    x = xs if x is None else x
    a, v, lp, f = _policy(_net(name), gpu, k, d, act, hs).forward_with_features(
        torch.from_numpy(x).to(gpu), 0, eps=torch.from_numpy(eps).to(gpu))
    return _cpu((f, a, v, lp)), x, eps, act, hs


@pytest.mark.parametrize("name", list(MATRIX))
def test_random_net_against_fp64_over_the_matrix(gpu, name):
    got, x, eps, act, hs = run_case(name, gpu)
    _, bad = precision("case " + name, got, _net(name), x, eps, act, hs)
    assert not bad, bad


@pytest.fixture(scope="module")
def stepped(gpu):
    """The frame window (257, 10, 15) of a stepped windowed F16Envs, read in place."""
    from f16_jsb_amd.env import F16Envs
    envs = F16Envs(N_ROWS, stack_k=10, device=gpu, seed=3, obs_layout="window")
    envs.reset()
    for t in range(12):
        envs.step(envs.sample_actions(9, t))
    obs = envs.obs
    assert tuple(obs.shape) == (N_ROWS, 10, 15) and not obs.is_contiguous() and obs.stride(2) == 1
    yield obs
    envs.close()


def test_case_r_on_stepped_observations(gpu, stepped):
    """Case R on the observations of a stepped env, read in place: the rule holds there too, the
    in-place view gives the bits of its contiguous copy, and the (n, K, 17) input form gives the
    bits of the raw frames when the features are f16env_features' of the same observations."""
    from f16_jsb_amd.features import features
    k, d, act, hs = _reaches("R")
    eps = torch.from_numpy(_inputs("R")[1]).to(gpu)
    pol = _policy(_net("R"), gpu, k, d, act, hs)
    a, v, lp, f = pol.forward_with_features(stepped, 0, eps=eps)
    _, bad = precision("case R stepped", _cpu((f, a, v, lp)), _net("R"), stepped.cpu().numpy(), eps.cpu().numpy(), act, hs)
    assert not bad, bad
    again = pol.forward_with_features(stepped.contiguous(), 0, eps=eps)
    assert all(torch.equal(p, q) for p, q in zip((a, v, lp, f), again))
    k17, d17, act17, hs17 = _reaches("R17")
    pol17 = _policy(_net("R"), gpu, k17, d17, act17, hs17)
    feat = features(stepped)
    assert tuple(feat.shape) == (N_ROWS, 10, 17)
    out17 = pol17.forward_with_features(feat, 0, eps=eps)
    assert all(torch.equal(p, q) for p, q in zip((a, v, lp, f), out17))


def test_from_state_dict_reproduces_the_restatement(gpu):
    """A state dict under the reference's key names (random tensors of the right shapes, the
    aliases of the shared extractor included) loads and meets the rule."""
    from f16_jsb_amd.lma_policy import DeviceLMAPolicy
    from test_lma_cpu import _state_dict
    k, d, act, hs = _reaches("R")
    net = _net("R", 1)
    x, eps = _inputs("R")
    pol = DeviceLMAPolicy.from_state_dict(_state_dict(net), stack_k=k, frame_dim=d, device=gpu)
    a, v, lp, f = pol.forward_with_features(torch.from_numpy(x).to(gpu), 0, eps=torch.from_numpy(eps).to(gpu))
    _, bad = precision("state dict R", _cpu((f, a, v, lp)), net, x, eps, act, hs)
    assert not bad, bad
    back = pol.state_dict()
    assert torch.equal(back["pi_features_extractor.lma_extractor.lma_blocks.1.attn.c_attn.weight"].cpu(),
                       torch.from_numpy(net["blocks"][1]["attn.c_attn"][0]))


# ---------------------------------------------------------------------------------------------
# (c) rows do not see each other
@pytest.fixture(scope="module")
def world(gpu):
    k, d, act, hs = _reaches("R")
    x, eps = _inputs("R")
    pol = _policy(_net("R"), gpu, k, d, act, hs, seed=77)
    x, eps = torch.from_numpy(x).to(gpu), torch.from_numpy(eps).to(gpu)
    a, v, lp, f = pol.forward_with_features(x, 0, eps=eps)
    return {"pol": pol, "x": x, "eps": eps, "out": (a, v, lp), "features": f}


def test_batch_invariance(world):
    """A row alone, in a batch of 33 and in the full batch: the same bits."""
    pol, x, eps, full, feats = world["pol"], world["x"], world["eps"], world["out"], world["features"]
    for i in (0, 5, 31, 32, 200, N_ROWS - 1):
        one = pol(x[i:i + 1], eps=eps[i:i + 1])
        assert all(torch.equal(o[0], f[i]) for o, f in zip(one, full)), i
        assert torch.equal(pol.value(x[i:i + 1])[0], full[1][i])
        assert torch.equal(pol.extract_features(x[i:i + 1])[0], feats[i])
        for s in {max(0, i - 32), max(0, min(i - 7, N_ROWS - 33)), min(i, N_ROWS - 33)}:
            part = pol(x[s:s + 33], eps=eps[s:s + 33])
            assert all(torch.equal(o[i - s], f[i]) for o, f in zip(part, full)), (i, s)


def test_non_finite_rows_stay_in_their_rows(world):
    """A NaN row, a +inf row and a -inf row (the last alone in its wave) leave every other row's
    bits unchanged; the NaN row's outputs are NaN."""
    pol, eps, full, feats = world["pol"], world["eps"], world["out"], world["features"]
    dirty = world["x"].clone()
    dirty[5, 2, 7], dirty[40, 1, 3], dirty[N_ROWS - 1, 9, 14] = float("nan"), float("inf"), float("-inf")
    touched = np.array([5, 40, N_ROWS - 1])
    others = np.setdiff1d(np.arange(N_ROWS), touched)
    a, v, lp, f = pol.forward_with_features(dirty, 0, eps=eps)
    for clean, got in zip(_cpu(full) + _cpu([feats]), _cpu((a, v, lp, f))):
        assert np.all(np.isfinite(clean))
        assert np.array_equal(_bits(clean[others]), _bits(got[others]))
    assert torch.equal(lp, full[2])  # log-probs do not read obs
    assert torch.isnan(a[5]).all() and torch.isnan(v[5]) and torch.isnan(f[5]).all()


def test_value_only_and_deterministic_flags(world):
    pol, x, eps, full = world["pol"], world["x"], world["eps"], world["out"]
    assert torch.equal(pol.value(x), full[1])
    out = torch.empty(N_ROWS, device=x.device)
    assert pol.value(x, out=out) is out and torch.equal(out, full[1])
    zero = pol(x, eps=torch.zeros_like(eps))
    det = pol(x, deterministic=True)
    assert all(torch.equal(p, q) for p, q in zip(zero, det))
    assert torch.equal(pol.predict(x), det[0]) and not torch.equal(det[0], full[0])
    assert torch.equal(det[1], full[1])
    assert torch.equal(pol.extract_features(x), world["features"])
    empty = pol(x[:0])
    assert [tuple(o.shape) for o in empty] == [(0, 4), (0,), (0,)] and tuple(pol.extract_features(x[:0]).shape) == (0, 160)


def test_noise_stream_is_the_device_policys(gpu, world):
    """Zero action heads and log_std make the actions the drawn eps: DeviceLMAPolicy and
    DevicePolicy draw the same bits for the same (seed, step, env_id_base)."""
    from f16_jsb_amd.policy import DevicePolicy
    k, d, act, hs = _reaches("R")
    net = dict(_net("R"))
    net["act"] = (np.zeros((4, 64), np.float32), np.zeros(4, np.float32))
    net["log_std"] = np.zeros(4, np.float32)
    base, seed, step = (1 << 33) + 5, 4321, (1 << 40) + 3
    lma = _policy(net, gpu, k, d, act, hs, seed=seed, env_id_base=base)
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
    mlp = DevicePolicy.from_layers([(z(32, k * d), z(32))], [(z(32, k * d), z(32))], (z(4, 32), z(4)), (z(1, 32), z(1)), z(4),
                                   stack_k=k, frame_dim=d, seed=seed, env_id_base=base)
    a, _, lp = lma(world["x"], step=step)
    b, _, lq = mlp(world["x"], step=step)
    assert torch.equal(a, b) and torch.equal(lp, lq) and float(a.abs().max()) > 1.0
    assert not torch.equal(lma(world["x"], step=step + 1)[0], a)


# ---------------------------------------------------------------------------------------------
# (d) graphs and streams
def test_graph_replay_follows_load_and_side_stream(gpu, stepped):
    k, d, act, hs = _reaches("R")
    first, second = _net("R"), _net("R", 1)
    obs, n = stepped, N_ROWS
    pol = _policy(first, gpu, k, d, act, hs, seed=5)
    eager = pol(obs, step=5)
    outs = (torch.zeros((n, 4), device=gpu), torch.zeros(n, device=gpu), torch.zeros(n, device=gpu))
    vout = torch.zeros(n, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pol.forward_into(obs, 5, *outs)
        pol.value(obs, out=vout)
    for o in outs + (vout,):
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(outs, eager)) and torch.equal(vout, eager[1])
    ptr = pol.blob.data_ptr()
    pol.load(*_args(second, gpu))
    assert pol.blob.data_ptr() == ptr
    for o in outs + (vout,):
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    fresh = _policy(second, gpu, k, d, act, hs, seed=5)(obs, step=5)
    assert all(torch.equal(p, q) for p, q in zip(outs, fresh)) and torch.equal(vout, fresh[1])
    assert not torch.equal(outs[1], eager[1])
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        got = pol(obs, step=5)
        v = pol.value(obs)
    side.synchronize()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(got, fresh)) and torch.equal(v, fresh[1])


# ---------------------------------------------------------------------------------------------
# (e) the rollout loop
def test_collect_rollout_fast_path_and_deferred_bootstrap(gpu):
    """collect_rollout(envs, buf, policy_fn=pol) with case R on a windowed F16Envs, 256 envs, 16
    steps, TimeLimit 5 (every lane truncates three times, so the deferred bootstrap runs): the
    buffers equal those of the same policy driven through a closure on the generic path, and the
    deferred bootstrap equals the per-step one, bit for bit."""
    from f16_jsb_amd.env import F16Envs
    from f16_jsb_amd.rollout import DeviceRolloutBuffer, collect_rollout
    k, d, act, hs = _reaches("R")
    n, T = 256, 16
    fields = ("frames", "actions", "rewards", "episode_starts", "values", "log_probs")
    runs = {}
    for mode in ("fast", "closure", "per_step"):
        pol = _policy(_net("R"), gpu, k, d, act, hs, seed=11)
        envs = F16Envs(n, stack_k=k, device=gpu, seed=61, max_steps=5, obs_layout="window")
        try:
            envs.reset()
            buf = DeviceRolloutBuffer(T, n, k, gpu)
            if mode == "closure":
                lv, ld = collect_rollout(envs, buf, seed=3, policy_fn=lambda o: pol(o), value_fn=pol.value)
            else:
                lv, ld = collect_rollout(envs, buf, seed=3, policy_fn=pol,
                                         bootstrap="per_step" if mode == "per_step" else "deferred")
            runs[mode] = {f: getattr(buf, f).clone() for f in fields}
            runs[mode]["last_v"], runs[mode]["last_d"] = lv.clone(), ld.clone()
        finally:
            envs.close()
    fast = runs["fast"]
    assert int((fast["episode_starts"][1:] > 0).sum()) >= 2 * n and torch.isfinite(fast["values"]).all()
    assert float(fast["values"].abs().max()) > 0 and float(fast["rewards"].abs().max()) > 0
    for other in ("closure", "per_step"):
        for f in fast:
            assert torch.equal(fast[f], runs[other][f]), (other, f)
