"""GPU checks of the device LMA policy (f16env_policy_lma_forward / DeviceLMAPolicy) over the case
matrix of tests/lma_ref.py: the exact integer layout (at every K and stacking), every case against
the fp64 restatement by the project's 4 x torch rule, the newer cases at the block edges, the
stress inputs (a saturated softmax, offset LayerNorm rows, degenerate and huge rows), the inherited
mean_and_value / evaluate_actions, strided observations, batch invariance, non-finite rows, the
flags, the noise stream, graphs and streams, and collect_rollout's fast path with the deferred
bootstrap.
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
    assert lma_ref.N_ROWS == N_ROWS
    return lma_ref.shared_inputs(name)   # (the CPU tests of the stress inputs read the same rows)


@functools.lru_cache(maxsize=None)
def _net(name, seed=0):
    return lma_ref.random_net(name, seed)


# ---------------------------------------------------------------------------------------------
# (a) exact integer layout: stages 2-4, the k-step map of W_2 and the MLP fan-in
EXACT = {"W%d" % k: (k, 17, 0, 128, [64], [64], "relu", 4, lma_ref.kernel_instance(k, 17, 0, 128, [64], [64]))
         for k in range(1, 11)}
assert EXACT["W3"][8] == (17, 79488) and EXACT["W10"][8] == (17, 95872)


def _int_case(name):
    return lma_ref.int_case(EXACT[name][0])


_int_forward = lma_ref.int_forward


@pytest.mark.parametrize("n", [1, RPB + 1, 2 * RPB + 1])
@pytest.mark.parametrize("name", ["W3", "W10"])
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


@pytest.mark.parametrize("k", range(1, 11))
def test_exact_integer_layout_every_k_and_stacking(gpu, k):
    """The same exact net at every K (every L_new, C_new and deal of frames to waves) under every
    stacking the launcher accepts (dk 64 .. 2: each another arithmetic path through rmap / cmap),
    n = 33: features, means and values equal the int64 reference bit for bit."""
    name, n = "W%d" % k, lma_ref.INT_ROWS
    k_, d, act, _ = _reaches(name, EXACT)
    net, pe = _int_case(name)
    x = lma_ref.int_inputs(k, n, d)
    xg, eps = torch.as_tensor(x.astype(np.float32), device=gpu), torch.zeros((n, 4), device=gpu)
    for hs in lma_ref.STACKINGS:
        f, mean, value, bound = _int_forward(net, pe, x, hs)
        assert bound < 2 ** 24, "test data: a sum may not be exact in float32"
        assert np.abs(f).max() > 0 and np.abs(mean).max() > 0 and np.abs(value).max() > 0
        pol = _policy(net, gpu, k, d, act, hs, pe=torch.as_tensor(pe.astype(np.float32)))
        a, v, lp, feats = pol.forward_with_features(xg, 0, eps=eps)
        assert np.array_equal(feats.cpu().numpy(), f.astype(np.float32)), hs
        assert np.array_equal(a.cpu().numpy(), mean.astype(np.float32)), hs
        assert np.array_equal(v.cpu().numpy(), value.astype(np.float32)), hs


# ---------------------------------------------------------------------------------------------
# (b) precision: every case against fp64 by the 4 x torch rule
def precision(label, got, net, x, eps, act, hs, rows=None, refs=None):
    """Per output kind (kernel error, torch CPU float32 error, floor, ratio) against the fp64
    restatement, and the kinds beyond 4 x max(torch, 2^-24 max|reference|). Prints every figure.
    refs: (fp64, float32) restatements of these inputs when they are already computed."""
    ref = lma_ref.forward(net, x, eps, torch.float64, act, hs) if refs is None else refs[0]
    t32 = lma_ref.forward(net, x, eps, torch.float32, act, hs) if refs is None else refs[1]
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
    eps = eps[:x.shape[0]]   # (x: the case's first rows)
    a, v, lp, f = _policy(_net(name), gpu, k, d, act, hs).forward_with_features(
        torch.from_numpy(x).to(gpu), 0, eps=torch.from_numpy(eps).to(gpu))
    return _cpu((f, a, v, lp)), x, eps, act, hs


@pytest.mark.parametrize("name", list(MATRIX))
def test_random_net_against_fp64_over_the_matrix(gpu, name):
    got, x, eps, act, hs = run_case(name, gpu)
    _, bad = precision("case " + name, got, _net(name), x, eps, act, hs)
    assert not bad, bad


_FULL = {}


def _full_run(name, gpu):
    """The case's 257-row kernel outputs: run once, shared, not changed."""
    if name not in _FULL:
        _FULL[name] = run_case(name, gpu)[0]
    return _FULL[name]


@functools.lru_cache(maxsize=None)
def _refs65(name):
    """The fp64 and torch float32 restatements of the case's first 65 shared rows."""
    k, d, nl, ff, pi_w, vf_w, act, hs, _ = MATRIX[name]
    x, eps = _inputs(name)
    return tuple(lma_ref.forward(_net(name), x[:65], eps[:65], dt, act, hs) for dt in (torch.float64, torch.float32))


@pytest.mark.parametrize("n", [RPB - 1, RPB, RPB + 1, 2 * RPB + 1])
@pytest.mark.parametrize("name", lma_ref.NEW_CASES)
def test_new_cases_at_block_edges(gpu, name, n):
    """The first n of the case's shared rows, n = 31 (the rowc clamp in the only block), 32, 33 (one
    row alone in a second block) and 65 (a third block with one live row): the rule holds, and
    every row has the bits it has in the 257-row run."""
    k, d, act, hs = _reaches(name)
    x, eps = _inputs(name)
    got, *_ = run_case(name, gpu, x[:n])
    refs = tuple(tuple(a[:n] for a in r) for r in _refs65(name))
    _, bad = precision("case %s n %d" % (name, n), got, _net(name), x[:n], eps[:n], act, hs, refs=refs)
    assert not bad, bad
    for kind, g, full in zip(KINDS, got, _full_run(name, gpu)):
        assert g.shape[0] == n and np.array_equal(_bits(g), _bits(full[:n])), kind


# ---------------------------------------------------------------------------------------------
# (b') inputs outside the easy regime: net K6 (L_new 3), 65 rows. test_lma_cpu.py shows that each is
# well conditioned (another summation order stays within 2 x torch) and that the defect it is there
# for -- softmax without the max subtraction, a one-pass variance -- fails this rule.
def run_stress(kind, gpu):
    k, d, act, hs = _reaches(lma_ref.STRESS_CASE)
    net, x, eps, rows = lma_ref.stress_case(kind)
    a, v, lp, f = _policy(net, gpu, k, d, act, hs).forward_with_features(
        torch.from_numpy(x).to(gpu), 0, eps=torch.from_numpy(eps).to(gpu))
    return _cpu((f, a, v, lp)), net, x, eps, act, hs, rows


@pytest.mark.parametrize("kind", lma_ref.STRESS)
def test_stress_inputs_against_fp64(gpu, kind):
    """sharp: attention scores of several hundred (the softmax is saturated; exp of a raw score
    overflows). offset: LayerNorm rows of mean 100 and spread 1..4. degenerate: an all-zero row
    and a row of one repeated frame (dist = 0, atan2(0, 0); the positional table alone tells the
    tokens apart). saturated: a row of +-1e4 (the MLPs' tanh far in its tail, features of 1e3).
    Every output is finite and the unchanged 4 x torch rule holds, on all rows for the first two
    and on the altered rows for the last two (their other rows are case K6's)."""
    got, net, x, eps, act, hs, rows = run_stress(kind, gpu)
    assert all(np.all(np.isfinite(g)) for g in got)
    ref, t32, _ = lma_ref.stress_refs(kind)
    _, bad = precision("stress " + kind, got, net, x, eps, act, hs, rows=rows, refs=(ref, t32))
    assert not bad, bad
    if rows is not None:   # the altered rows stay in their rows
        others = np.setdiff1d(np.arange(x.shape[0]), rows)
        for kn, g, full in zip(KINDS, got, _full_run(lma_ref.STRESS_CASE, gpu)):
            assert np.array_equal(_bits(g[others]), _bits(full[others])), kn


# ---------------------------------------------------------------------------------------------
# (b'') the inherited entry points, strided observations and a caller's features buffer (case R)
@pytest.fixture(scope="module")
def r65(gpu):
    k, d, act, hs = _reaches("R")
    x, eps = _inputs("R")
    return {"pol": _policy(_net("R"), gpu, k, d, act, hs), "x": torch.from_numpy(x[:65]).to(gpu), "xh": x[:65], "eps": eps[:65],
            "act": act, "hs": hs}


def test_mean_and_value_is_the_deterministic_forward(r65):
    pol, x = r65["pol"], r65["x"]
    assert not pol.blob.requires_grad
    with torch.no_grad():
        mean, values = pol.mean_and_value(x)
    assert tuple(mean.shape) == (65, 4) and tuple(values.shape) == (65,)
    assert torch.equal(mean, pol(x, deterministic=True)[0]) and torch.equal(values, pol.value(x))
    assert float(mean.abs().max()) > 0 and float(values.abs().max()) > 0


def test_evaluate_actions_against_fp64(r65):
    """values, log-prob and entropy of random actions against fp64 (the diagonal Gaussian on the
    fp64 restatement's mean and log_std), by the 4 x rule; the float32 yardstick is torch's Normal
    on the float32 restatement's mean. With a blob that does not require grad, grad mode changes
    nothing."""
    pol, x, net = r65["pol"], r65["x"], _net("R")
    actions = np.random.default_rng(77).standard_normal((65, 4)).astype(np.float32)
    zeros = np.zeros((65, 4), np.float32)
    ref = lma_ref.forward(net, r65["xh"], zeros, torch.float64, r65["act"], r65["hs"])
    t32 = lma_ref.forward(net, r65["xh"], zeros, torch.float32, r65["act"], r65["hs"])
    ls = net["log_std"].astype(np.float64)
    want = (ref[2], (-0.5 * ((actions - ref[4]) / np.exp(ls)) ** 2 - ls - lma_ref.LOG_SQRT_2PI).sum(-1),
            np.full(65, (0.5 + lma_ref.LOG_SQRT_2PI + ls).sum()))
    dist = torch.distributions.Normal(torch.from_numpy(t32[4]), torch.ones(65, 4) * torch.from_numpy(net["log_std"]).exp())
    yard = (t32[2], dist.log_prob(torch.from_numpy(actions)).sum(1).numpy(), dist.entropy().sum(1).numpy())
    assert torch.is_grad_enabled() and not pol.blob.requires_grad
    got = pol.evaluate_actions(x, torch.from_numpy(actions).to(x.device))
    with torch.no_grad():
        again = pol.evaluate_actions(x, torch.from_numpy(actions).to(x.device))
    assert all(torch.equal(p, q) and not p.requires_grad for p, q in zip(got, again))
    for kind, g, t, r in zip(("values", "log_prob", "entropy"), _cpu(got), yard, want):
        e_k, e_t, floor = np.abs(g.astype(np.float64) - r).max(), np.abs(t.astype(np.float64) - r).max(), 2.0 ** -24 * np.abs(r).max()
        print("evaluate_actions %s: kernel %.3e torch %.3e floor %.3e ratio %.2f" % (kind, e_k, e_t, floor, e_k / max(e_t, floor)))
        assert g.shape == (65,) and np.all(np.isfinite(g)) and e_k <= 4.0 * max(e_t, floor), kind


def test_strided_observations_give_the_bits_of_their_copies(gpu, r65):
    """A (65, K, 15) view whose rows are K 15 + 7 floats apart, cut from a wider buffer at a nonzero
    storage offset, and one frame expanded over K (frame stride 0): the bits of .contiguous()."""
    pol, x, eps = r65["pol"], r65["x"], torch.from_numpy(r65["eps"]).to(gpu)
    k, d = x.shape[1:]
    stride = k * d + 7
    buf = torch.full((5 + 65 * stride + 11,), float("nan"), device=gpu)
    view = torch.as_strided(buf, (65, k, d), (stride, d, 1), 5)
    view.copy_(x)
    assert view.stride() == (stride, d, 1) and view.storage_offset() == 5 and not view.is_contiguous()
    frame = x[:, 3:4, :].expand(65, k, d)
    assert frame.stride(1) == 0 and frame.storage_offset() == 3 * d
    for name, obs in (("row stride", view), ("expanded frame", frame)):
        got = pol.forward_with_features(obs, 0, eps=eps)
        want = pol.forward_with_features(obs.contiguous(), 0, eps=eps)
        assert all(torch.equal(p, q) for p, q in zip(got, want)) and torch.isfinite(got[3]).all(), name
        assert torch.equal(pol.value(obs), want[1]) and torch.equal(pol.mean_and_value(obs)[1], want[1]), name
    assert torch.equal(pol.forward_with_features(view, 0, eps=eps)[3], pol.extract_features(x))


def test_extract_features_into_a_callers_buffer(gpu, r65):
    pol, x = r65["pol"], r65["x"]
    out = torch.full((65, pol.features_dim), float("nan"), device=gpu)
    assert out.data_ptr() % 16 == 0
    assert pol.extract_features(x, out=out) is out
    assert torch.equal(out, pol.extract_features(x)) and torch.isfinite(out).all()
    with pytest.raises(ValueError):
        pol.extract_features(x, out=torch.empty((64, pol.features_dim), device=gpu))


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
