"""GPU tests of the device LMA policy's eval-mode backward (f16env_policy_lma_backward through
DeviceLMATrainPolicy): exact integer nets for every K and stacking, every matrix case against fp64
by the precision rule of tests/lma_grad_ref.py, tails, NULL branches, determinism, observations
read in place, the hard inputs, the autograd path with an optimiser step, and the edges."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import lma_grad_ref as G
import lma_ref
import policy_grad_ref

pytestmark = pytest.mark.gpu

MATRIX = lma_ref.MATRIX
OFF_VF0 = 6   # f16env_policy_blob_layout's slot of the vf branch's first hidden layer (6 b + 2 l, b = 1)


def _args(net, gpu):
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=gpu)  # noqa: E731
    pair = lambda wb: (t(wb[0]), t(wb[1]))  # noqa: E731
    ext = {"embed": pair(net["embed"]), "embed2": pair(net["embed2"]),
           "blocks": [{k: pair(v) for k, v in blk.items()} for blk in net["blocks"]]}
    return ext, [pair(l) for l in net["pi"]], [pair(l) for l in net["vf"]], pair(net["act"]), pair(net["val"]), t(net["log_std"])


def _policy(net, gpu, k, d, act="tanh", hs=4, **kw):
    from f16_jsb_amd.lma_policy import DeviceLMATrainPolicy
    return DeviceLMATrainPolicy.from_layers(*_args(net, gpu), stack_k=k, frame_dim=d, activation=act, heads_stacking=hs, **kw)


def _dev(a, gpu):
    return None if a is None else torch.as_tensor(np.asarray(a, np.float32), device=gpu).contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_untrained_zero(pol, blob):
    mask = torch.as_tensor(G.untrained_positions(pol.desc, pol.lma))
    assert not _bits(blob)[mask].any(), "a pad, log_std slot or PE position is not +0"


def _within(rule, pol, blob, label):
    """Print every tensor's figure, then assert it against the input's allowance."""
    res = rule.check(G.unpack(pol.desc, pol.lma, blob))
    worst = max(res, key=lambda n: res[n][0] / res[n][1] if res[n][1] > 0 else 0.0)
    print("%s: r %.2f F %.2f; worst %s: error %.3e allowance %.3e (%.2f x the base)"
          % (label, rule.r, rule.F, worst, res[worst][0], res[worst][1], rule.F * res[worst][0] / res[worst][1]))
    assert bool(torch.isfinite(blob).all()), label
    for name, (err, allow) in res.items():
        assert err <= allow, (label, name, err, allow)
    return res


# ---------------------------------------------------------------------------------------------
# (a) exact
@pytest.mark.parametrize("k", range(1, 11))
def test_exact_integer_gradient_every_k_and_stacking(gpu, k):
    """Zero-block integer nets under ReLU on D = 17 integer inputs, n = 33, every stacking, the
    default grid and one block: every partial sum is an integer below 2^24 (asserted on the CPU
    side), so the gradient equals the fp64 autograd value bit for bit in blob layout, pads,
    log_std and PE all-bits zero. This pins the transposed fold and both embeddings."""
    n = lma_ref.INT_ROWS
    net, pe, x, dm, dv = G.int_input(k, n)
    xg, dmg, dvg = _dev(x, gpu), _dev(dm, gpu), _dev(dv, gpu)
    for hs in lma_ref.STACKINGS:
        want, peak = G.int_vjp(k, hs, n)
        assert peak < G.EXACT, "test data: a sum may not be exact in float32"
        pol = _policy(net, gpu, k, 17, "relu", hs, pe=torch.as_tensor(pe.astype(np.float32)))
        wblob = G.pack(pol.desc, pol.lma, want)
        assert float(wblob.abs().max()) > 0
        for mb in (0, 1):
            got = pol.backward_blob(xg, dmg, dvg, max_blocks=mb)
            assert torch.equal(_bits(got), _bits(wblob)), (hs, mb)
            _assert_untrained_zero(pol, got)


# ---------------------------------------------------------------------------------------------
# (b) precision
def _run_case(name, gpu, n=lma_ref.N_ROWS, d_mean=True, d_values=True, max_blocks=0):
    k, d = MATRIX[name][:2]
    net, obs, dm, dv, act, hs = G.case_input(name, n)
    pol = _policy(net, gpu, k, d, act, hs)
    x = torch.from_numpy(obs).to(gpu)
    assert x.shape[0] == n
    return pol, x, pol.backward_blob(x, _dev(dm, gpu) if d_mean else None, _dev(dv, gpu) if d_values else None,
                                     max_blocks=max_blocks)


@pytest.mark.parametrize("name", list(MATRIX))
def test_matrix_against_fp64(gpu, name):
    """Every matrix case at 257 rows with its own activation and stacking, upstream gradients
    N(0, 1) / n: every parameter tensor within its case's allowance; the untrained positions +0."""
    pol, _, got = _run_case(name, gpu)
    _within(G.case_rule(name), pol, got, name)
    _assert_untrained_zero(pol, got)


@pytest.mark.parametrize("n", [1, 31, 33, 65])
@pytest.mark.parametrize("name", ["S", "K6"])
def test_tails_against_fp64(gpu, name, n):
    """obs, d_mean and d_values hold exactly n rows: one row; a tile one short; one row alone in a
    second tile; a third tile with one row. The rule of the input's own rows."""
    pol, x, got = _run_case(name, gpu, n)
    assert x.shape[0] == n
    _within(G.case_rule(name, n), pol, got, "%s n=%d" % (name, n))
    _assert_untrained_zero(pol, got)


# ---------------------------------------------------------------------------------------------
# (c) NULL branches
def test_null_branches(gpu):
    from f16_jsb_amd.abi import F16_POLICY_OFF_ACT_W, F16_POLICY_OFF_VAL_W
    name, n = "S", 65
    rule = G.case_rule(name, n)
    pol, x, both = _run_case(name, gpu, n)
    _, _, pi_only = _run_case(name, gpu, n, d_values=False)
    _, _, vf_only = _run_case(name, gpu, n, d_mean=False)
    off = pol.offsets
    vf_pieces = torch.zeros(pol.n_floats, dtype=torch.bool)
    vf_pieces[off[OFF_VF0]:off[F16_POLICY_OFF_ACT_W]] = True
    vf_pieces[off[F16_POLICY_OFF_VAL_W]:off[F16_POLICY_OFF_VAL_W + 1] + 32] = True
    pi_pieces = torch.zeros(pol.n_floats, dtype=torch.bool)
    pi_pieces[:off[OFF_VF0]] = True
    pi_pieces[off[F16_POLICY_OFF_ACT_W]:off[F16_POLICY_OFF_VAL_W]] = True
    assert not _bits(pi_only)[vf_pieces].any() and not _bits(vf_only)[pi_pieces].any()
    assert _bits(pi_only)[pi_pieces].any() and _bits(vf_only)[vf_pieces].any()
    assert torch.equal(_bits(pi_only)[pi_pieces], _bits(both)[pi_pieces])
    assert torch.equal(_bits(vf_only)[vf_pieces], _bits(both)[vf_pieces])
    _within(rule, pol, pi_only + vf_only, "one-sided sum")
    with pytest.raises(ValueError):
        pol.backward_blob(x, None, None)


# ---------------------------------------------------------------------------------------------
# (d) determinism
def test_determinism_graph_replay_and_load(gpu):
    name, n = "R", 65
    k, d = MATRIX[name][:2]
    net, obs, dm, dv, act, hs = G.case_input(name, n)
    rule = G.case_rule(name, n)
    pol = _policy(net, gpu, k, d, act, hs)
    x, dmg, dvg = torch.from_numpy(obs).to(gpu), _dev(dm, gpu), _dev(dv, gpu)
    first = pol.backward_blob(x, dmg, dvg)
    assert torch.equal(_bits(first), _bits(pol.backward_blob(x, dmg, dvg)))
    _within(rule, pol, first, "R n=65")
    pol.reserve_backward(n)
    out = torch.zeros(pol.n_floats, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pol.backward_blob(x, dmg, dvg, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(first))
    pol.load(*_args(net, gpu))
    assert torch.equal(_bits(pol.backward_blob(x, dmg, dvg)), _bits(first))
    for mb in (1, 2):
        _within(rule, pol, pol.backward_blob(x, dmg, dvg, max_blocks=mb), "max_blocks %d" % mb)
    assert torch.equal(_bits(pol.backward_blob(x, dmg, dvg, max_blocks=0)), _bits(first))


# ---------------------------------------------------------------------------------------------
# (e) in place
def test_observations_read_in_place(gpu):
    name, n = "R", 65
    k, d = MATRIX[name][:2]
    net, obs, dm, dv, act, hs = G.case_input(name, n)
    pol = _policy(net, gpu, k, d, act, hs)
    x, dmg, dvg = torch.from_numpy(obs).to(gpu), _dev(dm, gpu), _dev(dv, gpu)
    stride = k * d + 7
    buf = torch.full((5 + n * stride + 11,), float("nan"), device=gpu)
    view = torch.as_strided(buf, (n, k, d), (stride, d, 1), 5)
    view.copy_(x)
    assert view.stride() == (stride, d, 1) and view.storage_offset() == 5 and not view.is_contiguous()
    frame = x[:, 3:4, :].expand(n, k, d)
    assert frame.stride(1) == 0
    for label, o in (("row stride", view), ("expanded frame", frame)):
        got, want = pol.backward_blob(o, dmg, dvg), pol.backward_blob(o.contiguous(), dmg, dvg)
        assert torch.equal(_bits(got), _bits(want)) and bool(torch.isfinite(got).all()), label
    from f16_jsb_amd.features import stacked_features
    pol17 = _policy(net, gpu, k, 17, act, hs)
    _within(G.case_rule(name, n), pol17, pol17.backward_blob(stacked_features(x), dmg, dvg), "D = 17 on f16env_features")


# ---------------------------------------------------------------------------------------------
# (f) hard inputs
@pytest.mark.parametrize("kind", lma_ref.STRESS)
def test_stress_inputs_against_fp64(gpu, kind):
    """lma_ref.stress_case's four inputs on net K6, 65 rows: every gradient finite and within that
    input's own allowance (F from that input's r)."""
    net, obs, dm, dv, act, hs = G.stress_input(kind)
    k, d = MATRIX[lma_ref.STRESS_CASE][:2]
    pol = _policy(net, gpu, k, d, act, hs)
    got = pol.backward_blob(torch.from_numpy(obs).to(gpu), _dev(dm, gpu), _dev(dv, gpu))
    _within(G.stress_rule(kind), pol, got, kind)


# ---------------------------------------------------------------------------------------------
# (g) through autograd
def test_autograd_ppo_loss_and_adam_step(gpu):
    from f16_jsb_amd.abi import F16_POLICY_OFF_LOG_STD
    name, n = "S", 64
    k, d, act, hs = MATRIX[name][0], MATRIX[name][1], MATRIX[name][6], MATRIX[name][7]
    net = lma_ref.random_net(name)
    obs = lma_ref.shared_inputs(name)[0][:n]
    rng = np.random.default_rng(5)
    actions, adv, ret, old_lp = (rng.standard_normal(s).astype(np.float32) for s in ((n, 4), n, n, n))
    old_lp = old_lp * 0.1 - 4.0

    def loss_of(values, log_prob, entropy, dtype, dev):
        t = lambda a: torch.as_tensor(a).to(device=dev, dtype=dtype)  # noqa: E731
        return policy_grad_ref.ppo_loss(values, log_prob, entropy, t(adv), t(ret), t(old_lp))[0]

    def reference(dtype, flip=False):
        p = G.leaves(net, dtype)
        ls = torch.as_tensor(net["log_std"]).to(dtype).clone().requires_grad_(True)
        _, mean, values = G.forward(p, obs, dtype, act, hs, flip=flip)
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * ls.exp())
        a = torch.as_tensor(actions).to(dtype)
        loss_of(values, dist.log_prob(a).sum(1), dist.entropy().sum(1), dtype, "cpu").backward()
        g = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
        pair = lambda wb: (g(wb[0]), g(wb[1]))  # noqa: E731
        return ({"embed": pair(p["embed"]), "embed2": pair(p["embed2"]),
                 "blocks": [{piece: pair(blk[piece]) for piece in lma_ref.BLOCK_PIECES} for blk in p["blocks"]],
                 "pi": [pair(l) for l in p["pi"]], "vf": [pair(l) for l in p["vf"]], "act": pair(p["act"]),
                 "val": pair(p["val"])}, ls.grad)
    ref64, ls64 = reference(torch.float64)
    t32, ls32 = reference(torch.float32)
    f32, lsf = reference(torch.float32, flip=True)

    pol = _policy(net, gpu, k, d, act, hs).requires_grad_()
    x, a = torch.from_numpy(obs).to(gpu), torch.from_numpy(actions).to(gpu)
    values, log_prob, entropy = pol.evaluate_actions(x, a)
    loss = loss_of(values, log_prob, entropy, torch.float32, gpu)
    loss.backward(retain_graph=True)
    grad = pol.blob.grad.detach().clone()
    got = G.unpack(pol.desc, pol.lma, grad)
    ratios = {}
    for (tname, g_), (_, r_), (_, t_), (_, f_) in zip(G.named_tensors(got), G.named_tensors(ref64), G.named_tensors(t32),
                                                       G.named_tensors(f32)):
        base = max(G._err(t_, r_), 2.0 ** -24 * float(r_.abs().max()))
        ratios[tname] = (G._err(g_, r_), base, G._err(f_, r_))
    ls = pol.offsets[F16_POLICY_OFF_LOG_STD]
    base = max(G._err(ls32, ls64), 2.0 ** -24 * float(ls64.abs().max()))
    ratios["log_std"] = (G._err(grad[ls:ls + 4], ls64), base, G._err(lsf, ls64))
    r = max(f / b for _, b, f in ratios.values())
    F = max(4.0, 2.0 * r)
    worst = max(ratios, key=lambda t: ratios[t][0] / ratios[t][1])
    print("autograd: r %.2f F %.2f; worst %s %.2f x the base" % (r, F, worst, ratios[worst][0] / ratios[worst][1]))
    for tname, (e, b, _) in ratios.items():
        assert e <= F * b, (tname, e, F * b)
    mask = torch.as_tensor(G.untrained_positions(pol.desc, pol.lma))
    mask[ls:ls + 4] = False
    assert not _bits(grad)[mask].any()

    before = pol.blob.detach().clone()
    opt = torch.optim.Adam(pol.parameters(), lr=3e-4, eps=1e-5)
    torch.nn.utils.clip_grad_norm_(pol.parameters(), 0.5)
    opt.step()
    after = pol.blob.detach()
    assert torch.equal(_bits(after)[mask], _bits(before)[mask]) and not torch.equal(after, before)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


# ---------------------------------------------------------------------------------------------
# (h) edges
def test_edges(gpu):
    from f16_jsb_amd._lib import lib
    name, n = "S", 33
    k, d = MATRIX[name][:2]
    net, obs, dm, dv, act, hs = G.case_input(name, n)
    pol = _policy(net, gpu, k, d, act, hs)
    x, dmg, dvg = torch.from_numpy(obs).to(gpu), _dev(dm, gpu), _dev(dv, gpu)
    L = lib()
    ws = pol.reserve_backward(n)
    need = ctypes.c_int64(0)
    assert L.f16env_policy_lma_backward_workspace(pol._desc_ref, pol._lma_ref, n, 0, ctypes.byref(need)) == 0
    assert 0 < need.value <= ws.numel()
    out = torch.full((pol.n_floats + 4,), 7.0, device=gpu)

    def call(n_, ws_bytes, grad_ptr):
        return L.f16env_policy_lma_backward(None, pol._desc_ref, pol._lma_ref, pol.blob.data_ptr(), n_, x.data_ptr(),
                                            x.stride(0), x.stride(1), dmg.data_ptr(), dvg.data_ptr(), ws.data_ptr(), ws_bytes,
                                            0, grad_ptr)
    with torch.cuda.device(gpu):
        assert call(0, need.value, out.data_ptr()) == 0                      # n == 0 writes nothing
        assert call(n, need.value - 1, out.data_ptr()) < 0 and b"workspace" in L.f16env_last_error()
        assert call(n, need.value, out.data_ptr() + 4) < 0 and b"aligned" in L.f16env_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    got = pol.backward_blob(x, dmg, dvg, out=out[:pol.n_floats])
    assert got.data_ptr() == out.data_ptr() and float(out[pol.n_floats]) == 7.0
    _within(G.case_rule(name, n), pol, got, "S n=33 into a caller's buffer")
    empty = pol.backward_blob(x[:0], dmg[:0], dvg[:0])
    assert empty.shape == (pol.n_floats,) and not empty.any()
