"""GPU checks of device AM-PPO (f16env_ppo_dynago_update, f16env_ppo_loss_head_am, f16env_ppo_dag_step,
DevicePPO's am_ppo / optimizer arguments) against tests/am_ppo_ref.py's restatement of the reference
by the project's 4 x torch rule: the controller over the sizes and grids at which its sweep takes
another path, the AM head over ppo_ref.head_data's rows, DAG and AlphaGrad alone on the smallest and
the largest blob, one whole update on a real rollout, and a captured sampler + update against eager
updates bit for bit."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

import am_ppo_ref as A
import policy_grad_ref as G
import policy_ref
import ppo_ref as P
from f16_jsb_amd import abi
from test_gpu_ppo_update import B, N_ENVS, T_STEPS, _bits, _policy, _rollout, _same

pytestmark = pytest.mark.gpu

MATRIX = policy_ref.MATRIX
GUARD = 8
STATE0 = (1.0, A.as_f32(0.10))
STRIDE = 2048 * 256 * 4  # elements one stride of the controller's default grid covers


def _stream(gpu):
    return ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def _dyn_tensor(p, gpu):
    return torch.tensor([p[key] for key in A.DYNAGO], dtype=torch.float32, device=gpu)


# ---------------------------------------------------------------------------------------------
# 1. the controller
@functools.lru_cache(maxsize=None)
def _advantages(n, kind):
    rng = np.random.default_rng(9000 + n)
    a = rng.standard_normal(n)
    if kind == "offset":  # |mean| / std = 10^3: the variance's cancellation
        a = 1e-3 * a + 1.0
    return torch.from_numpy(a.astype(np.float32))


def _run_controller(gpu, adv, p, state, max_blocks, updates=2):
    """`updates` calls of f16env_ppo_dynago_update in a row on the same advantages: [(alpha, sat)]."""
    from f16_jsb_amd._lib import check, lib
    L = lib()
    n = adv.numel()
    need = ctypes.c_int64(0)
    check(L.f16env_ppo_dynago_workspace(n, max_blocks, ctypes.byref(need)), "f16env_ppo_dynago_workspace")
    ws = torch.full((need.value // 8 + GUARD,), -7.0, dtype=torch.float64, device=gpu)
    dev_adv, dyn = adv.to(gpu), _dyn_tensor(p, gpu)
    st = torch.tensor(state, dtype=torch.float32, device=gpu)
    out = []
    for _ in range(updates):
        check(L.f16env_ppo_dynago_update(_stream(gpu), n, dev_adv.data_ptr(), dyn.data_ptr(), st.data_ptr(), max_blocks,
                                         ws.data_ptr(), need.value), "f16env_ppo_dynago_update")
        torch.cuda.synchronize()
        out.append(tuple(float(v) for v in st.cpu()))
    assert (ws[-GUARD:] == -7.0).all() and _same(dev_adv, adv)
    return out


@pytest.mark.parametrize("kind", ["normal", "offset"])
@pytest.mark.parametrize("n", [2, 3, 1023, 1025, 65537, STRIDE + 5])
def test_controller_against_fp64_and_torch(gpu, n, kind):
    """n = 2, 3 (fewer elements than one vector / a tail alone), 1 023 and 1 025 (tails of 3 and 1,
    fewer vectors than a block / one into a second block), 65 537, and five past one whole stride of
    the default grid; normal advantages and advantages with |mean| / std = 10^3; max_blocks 0, 1, 2, 3.
    Two updates in a row, so the state feeds back. alpha by the 4 x rule; the saturation count within
    the number of elements whose |Z| lies within 2^-20 of tau in the fp64 reference, that band holding
    under 10^-3 of the elements; guard words and the advantages unchanged."""
    adv, p = _advantages(n, kind), A.dynago()
    bad = []
    for max_blocks in (0, 1, 2, 3):
        got = _run_controller(gpu, adv, p, STATE0, max_blocks)
        state64 = state32 = STATE0
        for i, (alpha, sat) in enumerate(got):
            r64, r32 = A.controller(adv, p, state64), A.controller(adv, p, state32, torch.float32)
            label = "n %d %s max_blocks %d update %d " % (n, kind, max_blocks, i)
            A.check(label + "alpha", alpha, r64["alpha"], r32["alpha"], bad)
            # sat' = (1 - rho_sat) sat + rho_sat count / n: the count the kernel took, from its own state
            count = (sat - (1 - p["rho_sat"]) * state64[1]) / p["rho_sat"] * n
            print(label + "count: kernel %.3f fp64 %d band %d" % (count, r64["count"], r64["band"]))
            assert r64["band"] <= 1e-3 * n, label
            # (sat' <= 1 is stored as float32: its rounding, 2^-25 at most, leaves the count to 2^-25 n / rho_sat,
            # a tenth of an element at the largest n here; 0.5 tells whole counts apart)
            if abs(count - r64["count"]) > r64["band"] + 0.5:
                bad.append((label + "count", count, r64["count"], r64["band"]))
            assert np.isfinite(alpha) and np.isfinite(sat)
            # the reference goes on from the kernel's state: each update is checked on its own
            state64 = state32 = (alpha, sat)
    assert not bad, bad


def test_controller_one_element_leaves_the_state(gpu):
    from f16_jsb_amd._lib import check, lib
    st = torch.tensor([3.25, 0.5], dtype=torch.float32, device=gpu)
    before = st.clone()
    one, dyn = torch.ones(4, device=gpu), _dyn_tensor(A.dynago(), gpu)
    ws = torch.zeros(16, dtype=torch.float64, device=gpu)
    for n in (0, 1):
        check(lib().f16env_ppo_dynago_update(_stream(gpu), n, one.data_ptr(), dyn.data_ptr(), st.data_ptr(), 0,
                                             ws.data_ptr(), 128), "f16env_ppo_dynago_update")
    torch.cuda.synchronize()
    assert _same(st, before)


# ---------------------------------------------------------------------------------------------
# 2. the AM head
HEAD_H = P.hyper(ent_coef=0.01, lr=0.0)


@functools.lru_cache(maxsize=None)
def _head_case(n, normalize, alpha, zero_adv=False):
    d = P.head_data(n)
    if zero_adv:
        d = dict(d, advantages=torch.zeros(n))
    p = A.dynago()
    return d, p, A.head_autograd(d, HEAD_H, p, alpha, normalize), A.head_autograd(d, HEAD_H, p, alpha, normalize,
                                                                                 torch.float32)


def _run_head(gpu, d, p, alpha, max_blocks, normalize):
    """f16env_ppo_loss_head_am, then f16env_ppo_adam_step with lr = 0 over a blob of eight floats whose
    last four are log_std (the AM head's workspace taken as the standard head's)."""
    from f16_jsb_amd._lib import check, lib
    L = lib()
    n = d["values"].numel()
    t = {key: d[key].to(gpu) for key in ("mean", "values", "actions", "old_log_prob", "advantages", "returns")}
    blob = torch.zeros(8, device=gpu)
    blob[4:] = d["log_std"].to(gpu)
    hyper, dyn = P.hyper_tensor(HEAD_H, gpu), _dyn_tensor(p, gpu)
    st = torch.tensor([alpha, 0.25], dtype=torch.float32, device=gpu)
    st0 = st.clone()
    need, blocks = ctypes.c_int64(0), ctypes.c_int32(0)
    check(L.f16env_ppo_workspace(n, max_blocks, ctypes.byref(need)), "f16env_ppo_workspace")
    check(L.f16env_ppo_head_blocks(n, max_blocks, ctypes.byref(blocks)), "f16env_ppo_head_blocks")
    ws = torch.full((need.value // 8 + GUARD,), -7.0, dtype=torch.float64, device=gpu)
    d_mean, d_values = torch.full((n, 4), float("nan"), device=gpu), torch.full((n,), float("nan"), device=gpu)
    grad, m, v = torch.zeros(8, device=gpu), torch.zeros(8, device=gpu), torch.zeros(8, device=gpu)
    step, stats = torch.zeros(1, dtype=torch.int32, device=gpu), torch.full((8,), float("nan"), device=gpu)
    am_stats = torch.full((4,), float("nan"), device=gpu)
    check(L.f16env_ppo_loss_head_am(_stream(gpu), n, t["mean"].data_ptr(), t["values"].data_ptr(), t["actions"].data_ptr(),
                                    t["old_log_prob"].data_ptr(), t["advantages"].data_ptr(), t["returns"].data_ptr(),
                                    blob.data_ptr() + 16, hyper.data_ptr(), dyn.data_ptr(), st.data_ptr(),
                                    abi.F16_PPO_AM_NORMALIZE if normalize else 0, max_blocks, ws.data_ptr(), need.value,
                                    d_mean.data_ptr(), d_values.data_ptr(), am_stats.data_ptr()), "f16env_ppo_loss_head_am")
    check(L.f16env_ppo_adam_step(_stream(gpu), 8, blob.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(),
                                 step.data_ptr(), hyper.data_ptr(), 4, ws.data_ptr(), blocks.value, stats.data_ptr()),
          "f16env_ppo_adam_step")
    torch.cuda.synchronize()
    assert (ws[-GUARD:] == -7.0).all() and ws[2].item() == n and _same(st, st0)   # the EMAs are frozen (ppo.py:338)
    return d_mean.cpu(), d_values.cpu(), grad[4:].cpu(), stats.cpu(), am_stats.cpu()


def _check_head(gpu, n, normalize, alpha, zero_adv=False):
    d, p, ref64, t32 = _head_case(n, normalize, alpha, zero_adv)
    bad = []
    for max_blocks in (0, 1, 2):
        d_mean, d_values, d_log_std, stats, am_stats = _run_head(gpu, d, p, alpha, max_blocks, normalize)
        label = "n %d %s alpha %g max_blocks %d " % (n, "normalized" if normalize else "raw", alpha, max_blocks)
        assert all(torch.isfinite(x).all() for x in (d_mean, d_values, d_log_std, stats, am_stats)), label
        for name, got in (("d_mean", d_mean), ("d_values", d_values), ("d_log_std", d_log_std), ("am_stats", am_stats)):
            if name == "am_stats":
                for i, key in enumerate(abi.PPO_AM_STATS):
                    A.check(label + key, got[i], ref64[name][i], t32[name][i], bad)
            else:
                A.check(label + name, got, ref64[name], t32[name], bad)
        for i, name in enumerate(P.STATS):
            A.check(label + name, stats[i], ref64["stats"][i], t32["stats"][i], bad)
        again = _run_head(gpu, d, p, alpha, max_blocks, normalize)
        assert all(_same(a, b) for a, b in zip((d_mean, d_values, d_log_std, stats, am_stats), again)), label
    return bad


@pytest.mark.parametrize("normalize", [True, False], ids=["normalized", "raw"])
@pytest.mark.parametrize("n", [1, 2, 129, 257, 1031])
def test_am_head_against_fp64_and_torch(gpu, n, normalize):
    """ppo_ref.head_data's rows (ratios off the clip edges) with old_values in place of the returns,
    alpha = 7.5 (most |Z| below 1), max_blocks 0, 1, 2: d_mean, d_values, d_log_std, the six
    statistics through f16env_ppo_adam_step (lr 0) and am_stats within 4 x torch CPU float32 autograd's
    error against fp64 autograd of the AM loss; two calls give the same bits; the state is not written."""
    bad = _check_head(gpu, n, normalize, 7.5)
    assert not bad, bad


def test_am_head_saturated_and_zero_advantages(gpu):
    """alpha = 400 at n = 257: |Z| = 400 |A| / 16 > 3 for nine rows in ten, most tanh saturate. And
    all-zero advantages (N_mb = 0, std(mod) = 0): every output finite."""
    bad = _check_head(gpu, 257, True, 400.0) + _check_head(gpu, 257, False, 400.0)
    bad += _check_head(gpu, 129, True, 7.5, zero_adv=True) + _check_head(gpu, 129, False, 7.5, zero_adv=True)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------
# 3. DAG and AlphaGrad alone
# sat_every 2 and warmup_steps 2 sample the saturation, end the warm-up and move s_t within six steps;
# lambda_rms 2 because with the default 0.3 the ratio rms_t / (lambda_rms rms0) of steady gradients
# is 3.3 and clamps to 1: s_t would stay 1 and the shrink's arithmetic would go unchecked
DAG_C = dict(warmup_steps=2, sat_every=2, lambda_rms=2.0)


def _dag_case(case, seed):
    k, d, pi_w, vf_w, _ = MATRIX[case]
    net = G.tanh_data(k, d, pi_w, vf_w, 1, seed=1)[0]
    desc = abi.policy_desc(k, d, pi_w, vf_w)
    from f16_jsb_amd.policy import pack_blob
    return k, d, pi_w, vf_w, net, desc, pack_blob(desc, *net), A.dag_gradients(desc, k, d, pi_w, vf_w, P.hyper(), seed=seed)


def _seg_rules(segs, got, ref64, t32, label, bad):
    for i, (o, n, _) in enumerate(segs):
        A.check("%s seg %d" % (label, i), got[o:o + n], ref64[o:o + n], t32[o:o + n], bad)


@pytest.mark.parametrize("case", ["G", "F"])
def test_dag_step_alone(gpu, case):
    """The smallest and the largest blob, six steps on random gradients (pads zero) with sat_every 2
    and warmup_steps 2: per step the blob per parameter tensor, every tensor's alpha and s_t,
    rms_t_ema, rms0_ema by the 4 x rule against the restatement fed the same gradients; the
    saturation per tensor exactly; pads all-bits zero; the gradient untouched; global_step 6.
    Precondition, on the fp64 reference: no |x| within 2^-20 of tau at a sampled step."""
    from f16_jsb_amd.ppo import DevicePPO
    k, d, pi_w, vf_w, net, desc, start, grads = _dag_case(case, 0)
    h, c = P.hyper(), A.dag_constants(**DAG_C)
    segs = abi.policy_segments(desc)
    ref, t32 = A.dag_steps(start, grads, h, c, segs), A.dag_steps(start, grads, h, c, segs, torch.float32)
    assert all(s["band"] == 0 for s in ref), "precondition: an |x| of the fp64 reference lies within 2^-20 of tau"
    assert any(cnt > 0 for s in ref for cnt in s["count"]) and len({s["s_t"] for s in ref}) > 2   # sampling and a moving s_t
    zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, start.numpy())["zero"]
    pol = _policy(net, gpu, k, d)
    ppo = DevicePPO(pol, max_batch=1, optimizer="dag", optimizer_kwargs=DAG_C)
    assert torch.equal(ppo.dag.cpu(), torch.tensor([c[key] for key in A.DAG])) and ppo.n_segments == len(segs)
    bad = []
    for step, g in enumerate(grads):
        dev_g = g.to(gpu)
        version = pol.blob._version
        ppo.step_from(dev_g)
        torch.cuda.synchronize()
        assert pol.blob._version > version and _same(dev_g, g)
        label = "case %s step %d" % (case, step)
        blob = pol.blob.detach().cpu()
        assert torch.isfinite(blob).all() and np.all(_bits(blob)[zero] == 0), label
        _seg_rules(segs, blob, ref[step]["blob"], t32[step]["blob"], label + " blob", bad)
        seg_state = ppo.seg_state.cpu().reshape(-1, 2)
        for i in range(len(segs)):
            A.check("%s alpha %d" % (label, i), seg_state[i, 0], ref[step]["alpha"][i], t32[step]["alpha"][i], bad)
        assert seg_state[:, 1].tolist() == ref[step]["sat"], (label, seg_state[:, 1].tolist(), ref[step]["sat"])
        ds, counters = ppo.dag_state.cpu(), ppo.dag_counters.cpu()
        for j, key in enumerate(("s_t", "rms_t", "rms0")):
            A.check("%s %s" % (label, key), ds[j], ref[step][key], t32[step][key], bad)
        assert counters.tolist() == [step + 1, 1, 1, 0]
        stats = ppo.stats.cpu()
        assert abs(stats[6].item() - ref[step]["norm"]) <= 2.0 ** -23 * ref[step]["norm"]
        assert abs(stats[7].item() - ref[step]["coef"]) <= 2.0 ** -22 * ref[step]["coef"]
    assert not bad, bad


@pytest.mark.parametrize("case", ["G", "F"])
def test_alphagrad_step_alone(gpu, case):
    """F16_PPO_DAG_FIXED_ALPHA: three steps of AlphaGrad (alpha 40, its epsilon 1e-8) checked the
    same way; DAG's state arrays are not touched."""
    from f16_jsb_amd.ppo import DevicePPO
    k, d, pi_w, vf_w, net, desc, start, grads = _dag_case(case, 1)
    grads = grads[:3]
    h, c = P.hyper(), A.dag_constants(alpha=40.0, eps=1e-8, kappa=0.0)
    segs = abi.policy_segments(desc)
    ref = A.dag_steps(start, grads, h, c, segs, fixed_alpha=True)
    t32 = A.dag_steps(start, grads, h, c, segs, torch.float32, fixed_alpha=True)
    zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, start.numpy())["zero"]
    pol = _policy(net, gpu, k, d)
    with pytest.raises(ValueError, match="Invalid alpha value"):
        DevicePPO(pol, max_batch=1, optimizer="alphagrad")
    ppo = DevicePPO(pol, max_batch=1, optimizer="alphagrad", optimizer_kwargs={"alpha": 40.0})
    before = [x.clone() for x in (ppo.seg_state, ppo.dag_state, ppo.dag_counters)]
    bad = []
    for step, g in enumerate(grads):
        dev_g = g.to(gpu)
        ppo.step_from(dev_g)
        torch.cuda.synchronize()
        blob = pol.blob.detach().cpu()
        assert _same(dev_g, g) and torch.isfinite(blob).all() and np.all(_bits(blob)[zero] == 0)
        _seg_rules(segs, blob, ref[step]["blob"], t32[step]["blob"], "alphagrad case %s step %d blob" % (case, step), bad)
    assert all(_same(a, b) for a, b in zip(before, (ppo.seg_state, ppo.dag_state, ppo.dag_counters)))
    assert not bad, bad


def test_dag_zero_gradient_moves_nothing_but_the_counter(gpu):
    from f16_jsb_amd.ppo import DevicePPO
    k, d, pi_w, vf_w, _ = MATRIX["G"]
    pol = _policy(G.tanh_data(k, d, pi_w, vf_w, 1, seed=1)[0], gpu, k, d)
    ppo = DevicePPO(pol, max_batch=1, optimizer="dag", optimizer_kwargs=DAG_C)
    start = pol.blob.detach().clone()
    for _ in range(4):
        ppo.step_from(torch.zeros(pol.n_floats, device=gpu))
    torch.cuda.synchronize()
    assert _same(pol.blob, start) and ppo.dag_counters.cpu().tolist() == [4, 1, 1, 0]
    assert torch.isfinite(ppo.seg_state).all() and torch.isfinite(ppo.dag_state).all()


# ---------------------------------------------------------------------------------------------
# 4. on a rollout
def test_am_dag_update_end_to_end(gpu, monkeypatch):
    """Case E, a minibatch of 129 from a tiny rollout: dynago_update over the buffer, then one update
    with am_ppo and the DAG optimiser. ppo.grad within the rule of the fp64 autograd of the AM loss
    (with the kernel's alpha); the new blob within the rule of the fp64 DAG reference fed the
    kernel's own gradient; train() makes eight more updates and one controller update; state_dict
    round-trips bit for bit; and a DevicePPO built with the defaults calls none of the new entry
    points."""
    from f16_jsb_amd import _lib
    from f16_jsb_amd.policy import unpack_blob
    from f16_jsb_amd.ppo import DevicePPO
    k, d, pi_w, vf_w, _ = MATRIX["E"]
    net = G.tanh_data(k, d, pi_w, vf_w, 1, seed=3)[0]
    pol = _policy(net, gpu, k, d, seed=11)
    buf = _rollout(gpu, pol, k)
    mb = next(iter(buf.get(B, generator=torch.Generator(device=gpu).manual_seed(1))))
    h, p, c = P.hyper(ent_coef=0.01), A.dynago(), A.dag_constants(**DAG_C)
    ppo = DevicePPO(pol, ent_coef=0.01, max_batch=B, am_ppo={}, optimizer="dag", optimizer_kwargs=DAG_C)
    assert torch.equal(ppo.dynago.cpu(), torch.tensor([p[key] for key in A.DYNAGO]))
    # the controller over the buffer
    adv_all = buf.advantages.detach().cpu().reshape(-1)
    ppo.dynago_update(buf.advantages)
    torch.cuda.synchronize()
    alpha, sat = (float(v) for v in ppo.am_state.cpu())
    r64, r32 = A.controller(adv_all, p, STATE0), A.controller(adv_all, p, STATE0, torch.float32)
    bad = []
    A.check("controller alpha", alpha, r64["alpha"], r32["alpha"], bad)
    count = (sat - (1 - p["rho_sat"]) * STATE0[1]) / p["rho_sat"] * adv_all.numel()
    assert abs(count - r64["count"]) <= r64["band"] + 0.5

    def loss_of(dtype):
        prm = G.as_params(net, dtype, "cpu")
        cc = lambda t: t.to(device="cpu", dtype=dtype)  # noqa: E731
        v, lp, ent = G.evaluate_actions(cc(mb.observations), cc(mb.actions), *prm, "tanh")
        loss, ratio, _ = A.am_loss(v, lp, ent, mb.advantages.cpu(), cc(mb.old_values), cc(mb.old_log_prob), p, alpha, h, True)
        loss.backward()
        return G.grads_of(prm), ratio.detach()

    ref64, ratio = loss_of(torch.float64)
    assert (ratio - 1).abs().max() < 1e-3          # unchanged weights: no row near a clip edge
    t32, _ = loss_of(torch.float32)
    start = pol.blob.detach().cpu().clone()
    ppo.update(mb)
    torch.cuda.synchronize()
    grad = ppo.grad.clone()
    assert torch.isfinite(grad).all() and ppo.dag_counters.cpu().tolist()[0] == 1 and int(ppo.step.item()) == 0
    for name, (err, allow) in G.rule_of_four(unpack_blob(pol.desc, grad), ref64, t32).items():
        print("ppo.grad %s: kernel %.3e allowed %.3e ratio of torch's %.2f" % (name, err, allow, 4.0 * err / allow if allow else 0.0))
        if not err <= allow:
            bad.append(("grad", name, err, allow))
    segs = abi.policy_segments(pol.desc)
    d64 = A.dag_steps(start, [grad.cpu()], h, c, segs)[0]
    d32 = A.dag_steps(start, [grad.cpu()], h, c, segs, torch.float32)[0]
    _seg_rules(segs, pol.blob.detach().cpu(), d64["blob"], d32["blob"], "new blob", bad)
    am_stats = ppo.am_stats.cpu()
    assert torch.isfinite(am_stats).all() and am_stats[3].item() == alpha and torch.isfinite(ppo.stats).all()
    assert not bad, bad
    zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, np.zeros(pol.n_floats, np.float32))["zero"]
    assert np.all(_bits(pol.blob)[zero] == 0) and not torch.equal(pol.blob.detach().cpu(), start)
    # train(): one controller update, two passes of four minibatches
    state_before = ppo.am_state.clone()
    assert ppo.train(buf, 2, 128, generator=torch.Generator(device=gpu).manual_seed(2)) == 8
    torch.cuda.synchronize()
    assert ppo.dag_counters.cpu().tolist()[0] == 9 and not _same(ppo.am_state, state_before)
    once = A.controller(adv_all, p, tuple(float(v) for v in state_before.cpu()))
    assert abs(ppo.am_state[0].item() - once["alpha"]) <= 4 * 2.0 ** -24 * once["alpha"]      # one update, not eight
    assert torch.isfinite(pol.blob).all() and torch.isfinite(ppo.stats).all()
    # state_dict round-trips bit for bit into a fresh DevicePPO
    sd = ppo.state_dict()
    other = DevicePPO(_policy(net, gpu, k, d), max_batch=1, am_ppo={}, optimizer="dag").load_state_dict(sd)
    for key in ("exp_avg", "exp_avg_sq", "step", "hyper", "am_state", "dynago", "dag", "seg_state", "dag_state",
                "dag_counters"):
        assert _same(getattr(other, key), getattr(ppo, key)), key
    # the defaults launch the old path: none of the new entry points is looked up or called
    called = []
    real_fn = _lib.fn

    def spying_fn(name):
        f = real_fn(name)
        if name not in ("f16env_ppo_workspace", "f16env_ppo_head_blocks", "f16env_ppo_loss_head", "f16env_ppo_adam_step"):
            called.append(name)
        return f
    monkeypatch.setattr(_lib, "fn", spying_fn)
    plain = DevicePPO(_policy(net, gpu, k, d), ent_coef=0.01, max_batch=B)
    plain.update(mb)
    plain.step_from(grad)
    torch.cuda.synchronize()
    assert [n for n in called if "dynago" in n or "_am" in n or "dag" in n] == [] and int(plain.step.item()) == 2
    assert not any(hasattr(plain, key) for key in ("dynago", "am_state", "dag", "seg_state", "dag_state"))


def test_captured_sampler_and_am_dag_update_equal_eager_updates(gpu):
    """rollout_minibatch(view, idx, out=samples) + the AM / DAG update captured once and replayed three
    times with idx overwritten in place equals three eager updates from the same start bit for bit,
    in the blob and in every state array."""
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
    names = ("blob", "seg_state", "dag_state", "dag_counters", "am_state", "am_stats", "stats", "grad")
    state = lambda pol, ppo: [x.detach().clone() for x in (pol.blob, ppo.seg_state, ppo.dag_state, ppo.dag_counters,  # noqa: E731
                                                          ppo.am_state, ppo.am_stats, ppo.stats, ppo.grad)]
    make = lambda pol: DevicePPO(pol, ent_coef=0.01, max_batch=B, am_ppo={}, optimizer="dag",  # noqa: E731
                                 optimizer_kwargs=DAG_C).dynago_update(buf.advantages)

    pol_e = _policy(net, gpu, k, d)
    ppo_e = make(pol_e)
    samples_e, eager = new_samples(), []
    for idx in batches:
        rollout_minibatch(view, idx, out=samples_e)
        ppo_e.update(samples_e)
        eager.append(state(pol_e, ppo_e))
    torch.cuda.synchronize()
    assert not _same(eager[0][0], eager[1][0]) and not _same(eager[1][0], eager[2][0])

    pol_g = _policy(net, gpu, k, d)
    ppo_g = make(pol_g)
    samples_g, idx = new_samples(), batches[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rollout_minibatch(view, idx, out=samples_g)
        ppo_g.update(samples_g)
    assert ppo_g.dag_counters.cpu().tolist()[0] == 0  # (the capture ran nothing)
    for i, batch in enumerate(batches):
        idx.copy_(batch)
        graph.replay()
        torch.cuda.synchronize()
        for name, a, b in zip(names, state(pol_g, ppo_g), eager[i]):
            assert _same(a, b), (i, name)
    assert ppo_g.dag_counters.cpu().tolist()[0] == 3
