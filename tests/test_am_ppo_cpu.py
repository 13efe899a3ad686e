"""CPU checks of device AM-PPO: the library exports the new entry points under ABI 7 and refuses bad
arguments before any launch (no device needed); the workspace functions are pure and monotone; and
the restatement of the reference that the GPU tests check the kernels against (tests/am_ppo_ref.py)
is pinned by known answers, by its edge cases and by planted defects."""
from __future__ import annotations

import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import am_ppo_ref as A
import policy_grad_ref as G
import policy_ref
import ppo_ref as P
from f16_jsb_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("f16env_ppo_dynago_workspace", "f16env_ppo_dynago_update", "f16env_ppo_loss_head_am", "f16env_ppo_dag_step")
PTR = 0x10000  # a non-NULL, 16-B aligned address that is never dereferenced: every call below fails before a launch


@pytest.fixture(scope="module")
def L():
    from f16_jsb_amd.build import build
    build()
    from f16_jsb_amd import _lib
    return _lib.lib()


def test_library_exports_the_new_symbols_under_abi_7(L):
    from f16_jsb_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (f16env_\w+)", out))
    assert set(NEW) <= exported and set(NEW) <= set(_lib.EXPORTED_SYMBOLS)
    assert "#define F16ENV_ABI_VERSION 7" in open(os.path.join(ROOT, "include", "f16env.h")).read()
    assert L.f16env_abi_version() == 7 == abi.F16ENV_ABI_VERSION
    assert len(abi.PPO_DYNAGO) == abi.F16_PPO_N_DYNAGO == len(A.DYNAGO) and abi.PPO_DYNAGO == A.DYNAGO
    assert len(abi.PPO_DAG) == abi.F16_PPO_N_DAG and abi.PPO_DAG == A.DAG
    assert [getattr(abi, "F16_PPO_DYNAGO_" + n.upper()) for n in abi.PPO_DYNAGO] == list(range(abi.F16_PPO_N_DYNAGO))
    assert [getattr(abi, "F16_PPO_DAG_" + n.upper()) for n in abi.PPO_DAG] == list(range(abi.F16_PPO_N_DAG))
    assert len(abi.PPO_AM_STATS) == abi.F16_PPO_N_AM_STATS


def test_workspace_functions_are_pure_and_monotone(L):
    def need(n, max_blocks):
        b = ctypes.c_int64(-1)
        assert L.f16env_ppo_dynago_workspace(n, max_blocks, ctypes.byref(b)) == 0
        return b.value
    assert need(0, 0) == 0 and need(1, 0) == 0 and need(2, 0) == 24 and need(1025, 0) == 24 * 2
    assert need(1 << 30, 0) == 24 * 2048 and need(1 << 30, 3) == 24 * 3
    ns = [0, 1, 2, 3, 1023, 1024, 1025, 65537, 2048 * 1024 + 5, 1 << 28]
    for mb in (0, 1, 2, 3, 4096):
        sizes = [need(n, mb) for n in ns]
        assert sizes == sorted(sizes), mb
    for n in ns:
        sizes = [need(n, mb) for mb in (1, 2, 3, 2048, 4096)]
        assert sizes == sorted(sizes) and need(n, 0) == need(n, 2048), n
    assert L.f16env_ppo_dynago_workspace(-1, 0, ctypes.byref(ctypes.c_int64())) < 0
    assert L.f16env_ppo_dynago_workspace(8, -1, ctypes.byref(ctypes.c_int64())) < 0
    assert L.f16env_ppo_dynago_workspace(8, 0, None) < 0


def test_dynago_update_refuses_bad_arguments(L):
    f = L.f16env_ppo_dynago_update
    assert f(None, 0, None, None, None, 0, None, 0) == 0            # n = 0: nothing to do
    assert f(None, 1, None, None, None, 0, None, 0) == 0            # n = 1: ppo.py:40-41 returns before any update
    good = [None, 1025, PTR, PTR, PTR, 0, PTR, 48]
    for i in (2, 3, 4, 6):                                          # NULL pointers
        a = list(good)
        a[i] = None
        assert f(*a) < 0, i
    for i, off in ((2, 4), (3, 2), (4, 2), (6, 4)):                 # advantages off 16 B, floats off 4, workspace off 8
        a = list(good)
        a[i] = PTR + off
        assert f(*a) < 0, i
    assert f(*good[:7], 47) < 0                                     # a short workspace
    assert f(None, -1, PTR, PTR, PTR, 0, PTR, 48) < 0 and f(None, 1025, PTR, PTR, PTR, -1, PTR, 48) < 0
    assert L.f16env_last_error()


def test_loss_head_am_refuses_bad_arguments(L):
    f = L.f16env_ppo_loss_head_am
    n, ws = 300, 8 * (4 + 8 * 2)
    good = [None, n] + [PTR] * 10 + [abi.F16_PPO_AM_NORMALIZE, 0, PTR, ws, PTR, PTR, PTR]
    assert f(*([None, 0] + [None] * 10 + [0, 0, None, 0, None, None, None])) == 0    # n = 0
    for i in list(range(2, 12)) + [14, 16, 17]:                     # every pointer but am_stats may not be NULL
        a = list(good)
        a[i] = None
        assert f(*a) < 0, i
    for i, off in ((2, 4), (4, 8), (16, 4), (14, 4), (3, 2), (10, 2), (11, 2), (18, 2)):
        a = list(good)
        a[i] = PTR + off
        assert f(*a) < 0, i
    for flags in (0x2, 0x80000000):
        assert f(*(good[:12] + [flags] + good[13:])) < 0
    assert f(*(good[:15] + [ws - 1] + good[16:])) < 0               # a short workspace
    assert f(*(good[:13] + [-1] + good[14:])) < 0 and f(*([None, -1] + good[2:])) < 0


def test_dag_step_refuses_bad_arguments(L):
    f = L.f16env_ppo_dag_step
    table = lambda *rows: (ctypes.c_int32 * (3 * len(rows)))(*[v for r in rows for v in r])  # noqa: E731
    ok = table((0, 64, 60), (64, 32, 4))
    nf = 100

    def call(segments=ok, n_segments=2, flags=0, **kw):
        a = dict(nf=nf, blob=PTR, grad=PTR, hyper=PTR, dag=PTR, seg_state=PTR, dag_state=PTR, counters=PTR, ls=0, ws=None,
                 blocks=0, stats=PTR)
        a.update(kw)
        return f(None, a["nf"], a["blob"], a["grad"], a["hyper"], a["dag"], segments, n_segments, a["seg_state"],
                 a["dag_state"], a["counters"], flags, a["ls"], a["ws"], a["blocks"], a["stats"])
    assert f(None, 0, None, None, None, None, None, 0, None, None, None, 0, 0, None, 0, None) == 0   # n_floats = 0
    assert call(nf=-1) < 0
    for key in ("blob", "grad", "hyper", "dag", "seg_state", "dag_state", "counters"):
        assert call(**{key: None}) < 0, key
        assert call(**{key: PTR + 2}) < 0, key
    assert call(dag_state=PTR + 4) < 0 and call(stats=PTR + 2) < 0
    assert call(segments=None) < 0
    for flags in (0x2, 0x100):
        assert call(flags=flags) < 0
    # bad segment tables: none or too many, out of the blob, overlapping, descending, count 0 or past the length
    assert call(n_segments=0) < 0 and call(segments=table(*[(i, 1, 1) for i in range(18)]), n_segments=18) < 0
    for bad in (table((0, 64, 60), (64, 37, 4)), table((0, 64, 60), (63, 32, 4)), table((64, 32, 4), (0, 64, 60)),
                table((0, 64, 0), (64, 32, 4)), table((0, 64, 65), (64, 32, 4)), table((-1, 64, 60), (64, 32, 4)),
                table((0, 0, 0), (64, 32, 4))):
        assert call(segments=bad) < 0, list(bad)
    assert b"segment" in L.f16env_last_error()
    # with a head workspace: its alignment, head_blocks, log_std_offset
    assert call(ws=PTR + 4, blocks=1) < 0 and call(ws=PTR, blocks=0) < 0
    assert call(ws=PTR, blocks=1, ls=-1) < 0 and call(ws=PTR, blocks=1, ls=nf - 3) < 0


def test_python_refuses_what_the_kernel_does_not_build():
    """sgd.py:414-415: AlphaGrad's alpha <= 0 (train.py's default of 0.0) raises ValueError; DAG's
    momentum, weight decay, schedule and exact-sigma options are refused; kappa's default is
    tau / Phi^-1(1 - p_star / 2)."""
    from f16_jsb_amd import ppo
    with pytest.raises(ValueError, match="Invalid alpha value"):
        ppo._dag_constants("alphagrad", {})
    with pytest.raises(ValueError, match="Invalid alpha value"):
        ppo._dag_constants("alphagrad", {"alpha": -1.0})
    assert ppo._dag_constants("alphagrad", {"alpha": 2.0})["eps"] == 1e-8
    for key, value in (("momentum", 0.9), ("weight_decay", 1e-2), ("nesterov", True), ("maximize", True),
                       ("k_sched", lambda step: 1.0), ("use_exact_sigma", True)):
        with pytest.raises(ValueError, match="not built"):
            ppo._dag_constants("dag", {key: value})
    with pytest.raises(ValueError, match="unknown DAG"):
        ppo._dag_constants("dag", {"learning_rate": 1.0})
    c = ppo._dag_constants("dag", {"hyper": {"tau": 1.5}, "shrink": {"warmup_steps": 7}, "sat_every": 3})
    assert set(c) == set(abi.PPO_DAG) and c["tau"] == 1.5 and c["warmup_steps"] == 7 and c["sat_every"] == 3
    assert abs(c["kappa"] - 1.5 / 1.6448536269514722) < 1e-12      # Phi^-1(0.95)
    assert A.dag_constants()["kappa"] == float(np.float32(ppo.dag_kappa(1.25, 0.10)))
    assert set(ppo.AM_PPO_DEFAULTS) - {"alpha_init", "sat_init", "norm_adv"} == set(abi.PPO_DYNAGO)


def test_policy_segments_tile_the_blob():
    """The table DevicePPO hands f16env_ppo_dag_step: one segment per parameter tensor, at most 17,
    ascending and tiling the blob; the true counts are the tensors' numel, and exactly the pads lie
    outside them."""
    for case, (k, d, pi_w, vf_w, _) in policy_ref.MATRIX.items():
        desc = abi.policy_desc(k, d, pi_w, vf_w)
        off, total = abi.policy_blob_layout(desc)
        segs = abi.policy_segments(desc)
        assert len(segs) == 2 * (len(pi_w) + len(vf_w)) + 5 <= abi.F16_PPO_DAG_MAX_SEGMENTS, case
        assert segs[0][0] == 0 and segs[-1][0] + segs[-1][1] == total
        assert all(a[0] + a[1] == b[0] for a, b in zip(segs, segs[1:]))
        zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, np.zeros(total, np.float32))["zero"]
        assert sum(c for _, _, c in segs) == total - int(np.count_nonzero(zero)), case
        net = G.tanh_data(k, d, pi_w, vf_w, 1)[0]
        assert [c for _, _, c in segs] == [t.numel() for _, t in G.named_tensors(net)], case


# ---------------------------------------------------------------------------------------------
# the restatement, pinned
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_known_answers_pin_the_restatement(dtype):
    """A = (+a, -a, ...) with M even: N = a sqrt(M), mean 0, std = a sqrt(M / (M - 1)); every |Z| is
    alpha' a / (N + eps), so the saturation is exactly 0 or 1 on either side of tau; mod = +-a
    (kappa tanh Z) + a v. Through one controller update and one modulation."""
    M, a = 64, 0.5                                       # a, N = 4, N^2 = 16 exact in float32
    adv = torch.tensor([a, -a] * (M // 2), dtype=torch.float32)
    tol = 1e-12 if dtype == torch.float64 else 2e-6
    for tau, expect_sat in ((0.2, 1.0), (0.5, 0.0)):
        p = A.dynago(tau=tau, v_shift=0.25)
        eps, alpha0, sat0 = p["eps"], 1.0, A.as_f32(0.10)
        out = A.controller(adv, p, (alpha0, sat0), dtype)
        N, sigma = a * math.sqrt(M), a * math.sqrt(M / (M - 1)) + eps
        assert abs(out["N"] - N) <= tol * N and abs(out["sigma"] - sigma) <= tol * sigma
        a_hat = p["kappa_controller"] * (N + eps) / (sigma + eps) * (p["p_star"] / (sat0 + eps)) ** p["eta"]
        alpha = min(max((1 - p["rho"]) * alpha0 + p["rho"] * a_hat, p["alpha_min"]), p["alpha_max"])
        assert abs(out["alpha"] - alpha) <= max(tol, 2.0 ** -24) * alpha and out["alpha"] == A.as_f32(out["alpha"])
        z = out["alpha"] / (N + eps) * a                 # every |Z|: 0.31, between the two taus, far from both
        assert 0.2 * 1.25 < z < 0.5 / 1.25
        assert out["count"] == (M if expect_sat else 0) and out["band"] == 0
        sat = (1 - p["rho_sat"]) * sat0 + p["rho_sat"] * expect_sat
        assert abs(out["sat"] - sat) <= 2.0 ** -23
        mod, n_mb = A.modulate(adv, p, out["alpha"], dtype)
        sign = torch.tensor([1.0, -1.0] * (M // 2), dtype=torch.float64)
        want = a * (p["kappa"] * math.tanh(z) * sign + p["v_shift"])
        assert abs(float(n_mb) - N) <= tol * N
        assert (mod.double() - want).abs().max().item() <= max(tol, 2.0 ** -22) * float(want.abs().max())


def test_edge_cases_of_the_restatement():
    p, h, c = A.dynago(), P.hyper(), A.dag_constants(warmup_steps=2, sat_every=2)
    state = (1.0, A.as_f32(0.1))
    # n = 1 is the identity, for the controller and for the modulation
    one = torch.tensor([0.7], dtype=torch.float32)
    out = A.controller(one, p, state)
    assert (out["alpha"], out["sat"]) == state
    assert torch.equal(A.modulate(one, p, 3.0)[0], one.double())
    # all-zero advantages: finite everywhere
    zeros = torch.zeros(64)
    for dtype in (torch.float64, torch.float32):
        out = A.controller(zeros, p, state, dtype)
        assert math.isfinite(out["alpha"]) and math.isfinite(out["sat"]) and out["count"] == 0
        assert torch.equal(A.modulate(zeros, p, out["alpha"], dtype)[0], torch.zeros(64, dtype=dtype))
    # DAG on a gradient of zeros: the blob does not move, global_step does
    segs = [(0, 64, 60), (64, 32, 4)]
    blob = torch.randn(96, generator=torch.Generator().manual_seed(0))
    steps = A.dag_steps(blob, [torch.zeros(96)] * 4, h, c, segs)
    assert all(torch.equal(s["blob"], blob.double()) for s in steps) and [s["step"] for s in steps] == [1, 2, 3, 4]
    assert all(math.isfinite(v) for s in steps for v in s["alpha"] + s["sat"] + [s["s_t"], s["rms_t"], s["rms0"]])
    # the float32 restatement against the fp64 one on well-conditioned rows: a handful of float32
    # operations per scalar (each 2^-24) behind float32 sums over about a thousand terms: within
    # 64 x 2^-24 relative, alpha, mod and the DAG blob alike
    adv = P.head_data(1025)["advantages"]
    c64, c32 = A.controller(adv, p, state), A.controller(adv, p, state, torch.float32)
    rel = 64 * 2.0 ** -24
    assert abs(c32["alpha"] - c64["alpha"]) <= rel * c64["alpha"] and abs(c32["count"] - c64["count"]) <= max(1, c64["band"])
    m64, m32 = A.modulate(adv, p, c64["alpha"])[0], A.modulate(adv, p, c64["alpha"], torch.float32)[0]
    assert (m32.double() - m64).abs().max() <= rel * m64.abs().max()
    g = [torch.randn(96, generator=torch.Generator().manual_seed(i)) for i in range(1, 5)]
    s64, s32 = A.dag_steps(blob, g, h, c, segs), A.dag_steps(blob, g, h, c, segs, torch.float32)
    for a, b in zip(s64, s32):
        assert (b["blob"].double() - a["blob"]).abs().max() <= rel * a["blob"].abs().max()
        assert np.allclose(b["alpha"], a["alpha"], rtol=rel, atol=0) and abs(b["s_t"] - a["s_t"]) <= rel


def test_planted_defects_move_a_checked_quantity_past_its_allowance():
    """The checker has teeth at the inputs the GPU tests use: each planted mistake, taken as "the
    kernel", misses the 4 x rule (or the exact count) against the fp64 restatement."""
    p, h = A.dynago(), P.hyper(ent_coef=0.01, lr=0.0)
    state = (1.0, A.as_f32(0.1))
    adv = P.head_data(1025)["advantages"]
    ref, t32 = A.controller(adv, p, state), A.controller(adv, p, state, torch.float32)
    # eps added to sigma once instead of twice: alpha
    bad = A.controller(adv, p, state, defect="eps_once")
    err, allow = A.rule(bad["alpha"], ref["alpha"], t32["alpha"])
    assert err > allow, (err, allow)
    # the saturation EMA formed with the old alpha: the count is off by more than the band admits
    # (on the second update in a row, as the GPU test makes it: after the first, alpha is 7 and no
    # |Z| of normal advantages reaches tau with either alpha)
    second = (ref["alpha"], ref["sat"])
    ref2, bad = A.controller(adv, p, second), A.controller(adv, p, second, defect="old_alpha_sat")
    assert ref2["count"] > 0 and ref2["band"] < 1e-3 * adv.numel() and abs(bad["count"] - ref2["count"]) > ref2["band"]
    # the normalised mod in the value target: d_values and the value loss
    d = P.head_data(257)
    r64, r32 = A.head_autograd(d, h, p, ref["alpha"], True), A.head_autograd(d, h, p, ref["alpha"], True, torch.float32)
    bad = A.head_autograd(d, h, p, ref["alpha"], True, defect="normalized_target")
    for got, want, t in ((bad["d_values"], r64["d_values"], r32["d_values"]),
                         (bad["stats"][1], r64["stats"][1], r32["stats"][1])):
        err, allow = A.rule(got, want, t)
        assert err > allow, (err, allow)
    # DAG's saturation divided by the padded length: a head's sat_s at a sampled step
    k, dd, pi_w, vf_w, _ = policy_ref.MATRIX["G"]
    desc = abi.policy_desc(k, dd, pi_w, vf_w)
    segs = abi.policy_segments(desc)
    from f16_jsb_amd.policy import pack_blob
    blob = pack_blob(desc, *G.tanh_data(k, dd, pi_w, vf_w, 1, seed=1)[0])
    hh, c = P.hyper(), A.dag_constants(warmup_steps=2, sat_every=2)
    grads = A.dag_gradients(desc, k, dd, pi_w, vf_w, hh)
    good, bad = A.dag_steps(blob, grads, hh, c, segs), A.dag_steps(blob, grads, hh, c, segs, defect="padded_sat")
    padded = [i for i, (_, n, cnt) in enumerate(segs) if n != cnt]
    assert padded and any(good[s]["sat"][i] != bad[s]["sat"][i] for s in range(len(grads)) for i in padded)
