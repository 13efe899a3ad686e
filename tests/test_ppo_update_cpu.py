"""CPU checks of the device PPO update (f16env_ppo_loss_head, f16env_ppo_adam_step, still ABI 7):
the host side of the new entry points without a device (symbols, workspace size, argument
validation), the checkers of tests/ppo_ref.py against torch's fp64 autograd and torch's Adam, and
DevicePPO's refusal of a CPU policy."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import policy_grad_ref as G
import policy_ref
import ppo_ref as P
from f16_jsb_amd import abi

NEW = ("f16env_ppo_workspace", "f16env_ppo_head_blocks", "f16env_ppo_loss_head", "f16env_ppo_adam_step")
SIZES = (1, 2, 129, 257, 1031)


@pytest.fixture(scope="module")
def L():
    from f16_jsb_amd.build import build
    build()
    from f16_jsb_amd import _lib
    return _lib.lib()


def test_library_exports_the_ppo_symbols(L):
    from f16_jsb_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "f16env.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
        assert getattr(L, name).restype is ctypes.c_int and getattr(L, name).argtypes
    assert "#define F16ENV_ABI_VERSION 7" in header
    assert L.f16env_abi_version() == abi.F16ENV_ABI_VERSION == 7
    assert "#define F16_PPO_NORMALIZE_ADV 0x%x" % abi.F16_PPO_NORMALIZE_ADV in header
    for i, key in enumerate(abi.PPO_HYPER):
        assert "#define F16_PPO_HYPER_%s %d" % (key.upper(), i) in header
    assert abi.PPO_HYPER == P.HYPER and abi.PPO_STATS[:6] == P.STATS
    assert "#define F16_PPO_N_HYPER %d" % len(abi.PPO_HYPER) in header
    assert "#define F16_PPO_N_STATS %d" % len(abi.PPO_STATS) in header
    import f16_jsb_amd
    from f16_jsb_amd.ppo import DevicePPO
    assert f16_jsb_amd.DevicePPO is DevicePPO and "DevicePPO" in f16_jsb_amd.__all__


def _workspace(L, n, max_blocks):
    out, blocks = ctypes.c_int64(-1), ctypes.c_int32(-1)
    assert L.f16env_ppo_workspace(n, max_blocks, ctypes.byref(out)) == 0
    assert L.f16env_ppo_head_blocks(n, max_blocks, ctypes.byref(blocks)) == 0
    assert out.value == (8 * (4 + 8 * blocks.value) if n else 0)
    return out.value, blocks.value


def test_workspace_is_monotone_and_needs_no_device(L):
    """One set of eight doubles per block of 256 rows behind a header of four; the grid is
    min(ceil(n / 256), max_blocks or 256); monotone in n and in max_blocks; 0 for n = 0."""
    assert _workspace(L, 0, 0) == (0, 0)
    for n, want in ((1, 1), (256, 1), (257, 2), (1031, 5), (65536, 256), (1 << 30, 256)):
        assert _workspace(L, n, 0)[1] == want, n
    assert [_workspace(L, 1031, mb)[1] for mb in range(1, 8)] == [1, 2, 3, 4, 5, 5, 5]
    assert _workspace(L, 1 << 20, 1000)[1] == 1000
    for mb in (0, 1, 2, 7):
        sizes = [_workspace(L, n, mb)[0] for n in range(0, 3000, 37)]
        assert sizes == sorted(sizes), mb
    for n in (1, 257, 70000):
        sizes = [_workspace(L, n, mb)[0] for mb in range(1, 300)]
        assert sizes == sorted(sizes), n


def test_bad_arguments_return_errors_without_a_device(L):
    out, blocks = ctypes.c_int64(0), ctypes.c_int32(0)
    ws_fn, bl_fn, head, adam = (getattr(L, name) for name in NEW)
    assert ws_fn(-1, 0, ctypes.byref(out)) < 0 and b"n must be" in L.f16env_last_error()
    assert ws_fn(4, -1, ctypes.byref(out)) < 0 and b"max_blocks" in L.f16env_last_error()
    assert ws_fn(4, 0, None) < 0
    assert bl_fn(-1, 0, ctypes.byref(blocks)) < 0 and bl_fn(4, -1, ctypes.byref(blocks)) < 0 and bl_fn(4, 0, None) < 0
    A = 4096  # a non-NULL, 16-B aligned stand-in address (never dereferenced: the call is refused first)
    big = 1 << 20
    # f16env_ppo_loss_head(stream, n, mean, values, actions, old_log_prob, advantages, target_values, log_std, hyper,
    #                      flags, max_blocks, workspace, workspace_bytes, d_mean, d_values)
    good = [None, 4, A, A, A, A, A, A, A, A, 1, 0, A, big, A, A]

    def head_with(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return head(*a)
    assert head_with(_1=-1) < 0 and b"n must be" in L.f16env_last_error()
    assert head_with(_11=-1) < 0 and b"max_blocks" in L.f16env_last_error()
    assert head_with(_10=2) < 0 and b"flags" in L.f16env_last_error()
    for i in (2, 3, 4, 5, 6, 7, 8, 9, 12, 14, 15):                               # every pointer NULL
        assert head_with(**{"_%d" % i: None}) < 0 and b"null" in L.f16env_last_error(), i
    for i in (2, 4, 14):                                                         # 16-B: mean, actions, d_mean
        assert head_with(**{"_%d" % i: A + 4}) < 0 and b"aligned" in L.f16env_last_error(), i
    for i in (3, 5, 6, 7, 8, 9, 15):                                             # float-aligned
        assert head_with(**{"_%d" % i: A + 2}) < 0 and b"aligned" in L.f16env_last_error(), i
    assert head_with(_12=A + 4) < 0 and b"aligned" in L.f16env_last_error()      # workspace: 8-B
    assert head_with(_1=257, _13=_workspace(L, 257, 0)[0] - 1) < 0 and b"workspace" in L.f16env_last_error()
    assert head_with(_1=0, _2=None) == 0                                         # n = 0: nothing is looked at
    # f16env_ppo_adam_step(stream, n_floats, blob, grad_blob, exp_avg, exp_avg_sq, step, hyper, log_std_offset,
    #                      head_workspace, head_blocks, stats)
    good_a = [None, 64, A, A, A, A, A, A, 60, A, 1, A]

    def adam_with(**kw):
        a = list(good_a)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return adam(*a)
    assert adam_with(_1=-1) < 0 and b"n_floats" in L.f16env_last_error()
    for i in (2, 3, 4, 5, 6, 7):
        assert adam_with(**{"_%d" % i: None}) < 0 and b"null" in L.f16env_last_error(), i
        assert adam_with(**{"_%d" % i: A + 2}) < 0 and b"aligned" in L.f16env_last_error(), i
    assert adam_with(_11=A + 2) < 0 and b"aligned" in L.f16env_last_error()      # stats
    assert adam_with(_9=A + 4) < 0 and b"aligned" in L.f16env_last_error()       # head workspace: 8-B
    assert adam_with(_10=0) < 0 and b"head_blocks" in L.f16env_last_error()
    assert adam_with(_8=-1) < 0 and adam_with(_8=61) < 0 and b"log_std_offset" in L.f16env_last_error()
    assert adam_with(_1=0, _2=None) == 0                                         # n_floats = 0: a no-op


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_closed_form_head_equals_fp64_autograd(n, normalize):
    """On the generator's data the closed form of include/f16env.h equals torch's fp64 autograd of
    policy_grad_ref.ppo_loss over the leaves (mean, values, log_std) to 1e-12 relative, the clipped
    rows' d_mean are exactly 0 in both -- and without the clip mask it does not agree: the data
    exercises the clip."""
    d = P.head_data(n)
    h = P.hyper(ent_coef=0.01)
    got, want = P.head_closed_form(d, h, normalize), P.head_autograd(d, h, normalize)
    for key in ("d_mean", "d_values", "d_log_std", "stats"):
        scale = want[key].abs().max().item()
        assert (got[key] - want[key]).abs().max().item() <= 1e-12 * scale, key
    clipped = got["clipped"]
    assert torch.equal(clipped, (want["d_mean"] == 0).all(dim=1))
    assert (got["d_mean"][clipped] == 0).all() and (got["d_mean"][~clipped] != 0).all()
    assert got["stats"][5].item() == ((d["ratio64"] - 1).abs() > h["clip_range"]).double().mean().item()
    if n >= 129:
        assert 0.2 * n < int(clipped.sum()) < 0.8 * n
        loose = P.head_closed_form(d, h, normalize, clip_mask=False)
        for key in ("d_mean", "d_log_std"):
            assert (loose[key] - want[key]).abs().max().item() > 1e-3 * want[key].abs().max().item(), key


def test_planted_ratios_are_the_fp64_ratios():
    d = P.head_data(1031)
    nearest = np.abs(d["ratio64"].numpy()[None, :] / np.array(P.RATIOS)[:, None] - 1.0).min(axis=0)
    assert nearest.max() <= 0.01 + 1e-5
    assert all((np.abs(d["ratio64"].numpy() / r - 1.0) <= 0.0101).any() for r in P.RATIOS)


@pytest.mark.parametrize("case", ["G", "F"])
def test_fp64_adam_reference_against_torch_adam(case):
    """Three clipped Adam steps (the gradient's norm once below and twice above max_grad_norm) on a
    packed blob: torch's float32 result sits within the 4 x rule of the fp64 reference per parameter
    tensor (its own error against its own allowance: the reference and the rule agree with torch),
    the pads stay all-bits zero, and the two clipped steps really were clipped."""
    from f16_jsb_amd.policy import pack_blob, unpack_blob
    k, d, pi_w, vf_w, _ = policy_ref.MATRIX[case]
    desc = abi.policy_desc(k, d, pi_w, vf_w)
    h = P.hyper()
    blob = pack_blob(desc, *G.tanh_data(k, d, pi_w, vf_w, 1, seed=1)[0])
    grads = P.adam_gradients(desc, k, d, pi_w, vf_w, h)
    norms = [g.double().norm().item() for g in grads]
    assert norms[0] < h["max_grad_norm"] < min(norms[1:])
    ref, t32 = P.adam_ref64(blob, grads, h), P.adam_torch32(blob, grads, h)
    zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, blob.numpy())["zero"]
    for step in range(3):
        for which, name in enumerate(("blob", "exp_avg", "exp_avg_sq")):
            rounded = ref[step][which].float()
            rules = G.rule_of_four(unpack_blob(desc, rounded), unpack_blob(desc, ref[step][which]),
                                   unpack_blob(desc, t32[step][which]))
            for tensor, (err, allow) in rules.items():
                assert err <= allow, (step, name, tensor, err, allow)
            assert np.all(t32[step][which].numpy()[zero].view(np.uint32) == 0)
            assert np.all(ref[step][which].numpy()[zero] == 0)
    assert not torch.equal(ref[2][0].float(), blob)


def test_device_ppo_refuses_a_cpu_policy():
    from f16_jsb_amd._lib import F16EnvError
    from f16_jsb_amd.policy import DevicePolicy
    from f16_jsb_amd.ppo import DevicePPO
    net = G.tanh_data(4, 15, [64, 64], [64, 64], 1)[0]
    pol = DevicePolicy.from_layers(*net, stack_k=4, device="cpu")
    with pytest.raises(F16EnvError, match="no fallback"):
        DevicePPO(pol)
