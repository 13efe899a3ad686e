"""CPU checks of the device policy's backward (f16env_policy_backward, still ABI 7): the checkers
of tests/policy_grad_ref.py against each other, unpack_blob / state_dict, the optimiser on the
packed blob against the optimiser on the layers, and the host side of the two new entry points
(symbols, workspace size, argument validation, the LDS rule) without a device."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import policy_grad_ref as G
import policy_ref
from f16_jsb_amd import abi

MATRIX = policy_ref.MATRIX
CASES = [pytest.param(*c[:4], id=name) for name, c in MATRIX.items()]
N_INT = 257


@pytest.fixture(scope="module")
def L():
    from f16_jsb_amd.build import build
    build()
    from f16_jsb_amd import _lib
    return _lib.lib()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("k,d,pi_w,vf_w", CASES)
def test_integer_reference_equals_fp64_autograd(k, d, pi_w, vf_w):
    """On the generator's data (which asserts the 2^24 condition and the zero / negative
    pre-activations itself, at the GPU test's largest n) the exact integer vjp equals torch's fp64
    autograd element for element, every parameter tensor's gradient is alive, and so do the two
    with one upstream gradient absent."""
    net, obs, d_mean, d_values = G.int_data(k, d, pi_w, vf_w, N_INT)
    for dm, dv in ((d_mean, d_values), (None, d_values), (d_mean, None)):
        want = G.named_tensors(G.int_vjp(net, obs.numpy(), None if dm is None else dm.numpy(),
                                         None if dv is None else dv.numpy())[0])
        got = G.named_tensors(G.vjp(net, obs, dm, dv, "relu"))
        for (name, w), (_, g) in zip(want, got):
            assert np.array_equal(np.asarray(w, np.float64), g.numpy()), name
            alive = name != "log_std" and (dm is not None or name[:2] not in ("pi", "ac")) \
                and (dv is not None or name[:2] not in ("vf", "va"))
            assert bool(np.any(np.asarray(w) != 0)) == alive, name
    # and the packed reference is exact in float32
    desc = abi.policy_desc(k, d, pi_w, vf_w, "relu")
    ref = G.int_vjp(net, obs.numpy(), d_mean.numpy(), d_values.numpy())[0]
    blob = G.pack(desc, ref).numpy()
    u = policy_ref.unpack_blob(k, d, pi_w, vf_w, blob)
    assert np.array_equal(u["pi"][0][0].astype(np.int64), ref[0][0][0]) and np.all(blob[u["zero"]] == 0)


@pytest.mark.parametrize("k,d,pi_w,vf_w", CASES)
def test_unpack_blob_inverts_pack_blob(k, d, pi_w, vf_w):
    from f16_jsb_amd.policy import pack_blob, unpack_blob
    net = G.tanh_data(k, d, pi_w, vf_w, 1)[0]
    desc = abi.policy_desc(k, d, pi_w, vf_w)
    blob = pack_blob(desc, *net)
    got = unpack_blob(desc, blob)
    u = policy_ref.unpack_blob(k, d, pi_w, vf_w, blob.numpy())
    theirs = (u["pi"], u["vf"], u["act_head"], u["val_head"], u["log_std"])
    for (name, g), (_, w), (_, t) in zip(G.named_tensors(got), G.named_tensors(net), G.named_tensors(theirs)):
        assert _bits_equal(g.numpy(), w.numpy()) and _bits_equal(g.numpy(), t), name
    assert torch.equal(pack_blob(desc, *got), blob)
    with pytest.raises(ValueError):
        unpack_blob(desc, blob[:-1])


def test_state_dict_carries_sb3_key_names():
    from f16_jsb_amd.policy import DevicePolicy, layers_from_state_dict
    net = G.tanh_data(4, 15, [32, 96, 64], [128, 64], 1)[0]
    pol = DevicePolicy.from_layers(*net, stack_k=4, device="cpu")
    sd = pol.state_dict()
    want = {"log_std", "action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias"}
    want |= {"mlp_extractor.policy_net.%d.%s" % (i, p) for i in (0, 2, 4) for p in ("weight", "bias")}
    want |= {"mlp_extractor.value_net.%d.%s" % (i, p) for i in (0, 2) for p in ("weight", "bias")}
    assert set(sd) == want
    for (name, g), (_, w) in zip(G.named_tensors(layers_from_state_dict(sd)), G.named_tensors(net)):
        assert _bits_equal(g.numpy(), w.numpy()), name
    assert torch.equal(DevicePolicy.from_state_dict(sd, stack_k=4, device="cpu").blob, pol.blob)
    assert pol.parameters()[0] is pol.blob and not pol.blob.requires_grad
    assert pol.requires_grad_() is pol and pol.blob.requires_grad and pol.blob.is_leaf
    pol.load(*net)  # legal on a leaf that requires grad


@pytest.mark.parametrize("k,d,pi_w,vf_w", [CASES[1], CASES[3], CASES[8]])
def test_adam_on_the_blob_is_adam_on_the_layers(k, d, pi_w, vf_w):
    """Three Adam steps on the packed blob and on the unpacked layers with the unpacked gradient:
    bit-equal layers, pads still exactly 0. The float64 norm of the packed gradient is that of the
    pieces (clip_grad_norm_ forms its float32 norm in another order on one tensor than on many, so
    its scale factor may differ in the last bit: the same clipping, not the same bits)."""
    from f16_jsb_amd.policy import pack_blob, unpack_blob
    desc = abi.policy_desc(k, d, pi_w, vf_w)
    blob = pack_blob(desc, *G.tanh_data(k, d, pi_w, vf_w, 1, seed=1)[0]).requires_grad_(True)
    layers = [t.clone().requires_grad_(True) for _, t in G.named_tensors(unpack_blob(desc, blob))]
    zero = policy_ref.unpack_blob(k, d, pi_w, vf_w, blob.detach().numpy())["zero"]
    opt_b = torch.optim.Adam([blob], lr=3e-4, eps=1e-5)
    opt_l = torch.optim.Adam(layers, lr=3e-4, eps=1e-5)
    for step in range(3):
        grad = pack_blob(desc, *G.tanh_data(k, d, pi_w, vf_w, 1, seed=2 + step)[0])  # blob layout, zero pads
        pieces = [t for _, t in G.named_tensors(unpack_blob(desc, grad))]
        norm_b = grad.double().norm().item()
        norm_l = torch.sqrt(sum(p.double().pow(2).sum() for p in pieces)).item()
        assert abs(norm_b - norm_l) <= 1e-12 * norm_l
        blob.grad = grad.clone()
        for t, p in zip(layers, pieces):
            t.grad = p.clone()
        opt_b.step()
        opt_l.step()
        for (name, g), t in zip(G.named_tensors(unpack_blob(desc, blob)), layers):
            assert _bits_equal(g.numpy(), t.detach().numpy()), (step, name)
        assert np.all(blob.detach().numpy()[zero].view(np.uint32) == 0)
    assert not torch.equal(blob.detach(), pack_blob(desc, *G.tanh_data(k, d, pi_w, vf_w, 1, seed=1)[0]))


def test_library_exports_the_backward_symbols(L):
    from f16_jsb_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "f16env.h")).read()
    for name in ("f16env_policy_backward_workspace", "f16env_policy_backward"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert "#define F16ENV_ABI_VERSION 7" in header
    assert L.f16env_abi_version() == abi.F16ENV_ABI_VERSION == 7


def _workspace(L, desc, n, max_blocks):
    out = ctypes.c_int64(-1)
    assert L.f16env_policy_backward_workspace(ctypes.byref(desc), n, max_blocks, ctypes.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("k,d,pi_w,vf_w", CASES)
def test_workspace_size_and_waves_per_block(L, k, d, pi_w, vf_w):
    """The workspace function needs no device; it holds one partial gradient per wave of the grid
    (the waves per block as policy_grad_ref.backward_waves states them, whose images fit 160 KiB),
    is monotone in max_blocks up to the grid and constant past it, and 0 for n = 0."""
    desc = abi.policy_desc(k, d, pi_w, vf_w)
    nf = abi.policy_blob_layout(desc)[1]
    waves, per_wave = G.backward_waves(k, d, pi_w, vf_w)
    assert waves in (1, 2, 4) and waves * per_wave <= G.LDS_BYTES and (waves == 4 or 2 * waves * per_wave > G.LDS_BYTES)
    assert _workspace(L, desc, 1 << 20, 1) == waves * nf * 4
    n = 257
    grid = -(-9 // waves)
    sizes = [_workspace(L, desc, n, mb) for mb in range(1, grid + 3)]
    assert sizes == [min(mb, grid) * waves * nf * 4 for mb in range(1, grid + 3)]
    assert _workspace(L, desc, n, 0) == sizes[-1] and _workspace(L, desc, 0, 0) == 0
    assert _workspace(L, desc, 1 << 20, 0) == 256 * waves * nf * 4  # the default grid limit


def test_one_wave_fits_for_every_descriptor():
    """The largest images any accepted descriptor has (K = 10, D = 17, three layers of 128 per
    branch) fit one wave, so the entry point's 'does not fit' error is unreachable."""
    waves, per_wave = G.backward_waves(10, 17, [128] * 3, [128] * 3)
    assert waves == 1 and per_wave == 4 * 33 * (170 + 384 + 128) <= G.LDS_BYTES
    assert G.backward_waves(*MATRIX["D"][:4]) == (2, 4 * 33 * (170 + 192 + 128))
    for k in range(1, 11):
        for d in (15, 17):
            assert G.backward_waves(k, d, [128] * 3, [128] * 3)[0] >= 1


def test_backward_bad_arguments_return_errors_without_a_device(L):
    good = abi.policy_desc(4, 15, [64, 64], [64, 64])
    g = ctypes.byref(good)
    out = ctypes.c_int64(0)
    ws_fn, bwd = L.f16env_policy_backward_workspace, L.f16env_policy_backward
    assert ws_fn(None, 4, 0, ctypes.byref(out)) < 0
    assert ws_fn(g, -1, 0, ctypes.byref(out)) < 0
    assert ws_fn(g, 4, -1, ctypes.byref(out)) < 0 and b"max_blocks" in L.f16env_last_error()
    assert ws_fn(g, 4, 0, None) < 0
    A = 4096  # a non-NULL, 16-B aligned stand-in address (never dereferenced: the call is refused first)
    big = 1 << 30
    for kw in (dict(K=0), dict(D=16), dict(n_pi=0), dict(n_vf=4), dict(activation=2)):
        bad = abi.policy_desc(4, 15, [64, 64], [64, 64])
        for key, v in kw.items():
            setattr(bad, key, v)
        assert ws_fn(ctypes.byref(bad), 4, 0, ctypes.byref(out)) < 0
        assert bwd(None, ctypes.byref(bad), A, 4, A, 60, 15, A, A, A, big, 0, A) < 0
        assert L.f16env_last_error()
    assert bwd(None, None, A, 4, A, 60, 15, A, A, A, big, 0, A) < 0            # no descriptor
    assert bwd(None, g, A, -1, A, 60, 15, A, A, A, big, 0, A) < 0              # n < 0
    assert b"n must be" in L.f16env_last_error()
    assert bwd(None, g, A, 4, A, 60, 15, A, A, A, big, -1, A) < 0              # max_blocks < 0
    assert bwd(None, g, None, 4, A, 60, 15, A, A, A, big, 0, A) < 0            # blob
    assert bwd(None, g, A, 4, None, 60, 15, A, A, A, big, 0, A) < 0            # obs
    assert bwd(None, g, A, 4, A, 60, 15, A, A, None, big, 0, A) < 0            # workspace
    assert bwd(None, g, A, 4, A, 60, 15, A, A, A, big, 0, None) < 0            # grad_blob
    assert bwd(None, g, A, 4, A, 60, 15, None, None, A, big, 0, A) < 0         # both upstream gradients NULL
    assert b"both NULL" in L.f16env_last_error()
    assert bwd(None, g, A + 4, 4, A, 60, 15, A, A, A, big, 0, A) < 0           # blob not 16-B aligned
    assert b"aligned" in L.f16env_last_error()
    assert bwd(None, g, A, 4, A, 60, 15, A + 4, A, A, big, 0, A) < 0           # d_mean not 16-B aligned
    assert bwd(None, g, A, 4, A, 60, 15, A, A + 2, A, big, 0, A) < 0           # d_values not float-aligned
    assert bwd(None, g, A, 4, A, 60, 15, A, A, A + 8, big, 0, A) < 0           # workspace not 16-B aligned
    assert bwd(None, g, A, 4, A, 60, 15, A, A, A, big, 0, A + 4) < 0           # grad_blob not 16-B aligned
    assert bwd(None, g, A, 4, A + 2, 60, 15, A, A, A, big, 0, A) < 0           # obs not float-aligned
    assert bwd(None, g, A, 4, A, -1, 15, A, A, A, big, 0, A) < 0               # negative strides
    assert bwd(None, g, A, 4, A, 60, -1, A, A, A, big, 0, A) < 0
    need = _workspace(L, good, 4, 0)
    assert bwd(None, g, A, 4, A, 60, 15, A, A, A, need - 1, 0, A) < 0          # workspace too small
    assert b"workspace" in L.f16env_last_error()
