"""CPU checks of the device LMA policy's eval-mode backward (f16env_policy_lma_backward, still ABI
7): the restatement of tests/lma_grad_ref.py against lma_ref, the precision rule's condition on
the matrix, the negative controls, the host side of the two new entry points without a device (the
workspace size, the budget rule, argument validation) and the opt-in class on the CPU."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import lma_grad_ref as G
import lma_ref

MATRIX = lma_ref.MATRIX
R_CAP = 3.0   # a condition on the test data, not a tolerance: where a case exceeds it, its seed changes (UPSTREAM_SEED)


@pytest.fixture(scope="module")
def L():
    from f16_jsb_amd.build import build
    build()
    from f16_jsb_amd import _lib
    return _lib.lib()


def _layers(net):
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))  # noqa: E731
    pair = lambda wb: (t(wb[0]), t(wb[1]))  # noqa: E731
    ext = {"embed": pair(net["embed"]), "embed2": pair(net["embed2"]),
           "blocks": [{k: pair(v) for k, v in blk.items()} for blk in net["blocks"]]}
    return ext, [pair(l) for l in net["pi"]], [pair(l) for l in net["vf"]], pair(net["act"]), pair(net["val"]), t(net["log_std"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_equals_lma_ref_bit_for_bit(dtype):
    """The restatement over torch parameters computes lma_ref.forward's features, means and values
    on case S (65 rows) bit for bit, in fp64 and in float32."""
    net = lma_ref.random_net("S")
    x, eps = lma_ref.shared_inputs("S")
    act, hs = MATRIX["S"][6:8]
    ref = lma_ref.forward(net, x[:65], eps[:65], dtype, act, hs)
    f, mean, values = G.forward(G.leaves(net, dtype), x[:65], dtype, act, hs)
    for got, want in ((f, ref[0]), (mean, ref[4]), (values, ref[2])):
        got = got.detach().numpy()
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("name", list(MATRIX))
def test_reorder_ratio_within_the_cap(name):
    """r of every matrix case at 257 rows (the float32 restatement summed in the other order against
    the allowance base) stays within the cap, every gradient is finite and every tensor's is alive.
    r depends on the host's float32 BLAS as well as on the data (not on its thread count), so every
    case has its own upstream seed (lma_grad_ref.UPSTREAM_SEED) with r below 2 under two BLAS builds. Where a case
    exceeds the cap its seed changes, not the cap."""
    rule = G.case_rule(name)
    print("%s: r %.2f (%s) F %.2f" % (name, rule.r, max(rule.flip_ratio, key=rule.flip_ratio.get), rule.F))
    assert rule.finite and rule.r <= R_CAP and rule.F == max(4.0, 2.0 * rule.r)
    for tname, t in G.named_tensors(rule.ref64):
        assert float(t.abs().max()) > 0, tname


@pytest.mark.parametrize("kind", lma_ref.STRESS)
def test_stress_inputs_have_finite_gradients(kind):
    rule = G.stress_rule(kind)
    print("%s: r %.2f F %.2f" % (kind, rule.r, rule.F))
    assert rule.finite


@pytest.mark.parametrize("wrong", [w for w in G.WRONG if w != "perm_untransposed"])
def test_planted_wrong_derivatives_exceed_the_allowance(wrong):
    """Each planted wrong derivative, in fp64 (no rounding to hide behind), exceeds case S's
    allowance on at least one tensor."""
    rule = G.case_rule("S")
    net, obs, d_mean, d_values, act, hs = G.case_input("S")
    bad = {n: e / a for n, (e, a) in rule.check(G.vjp(net, obs, d_mean, d_values, torch.float64, act, hs, wrong=wrong)).items()}
    worst = max(bad, key=bad.get)
    print("%s: %.3g x the allowance on %s" % (wrong, bad[worst], worst))
    assert bad[worst] > 1.0


def test_untransposed_permutation_exceeds_the_allowance():
    """The stacking permutation applied forward in the backward (instead of its transpose). Case
    S's own permutation (K = 4, heads_stacking 4) swaps the two indices of a 4 x 4 grid, so it is
    its own inverse and no test on S as it stands can see this defect (asserted). The control
    therefore runs on case S's net and rows at heads_stacking 2 (dk 32), where the permutation is
    not an involution, against that input's own allowance, and on case R."""
    idx = lma_ref.flat_index(4, 64, 4).reshape(-1)
    assert np.array_equal(idx[idx], np.arange(idx.size))
    net, obs, d_mean, d_values, act, _ = G.case_input("S")
    idx2 = lma_ref.flat_index(4, 64, 2).reshape(-1)
    assert not np.array_equal(idx2[idx2], np.arange(idx2.size))
    rule = G.Rule(net, obs, d_mean, d_values, act, 2)
    assert rule.r <= R_CAP
    bad = {n: e / a for n, (e, a) in rule.check(G.vjp(net, obs, d_mean, d_values, torch.float64, act, 2,
                                                        wrong="perm_untransposed")).items()}
    assert max(bad.values()) > 1.0
    rule, (net, obs, d_mean, d_values, act, hs) = G.case_rule("R"), G.case_input("R")
    bad = {n: e / a for n, (e, a) in rule.check(G.vjp(net, obs, d_mean, d_values, torch.float64, act, hs,
                                                        wrong="perm_untransposed")).items()}
    assert max(bad.values()) > 1.0


def test_integer_gradients_are_exact_in_float32():
    """The guard of the GPU's exact test: for every K and stacking the largest sum of magnitudes
    behind any forward value or gradient element stays below 2^24, the fp64 gradient is made of
    integers, and every weight's gradient is alive."""
    worst = 0
    for k in range(1, 11):
        for hs in lma_ref.STACKINGS:
            g, peak = G.int_vjp(k, hs)
            worst = max(worst, peak)
            assert peak < G.EXACT, (k, hs, peak)
            for name, t in G.named_tensors(g):
                assert bool((t == t.round()).all()), (k, hs, name)
                assert float(t.abs().max()) > 0 or not name.endswith(".weight"), (k, hs, name)
    print("largest sum of magnitudes: %d" % worst)


def test_pack_and_unpack_are_inverse_and_name_the_untrained_positions():
    desc, lma = G.descriptors(*MATRIX["S"][:8])
    g = G.case_rule("S").t32
    blob = G.pack(desc, lma, g)
    for (name, a), (_, b) in zip(G.named_tensors(G.unpack(desc, lma, blob)), G.named_tensors(g)):
        assert torch.equal(a, b), name
    mask = G.untrained_positions(desc, lma)
    assert not blob.numpy()[mask].any()
    from f16_jsb_amd.abi import F16_LMA_OFF_PE, F16_POLICY_OFF_LOG_STD, lma_blob_layout
    off, total = lma_blob_layout(desc, lma)
    assert mask.size == total and mask[off[F16_POLICY_OFF_LOG_STD]:off[F16_POLICY_OFF_LOG_STD] + 4].all()
    assert mask[off[F16_LMA_OFF_PE]:off[F16_LMA_OFF_PE] + 4 * 64].all()


# ---------------------------------------------------------------------------------------------
# the host side, without a device
def _workspace(L, desc, lma, n, max_blocks):
    out = ctypes.c_int64(-1)
    assert L.f16env_policy_lma_backward_workspace(ctypes.byref(desc), ctypes.byref(lma), n, max_blocks, ctypes.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("name", list(MATRIX))
def test_workspace_size_and_budget_rule(L, name):
    """The workspace function needs no device and accepts every matrix case; its size is the
    documented one (per block the blob's floats and a checkpoint per extractor block), monotone in n
    and in max_blocks; the documented LDS budget fits 160 KiB for the case. What this file can hold
    the budget rule against is the library's verdict -- every matrix case is accepted, and the rule's
    bytes fit; the launch's dynamic LDS size itself is not observable through the ABI, so a launcher
    that under-sized it would be caught by tests/test_gpu_lma_backward.py, not here. The slot's
    checkpoint floats (n_layers x L_new images of 32 x 33), which follow from the same image size, are
    compared exactly."""
    k, d, nl, ff, pi_w, vf_w, act, hs, _ = MATRIX[name]
    desc, lma = G.descriptors(k, d, nl, ff, pi_w, vf_w, act, hs)
    assert G.backward_lds(k, nl, pi_w, vf_w) <= G.LDS_BYTES
    for n, mb in ((0, 0), (1, 0), (257, 0), (257, 1), (257, 3), (1 << 20, 0), (1 << 20, 7)):
        assert _workspace(L, desc, lma, n, mb) == G.workspace_bytes(k, nl, ff, pi_w, vf_w, n, mb), (n, mb)
    by_n = [_workspace(L, desc, lma, n, 0) for n in (0, 1, 32, 33, 257, 4096, 8192, 8193, 1 << 20)]
    assert by_n == sorted(by_n) and by_n[0] == 0
    by_mb = [_workspace(L, desc, lma, 1 << 20, mb) for mb in (1, 2, 3, 64, 256, 1000)]
    assert by_mb == sorted(by_mb)


def test_budget_rule_at_its_corners():
    """The budget rule over the whole lattice the forward accepts: the largest block is L_new = 5
    with blocks (38 images, 160 512 B), within 160 KiB, so 'does not fit' is unreachable."""
    worst = max(G.backward_lds(k, nl, [128] * 3, [128] * 3) for k in range(1, 11) for nl in range(4))
    assert worst == 38 * G.IMAGE_BYTES == 160512 <= G.LDS_BYTES
    assert G.backward_lds(10, 2, [64, 64], [128, 64]) == 160512     # case R
    assert G.backward_lds(3, 0, [64], [64]) == 2 * G.IMAGE_BYTES + (3 * 64 * 33 + 608) * 4 + 2 * G.IMAGE_BYTES  # case W


def test_backward_bad_arguments_return_errors_without_a_device(L):
    desc, lma = G.descriptors(*MATRIX["S"][:8])
    g, m = ctypes.byref(desc), ctypes.byref(lma)
    out = ctypes.c_int64(0)
    ws_fn, bwd = L.f16env_policy_lma_backward_workspace, L.f16env_policy_lma_backward
    assert ws_fn(None, m, 4, 0, ctypes.byref(out)) < 0
    assert ws_fn(g, None, 4, 0, ctypes.byref(out)) < 0
    assert ws_fn(g, m, -1, 0, ctypes.byref(out)) < 0
    assert ws_fn(g, m, 4, -1, ctypes.byref(out)) < 0 and b"max_blocks" in L.f16env_last_error()
    assert ws_fn(g, m, 4, 0, None) < 0
    bad, _ = G.descriptors(*MATRIX["S"][:8])
    bad.n_pi = 0
    assert ws_fn(ctypes.byref(bad), m, 4, 0, ctypes.byref(out)) < 0
    _, badm = G.descriptors(*MATRIX["S"][:8])
    badm.L_new = 3
    assert ws_fn(g, ctypes.byref(badm), 4, 0, ctypes.byref(out)) < 0 and b"L_new" in L.f16env_last_error()
    A, big = 4096, 1 << 30  # a non-NULL, 16-B aligned stand-in address (never dereferenced: the call is refused first)
    assert bwd(None, g, m, A, -1, A, 60, 15, A, A, A, big, 0, A) < 0 and b"n must be" in L.f16env_last_error()
    assert bwd(None, g, m, A, 4, A, 60, 15, A, A, A, big, -1, A) < 0
    assert bwd(None, None, m, A, 4, A, 60, 15, A, A, A, big, 0, A) < 0
    assert bwd(None, g, None, A, 4, A, 60, 15, A, A, A, big, 0, A) < 0
    assert bwd(None, g, m, None, 4, A, 60, 15, A, A, A, big, 0, A) < 0            # blob
    assert bwd(None, g, m, A, 4, None, 60, 15, A, A, A, big, 0, A) < 0            # obs
    assert bwd(None, g, m, A, 4, A, 60, 15, A, A, None, big, 0, A) < 0            # workspace
    assert bwd(None, g, m, A, 4, A, 60, 15, A, A, A, big, 0, None) < 0            # grad_blob
    assert bwd(None, g, m, A, 4, A, 60, 15, None, None, A, big, 0, A) < 0 and b"both NULL" in L.f16env_last_error()
    assert bwd(None, g, m, A + 4, 4, A, 60, 15, A, A, A, big, 0, A) < 0 and b"aligned" in L.f16env_last_error()
    assert bwd(None, g, m, A, 4, A, 60, 15, A + 4, A, A, big, 0, A) < 0           # d_mean not 16-B aligned
    assert bwd(None, g, m, A, 4, A, 60, 15, A, A + 2, A, big, 0, A) < 0           # d_values not float-aligned
    assert bwd(None, g, m, A, 4, A, 60, 15, A, A, A + 8, big, 0, A) < 0           # workspace not 16-B aligned
    assert bwd(None, g, m, A, 4, A, 60, 15, A, A, A, big, 0, A + 4) < 0           # grad_blob not 16-B aligned
    assert bwd(None, g, m, A, 4, A + 2, 60, 15, A, A, A, big, 0, A) < 0           # obs not float-aligned
    assert bwd(None, g, m, A, 4, A, -1, 15, A, A, A, big, 0, A) < 0               # negative strides
    assert bwd(None, g, m, A, 4, A, 60, -1, A, A, A, big, 0, A) < 0
    need = _workspace(L, desc, lma, 4, 0)
    assert bwd(None, g, m, A, 4, A, 60, 15, A, A, A, need - 1, 0, A) < 0 and b"workspace" in L.f16env_last_error()


def test_header_and_table_name_the_new_symbols(L):
    import os
    import re
    from f16_jsb_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "f16env.h")).read()
    for name in ("f16env_policy_lma_backward_workspace", "f16env_policy_lma_backward"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert "#define F16ENV_ABI_VERSION 7" in header


# ---------------------------------------------------------------------------------------------
# the class on the CPU
def test_train_policy_is_opt_in_and_the_forward_only_class_still_refuses():
    import f16_jsb_amd
    from f16_jsb_amd.lma_policy import NO_BACKWARD, DeviceLMAPolicy, DeviceLMATrainPolicy
    from f16_jsb_amd.ppo import DevicePPO
    assert f16_jsb_amd.DeviceLMATrainPolicy is DeviceLMATrainPolicy and "DeviceLMATrainPolicy" in f16_jsb_amd.__all__
    assert issubclass(DeviceLMATrainPolicy, DeviceLMAPolicy)
    assert "lma_dropout=0.0" in DeviceLMATrainPolicy.__doc__.replace("lma_dropout = 0.0", "lma_dropout=0.0")
    layers = _layers(lma_ref.random_net("S"))
    pol = DeviceLMATrainPolicy.from_layers(*layers, stack_k=4, device="cpu")
    assert pol.requires_grad_() is pol and pol.blob.requires_grad
    params = pol.parameters()
    assert len(params) == 1 and params[0] is pol.blob
    assert pol.requires_grad_(False) is pol and not pol.blob.requires_grad
    with pytest.raises(NotImplementedError, match="LMA backward is not built"):
        DevicePPO(pol)
    plain = DeviceLMAPolicy.from_layers(*layers, stack_k=4, device="cpu")
    assert torch.equal(plain.blob, pol.blob)
    assert "LMA backward is not built" in NO_BACKWARD and "DeviceLMATrainPolicy" in NO_BACKWARD
    for call in (plain.requires_grad_, lambda: plain.backward_blob(None), lambda: plain.reserve_backward(8),
                 lambda: DevicePPO(plain)):
        with pytest.raises(NotImplementedError, match="LMA backward is not built"):
            call()
    plain.blob.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="LMA backward is not built"):
        plain.mean_and_value(torch.zeros(2, 4, 15))
    with pytest.raises(NotImplementedError, match="LMA backward is not built"):
        plain.evaluate_actions(torch.zeros(2, 4, 15), torch.zeros(2, 4))
