"""CPU checks of the device policy's host side (ABI 7): the exported symbols, the blob layout
against the Python packer, argument validation without a device, the SB3 state-dict route, and
the checker (tests/policy_ref.py) itself."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch

import policy_ref
from f16_jsb_amd import abi


@pytest.fixture(scope="module")
def L():
    from f16_jsb_amd.build import build
    build()
    from f16_jsb_amd import _lib
    return _lib.lib()


def _c_layout(L, desc):
    off = (ctypes.c_int64 * abi.F16_POLICY_N_OFFSETS)()
    n = ctypes.c_int64(0)
    assert L.f16env_policy_blob_layout(ctypes.byref(desc), off, ctypes.byref(n)) == 0
    return list(off), n.value


def _layers(rng, in_dim, widths):
    out, fan_in = [], in_dim
    for w in widths:
        out.append((torch.from_numpy(rng.standard_normal((w, fan_in)).astype(np.float32)),
                    torch.from_numpy(rng.standard_normal(w).astype(np.float32))))
        fan_in = w
    return out


def _net(rng, k, d, pi_w, vf_w):
    pi, vf = _layers(rng, k * d, pi_w), _layers(rng, k * d, vf_w)
    act = _layers(rng, pi_w[-1], [4])[0]
    val = _layers(rng, vf_w[-1], [1])[0]
    log_std = torch.from_numpy(rng.standard_normal(4).astype(np.float32))
    return pi, vf, act, val, log_std


def test_library_exports_policy_symbols(L):
    from f16_jsb_amd import _lib
    for name in ("f16env_policy_forward", "f16env_policy_blob_layout"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    assert L.f16env_abi_version() == abi.F16ENV_ABI_VERSION == 7


MATRIX_CASES = [pytest.param(*c[:4], id=name) for name, c in policy_ref.MATRIX.items()]


def _assert_matrix_instance(k, d, pi_w, vf_w):
    """A matrix case runs on the kernel instance its row of the matrix states."""
    for name, c in policy_ref.MATRIX.items():
        if c[:4] == (k, d, pi_w, vf_w):
            assert policy_ref.kernel_instance(k, d, pi_w, vf_w) == c[4], name


def test_matrix_reaches_the_instances_it_names():
    """The documented LDS rule (policy_ref.kernel_instance) puts every matrix case on the kernel
    instance its row states, all four instances occur, and so do the first-layer k-step counts
    with remainders 0..3 modulo the k loop's batch of four and hidden layers of 1..4 tiles."""
    for name, (k, d, pi_w, vf_w, inst) in policy_ref.MATRIX.items():
        assert policy_ref.kernel_instance(k, d, pi_w, vf_w) == inst, name
        desc = abi.policy_desc(k, d, pi_w, vf_w)
        assert abi.policy_blob_layout(desc)[1] == policy_ref.blob_floats(k, d, pi_w, vf_w), name
    cases = policy_ref.MATRIX.values()
    assert {c[4] for c in cases} == {(15, True), (15, False), (17, True), (17, False)}
    assert {((c[0] * c[1] + 1) // 2) % 4 for c in cases} == {0, 1, 2, 3}
    assert {w // 32 for c in cases for w in c[2] + c[3]} == {1, 2, 3, 4}
    assert {len(c[2]) for c in cases} | {len(c[3]) for c in cases} == {1, 2, 3}
    # the figures DESIGN section 4 and the matrix quote
    assert policy_ref.kernel_instance(4, 15, [64, 64], [64, 64]) == (15, True)
    k, d, pi_w, vf_w, _ = policy_ref.MATRIX["F"]
    assert policy_ref.blob_floats(k, d, pi_w, vf_w) == 2 * (21888 + 2 * 16512) + 2 * 4128 + 4  # 472 KB
    assert 4 * 4 * (170 * 33 + 128 * 32) == 155296 <= policy_ref.LDS_BYTES


@pytest.mark.parametrize("k,d,pi_w,vf_w", MATRIX_CASES)
def test_pack_unpack_round_trip(k, d, pi_w, vf_w):
    """pack_blob, then the documented layout read back (policy_ref.unpack_blob, which shares no
    code with the packer): every layer, head and log_std bit-equal, every pad position zero, and
    the pieces account for every float of the blob exactly once."""
    from f16_jsb_amd.policy import pack_blob
    _assert_matrix_instance(k, d, pi_w, vf_w)
    rng = np.random.default_rng(100 * k + d)
    pi, vf, act, val, log_std = _net(rng, k, d, pi_w, vf_w)
    blob = pack_blob(abi.policy_desc(k, d, pi_w, vf_w), pi, vf, act, val, log_std).numpy()
    assert blob.dtype == np.float32 and blob.shape == (policy_ref.blob_floats(k, d, pi_w, vf_w),)
    u = policy_ref.unpack_blob(k, d, pi_w, vf_w, blob)
    same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))  # noqa: E731
    for got, want in ((u["pi"], pi), (u["vf"], vf), ([u["act_head"]], [act]), ([u["val_head"]], [val])):
        assert len(got) == len(want)
        for (gw, gb), (w, b) in zip(got, want):
            assert same(gw, w.numpy()) and same(gb, b.numpy())
            assert np.all(gw != 0)  # (the random weights are nowhere zero: a zero read back is a miss)
    assert same(u["log_std"], log_std.numpy())
    assert np.all(u["claims"] == 1)
    assert np.all(blob[u["zero"]] == 0) and len(np.unique(u["zero"])) == len(u["zero"])
    n_weights = sum(w.numel() + b.numel() for w, b in pi + vf + [act, val]) + 4
    assert n_weights + len(u["zero"]) == blob.size


@pytest.mark.parametrize("k,d,pi_w,vf_w", [(4, 15, [64, 64], [64, 64]), (10, 17, [64, 64], [128, 64])] + MATRIX_CASES)
def test_blob_layout_matches_python_packer(L, k, d, pi_w, vf_w):
    from f16_jsb_amd.policy import pack_blob
    _assert_matrix_instance(k, d, pi_w, vf_w)
    desc = abi.policy_desc(k, d, pi_w, vf_w)
    off, total = _c_layout(L, desc)
    off_py, total_py = abi.policy_blob_layout(desc)
    assert off == off_py and total == total_py
    # the pieces tile the blob without overlap, each on the 16-B boundary the kernel's float4 reads assume
    sizes = {}
    for b, widths in enumerate((pi_w, vf_w)):
        fan_in = k * d
        for l, w in enumerate(widths):
            sizes[6 * b + 2 * l] = (w // 32) * ((fan_in + 1) // 2) * 64
            sizes[6 * b + 2 * l + 1] = w
            fan_in = w
        head = abi.F16_POLICY_OFF_VAL_W if b else abi.F16_POLICY_OFF_ACT_W
        sizes[head], sizes[head + 1] = ((fan_in + 1) // 2) * 64, 32
    sizes[abi.F16_POLICY_OFF_LOG_STD] = 4
    assert sorted(i for i, o in enumerate(off) if o >= 0) == sorted(sizes)
    spans = sorted((off[i], off[i] + sizes[i]) for i in sizes)
    assert spans[0][0] == 0 and spans[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert all(o % 4 == 0 for o in off if o >= 0) and total % 4 == 0
    # the packer fills exactly that blob, every element where the layout says
    rng = np.random.default_rng(3)
    pi, vf, act, val, log_std = _net(rng, k, d, pi_w, vf_w)
    blob = pack_blob(desc, pi, vf, act, val, log_std).numpy()
    assert blob.shape == (total,)
    for (w, bias), slot in ((pi[0], 0), (vf[-1], 6 + 2 * (len(vf_w) - 1)), (act, abi.F16_POLICY_OFF_ACT_W)):
        w, bias = w.numpy(), bias.numpy()
        nks = (w.shape[1] + 1) // 2
        for o, i in ((0, 0), (w.shape[0] - 1, w.shape[1] - 1), (w.shape[0] // 2, 7), (1, w.shape[1] - 2)):
            to, r, s, h = o // 32, o % 32, i // 2, i % 2
            assert blob[off[slot] + ((to * nks + s) * 2 + h) * 32 + r] == w[o, i]
        assert np.array_equal(blob[off[slot + 1]:off[slot + 1] + len(bias)], bias)
    if (k * d) % 2:  # the odd fan-in's pad input has zero weights
        assert np.all(blob[off[0] + ((k * d) // 2 * 2 + 1) * 32:][:32] == 0)
    assert np.array_equal(blob[off[abi.F16_POLICY_OFF_LOG_STD]:], log_std.numpy())
    # the head tile's rows past its outputs are zero
    head = blob[off[abi.F16_POLICY_OFF_VAL_W]:off[abi.F16_POLICY_OFF_VAL_B]].reshape(-1, 2, 32)
    assert np.all(head[:, :, 1:] == 0) and np.any(head[:, :, 0] != 0)


def test_odd_fan_in_is_padded_in_the_weights(L):
    from f16_jsb_amd.policy import pack_blob
    desc = abi.policy_desc(1, 15, [32], [32])
    off, total = _c_layout(L, desc)
    assert (off, total) == abi.policy_blob_layout(desc)
    assert off[1] - off[0] == 8 * 64  # ceil(15 / 2) k-steps of one tile
    blob = pack_blob(desc, *_net(np.random.default_rng(1), 1, 15, [32], [32])).numpy()
    assert np.all(blob[off[0] + (7 * 2 + 1) * 32:off[1]] == 0) and np.all(blob[off[0] + 7 * 64:][:32] != 0)


def test_bad_arguments_return_errors_without_a_device(L):
    """Every bad argument is refused with a negative status and a message before anything is
    launched (no device needed)."""
    good = abi.policy_desc(4, 15, [64, 64], [64, 64])
    off = (ctypes.c_int64 * abi.F16_POLICY_N_OFFSETS)()
    n = ctypes.c_int64(0)
    assert L.f16env_policy_blob_layout(None, off, ctypes.byref(n)) < 0
    assert L.f16env_policy_blob_layout(ctypes.byref(good), None, ctypes.byref(n)) < 0
    assert L.f16env_policy_blob_layout(ctypes.byref(good), off, None) < 0

    def bad_desc(**kw):
        d = abi.policy_desc(4, 15, [64, 64], [64, 64])
        for key, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, key)[v[0]] = v[1]
            else:
                setattr(d, key, v)
        return d

    for d in (bad_desc(K=0), bad_desc(K=11), bad_desc(D=16), bad_desc(n_pi=0), bad_desc(n_vf=4),
              bad_desc(pi_width=(0, 48)), bad_desc(vf_width=(1, 256)), bad_desc(activation=2)):
        assert L.f16env_policy_blob_layout(ctypes.byref(d), off, ctypes.byref(n)) < 0
        assert L.f16env_policy_forward(None, ctypes.byref(d), 256, 4, 256, 60, 15, 0, 0, 0, None, 256, 256, 256, 0) < 0
        assert L.f16env_last_error()

    fwd = L.f16env_policy_forward
    g = ctypes.byref(good)
    A = 4096  # a non-NULL, 16-B aligned stand-in address (never dereferenced: the call is refused first)
    assert fwd(None, None, A, 4, A, 60, 15, 0, 0, 0, None, A, A, A, 0) < 0          # no descriptor
    assert fwd(None, g, A, -1, A, 60, 15, 0, 0, 0, None, A, A, A, 0) < 0            # n < 0
    assert b"n must be" in L.f16env_last_error()
    assert fwd(None, g, None, 4, A, 60, 15, 0, 0, 0, None, A, A, A, 0) < 0          # blob
    assert fwd(None, g, A, 4, None, 60, 15, 0, 0, 0, None, A, A, A, 0) < 0          # obs
    assert fwd(None, g, A, 4, A, 60, 15, 0, 0, 0, None, None, A, A, 0) < 0          # actions
    assert fwd(None, g, A, 4, A, 60, 15, 0, 0, 0, None, A, None, A, 0) < 0          # values
    assert fwd(None, g, A, 4, A, 60, 15, 0, 0, 0, None, A, A, None, 0) < 0          # log_probs
    assert fwd(None, g, A, 4, A, 60, 15, 0, 0, 0, None, None, None, None, abi.F16_POLICY_VALUE_ONLY) < 0
    assert fwd(None, g, A + 4, 4, A, 60, 15, 0, 0, 0, None, A, A, A, 0) < 0         # blob not 16-B aligned
    assert b"aligned" in L.f16env_last_error()
    assert fwd(None, g, A, 4, A, 60, 15, 0, 0, 0, None, A + 4, A, A, 0) < 0         # actions not 16-B aligned
    assert fwd(None, g, A, 4, A, 60, 15, 0, 0, 0, A + 8, A, A, A, 0) < 0            # eps not 16-B aligned
    assert fwd(None, g, A, 4, A + 2, 60, 15, 0, 0, 0, None, A, A, A, 0) < 0         # obs not float-aligned
    assert fwd(None, g, A, 4, A, -1, 15, 0, 0, 0, None, A, A, A, 0) < 0             # negative stride
    assert fwd(None, g, A, 4, A, 60, 15, 0, 0, 0, None, A, A, A, 0x8) < 0           # unknown flag
    assert b"flags" in L.f16env_last_error()


def test_python_front_end_refuses_bad_shapes():
    with pytest.raises(ValueError):
        abi.policy_desc(4, 15, [48], [64])
    with pytest.raises(ValueError):
        abi.policy_desc(4, 15, [64] * 4, [64])
    with pytest.raises(ValueError):
        abi.policy_desc(11, 15, [64], [64])
    with pytest.raises(ValueError):
        abi.policy_desc(4, 15, [64], [64], activation="gelu")


def test_from_state_dict_packs_the_same_blob_as_from_layers():
    """SB3's ActorCriticPolicy key names (hand-built: stable_baselines3 is not imported)."""
    from f16_jsb_amd.policy import DevicePolicy
    rng = np.random.default_rng(5)
    pi, vf, act, val, log_std = _net(rng, 4, 15, [32, 96, 64], [128, 64])
    sd = {"log_std": log_std, "action_net.weight": act[0], "action_net.bias": act[1],
          "value_net.weight": val[0], "value_net.bias": val[1]}
    for name, layers in (("policy_net", pi), ("value_net", vf)):
        for i, (w, b) in enumerate(layers):
            sd["mlp_extractor.%s.%d.weight" % (name, 2 * i)] = w
            sd["mlp_extractor.%s.%d.bias" % (name, 2 * i)] = b
    a = DevicePolicy.from_state_dict(sd, stack_k=4, activation="relu", device="cpu")
    b = DevicePolicy.from_layers(pi, vf, act, val, log_std, stack_k=4, activation="relu", device="cpu")
    assert torch.equal(a.blob, b.blob) and a.blob.abs().sum() > 0
    assert list(a.desc.pi_width) == [32, 96, 64] and list(a.desc.vf_width)[:2] == [128, 64] and a.desc.n_vf == 2
    # a reload lands in the same blob (same storage)
    ptr = a.blob.data_ptr()
    a.load_state_dict({k: v * 2 for k, v in sd.items()})
    assert a.blob.data_ptr() == ptr and not torch.equal(a.blob, b.blob)
    # a host tensor is refused by the call, like any wrong buffer
    with pytest.raises(ValueError):
        a(torch.zeros(3, 4, 15))


# ---------------------------------------------------------------------------------------------
# the checker itself
def test_checker_normals_moments():
    """32 768 x 4 draws: |mean| < 0.012 and |var - 1| < 0.02 (4 sigma at that sample size)."""
    e = policy_ref.policy_normals(1234, np.arange(32768), 7)
    assert e.shape == (32768, 4) and np.all(np.isfinite(e)) and np.abs(e).max() <= 5.9
    assert abs(e.mean()) < 0.012 and abs(e.var() - 1.0) < 0.02
    # a stream per (seed, step, env): no two agree
    assert not np.array_equal(e, policy_ref.policy_normals(1234, np.arange(32768), 8))
    assert not np.array_equal(e, policy_ref.policy_normals(1235, np.arange(32768), 7))
    assert np.array_equal(e[100:200], policy_ref.policy_normals(1234, np.arange(100, 200), 7))


def test_checker_log_prob_matches_torch_normal():
    rng = np.random.default_rng(11)
    pi, vf, act, val, log_std = _net(rng, 4, 15, [64, 64], [64, 64])
    obs = rng.standard_normal((50, 4, 15))
    eps = rng.standard_normal((50, 4))
    a, v, lp, mean = policy_ref.forward(obs, [(w.numpy(), b.numpy()) for w, b in pi],
                                        [(w.numpy(), b.numpy()) for w, b in vf], (act[0].numpy(), act[1].numpy()),
                                        (val[0].numpy(), val[1].numpy()), log_std.numpy(), eps)
    dist = torch.distributions.Normal(torch.from_numpy(mean), torch.from_numpy(np.exp(log_std.numpy().astype(np.float64))))
    want = dist.log_prob(torch.from_numpy(a)).sum(-1).numpy()
    assert np.abs(lp - want).max() < 1e-12
    # and the forward is torch's in float64
    x = torch.from_numpy(obs).reshape(50, -1)
    h = x
    for w, b in pi:
        h = torch.tanh(torch.nn.functional.linear(h, w.double(), b.double()))
    assert np.abs(torch.nn.functional.linear(h, act[0].double(), act[1].double()).numpy() - mean).max() < 1e-12
    assert math.isclose(policy_ref.LOG_SQRT_2PI, 0.9189385332046727, rel_tol=1e-15)
