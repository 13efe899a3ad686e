"""CPU checks of the device LMA policy's host side: the re-chunk rule and the stacking permutation,
the restatement (tests/lma_ref.py) against independent torch pieces and its negative controls, the
packer against the documented blob layout, the state-dict key names, the ABI additions and the
refusals of everything that would need the extractor's backward. No GPU."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lma_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = lma_ref.MATRIX
L_NEW = [1, 1, 1, 2, 2, 3, 2, 4, 4, 5]
C_NEW = [64, 128, 192, 128, 160, 128, 224, 128, 144, 128]


def _tt(a):
    return torch.as_tensor(np.asarray(a))


def _layers(net):
    """lma_ref's numpy net as the product's arguments: (ext, pi, vf, act_head, val_head, log_std)."""
    pair = lambda wb: (_tt(wb[0]), None if wb[1] is None else _tt(wb[1]))  # noqa: E731
    ext = {"embed": pair(net["embed"]), "embed2": pair(net["embed2"]),
           "blocks": [{k: pair(v) for k, v in blk.items()} for blk in net["blocks"]]}
    return ext, [pair(l) for l in net["pi"]], [pair(l) for l in net["vf"]], pair(net["act"]), pair(net["val"]), _tt(net["log_std"])


def _state_dict(net, aliases=True, bias=True):
    sd = {}
    flat = {"initial_transform.input_embedding": net["embed"], "initial_transform.embed_layer_2": net["embed2"]}
    for i, blk in enumerate(net["blocks"]):
        for piece in lma_ref.BLOCK_PIECES:
            flat["lma_blocks.%d.%s" % (i, piece)] = blk[piece]
    for prefix in ("features_extractor.", "pi_features_extractor.", "vf_features_extractor.")[:3 if aliases else 1]:
        for name, (w, b) in flat.items():
            sd[prefix + "lma_extractor." + name + ".weight"] = _tt(w).clone()
            if bias:
                sd[prefix + "lma_extractor." + name + ".bias"] = _tt(b).clone()
    for name, layers in (("policy_net", net["pi"]), ("value_net", net["vf"])):
        for i, (w, b) in enumerate(layers):
            sd["mlp_extractor.%s.%d.weight" % (name, 2 * i)] = _tt(w).clone()
            sd["mlp_extractor.%s.%d.bias" % (name, 2 * i)] = _tt(b).clone()
    sd["action_net.weight"], sd["action_net.bias"] = _tt(net["act"][0]).clone(), _tt(net["act"][1]).clone()
    sd["value_net.weight"], sd["value_net.bias"] = _tt(net["val"][0]).clone(), _tt(net["val"][1]).clone()
    sd["log_std"] = _tt(net["log_std"]).clone()
    return sd


# ---------------------------------------------------------------------------------------------
def test_new_dims_and_permutation():
    from f16_jsb_amd.abi import lma_desc, lma_new_dims
    assert [lma_ref.new_dims(k)[0] for k in range(1, 11)] == L_NEW
    assert [lma_ref.new_dims(k)[1] for k in range(1, 11)] == C_NEW
    for k in range(1, 11):
        assert lma_new_dims(k, 64) == lma_ref.new_dims(k)
        m = lma_desc(k, 15)
        assert (m.L_new, m.C_new) == lma_ref.new_dims(k)
    assert lma_ref.new_dims(7, plus_first=True) == (4, 112)  # the wrong search order is a different network
    rng = np.random.default_rng(1)
    for k in range(1, 11):
        for hs in (1, 2, 4, 8, 16, 32):
            y = torch.from_numpy(rng.standard_normal((3, k, 64)))
            L, C = lma_ref.new_dims(k)
            want = torch.cat(torch.split(y, 64 // hs, dim=2), dim=1).reshape(3, -1).view(3, L, C)
            flat = torch.zeros(3, k * 64, dtype=torch.float64)
            flat[:, torch.from_numpy(lma_ref.flat_index(k, 64, hs).reshape(-1))] = y.reshape(3, -1)
            assert torch.equal(flat.view(3, L, C), want)
            # the kernel's view of it: channels 2 s, 2 s + 1 are neighbours in flat and share a token
            f = lma_ref.flat_index(k, 64, hs)
            assert np.all(f[:, 0::2] % 2 == 0) and np.all(f[:, 1::2] == f[:, 0::2] + 1) and C % 2 == 0


def _independent_features(net, x, pe):
    """The extractor from torch's own pieces in fp64: nn.Linear, F.layer_norm, nn.GELU,
    F.scaled_dot_product_attention, split / cat / reshape / view."""
    def linear(wb):
        m = torch.nn.Linear(wb[0].shape[1], wb[0].shape[0]).double()
        with torch.no_grad():
            m.weight.copy_(_tt(wb[0]))
            m.bias.copy_(_tt(wb[1]))
        return m
    with torch.no_grad():
        n, k, _ = x.shape
        y = torch.relu(linear(net["embed"])(x)) + pe.double()
        L, C = lma_ref.new_dims(k)
        z = torch.cat(torch.split(y, 16, dim=2), dim=1).reshape(n, -1).view(n, L, C)
        z = torch.relu(linear(net["embed2"])(z))
        for blk in net["blocks"]:
            h = F.layer_norm(z, (32,), _tt(blk["ln_1"][0]).double(), _tt(blk["ln_1"][1]).double(), 1e-5)
            q, kk, v = linear(blk["attn.c_attn"])(h).split(32, dim=2)
            q, kk, v = (a.view(n, L, 4, 8).transpose(1, 2) for a in (q, kk, v))
            o = F.scaled_dot_product_attention(q, kk, v, attn_mask=None, dropout_p=0.0, is_causal=False)
            z = z + linear(blk["attn.c_proj"])(o.transpose(1, 2).contiguous().view(n, L, 32))
            h = F.layer_norm(z, (32,), _tt(blk["ln_2"][0]).double(), _tt(blk["ln_2"][1]).double(), 1e-5)
            z = z + linear(blk["mlp.c_proj"])(torch.nn.GELU()(linear(blk["mlp.c_fc"])(h)))
        return z.reshape(n, -1)


@pytest.mark.parametrize("name", ["R17", "T", "V"])
def test_restatement_agrees_with_torch_pieces(name):
    k = MATRIX[name][0]
    net = lma_ref.random_net(name)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((33, k, 17)))
    want = _independent_features(net, x, lma_ref.positional_table(k)).numpy()
    got = lma_ref.extract(net, x.numpy(), torch.float64).numpy()
    assert got.shape == want.shape == (33, lma_ref.new_dims(k)[0] * 32)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_negative_controls_exceed_the_gpu_bound():
    """Each wrong reading of the network moves case R's features by more than the GPU test's bound
    (4 x torch float32's error against fp64), so that bound has teeth."""
    net = lma_ref.random_net("R")
    x = np.random.default_rng(6).standard_normal((64, 10, 15)).astype(np.float32)
    ref = lma_ref.extract(net, x, torch.float64).numpy()
    e32 = np.abs(lma_ref.extract(net, x, torch.float32).numpy().astype(np.float64) - ref).max()
    bound = 4.0 * max(e32, 2.0 ** -24 * np.abs(ref).max())
    print("torch float32 error %.3e, bound %.3e" % (e32, bound))
    assert 0 < bound < 1e-3
    for wrong in ("qk_swap", "head_order", "tanh_gelu", "unbiased_var", "no_pe"):
        moved = np.abs(lma_ref.extract(net, x, torch.float64, wrong=wrong).numpy() - ref).max()
        print("%s moves the features by %.3e" % (wrong, moved))
        assert moved > bound, wrong
    assert lma_ref.new_dims(7, plus_first=True) != lma_ref.new_dims(7)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MATRIX))
def test_pack_then_documented_unpack(name):
    from f16_jsb_amd.abi import lma_blob_layout, lma_desc, policy_desc
    from f16_jsb_amd.lma_policy import pack_lma_blob, positional_encoding, unpack_lma_blob
    k, d, nl, ff, pi_w, vf_w, act, hs, inst = MATRIX[name]
    assert lma_ref.kernel_instance(k, d, nl, ff, pi_w, vf_w) == inst
    net = lma_ref.random_net(name)
    desc, lma = policy_desc(k, d, pi_w, vf_w, act), lma_desc(k, d, heads_stacking=hs, ff_hidden=ff, n_layers=nl)
    pe = positional_encoding(k, 64)
    assert torch.equal(pe, lma_ref.positional_table(k))
    blob = pack_lma_blob(desc, lma, *((_layers(net)[0], pe) + _layers(net)[1:])).numpy()
    assert blob.shape[0] == lma_blob_layout(desc, lma)[1] == lma_ref.blob_floats(k, nl, ff, pi_w, vf_w)
    got = lma_ref.unpack_blob(k, nl, ff, pi_w, vf_w, blob)
    assert np.all(got["claims"] == 1) and np.all(blob[got["zero"]] == 0)
    eq = lambda a, b: np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))  # noqa: E731
    for key in ("embed", "embed2", "act", "val"):
        assert eq(got[key][0], net[key][0]) and eq(got[key][1], net[key][1]), key
    for br, layers in (("pi", net["pi"]), ("vf", net["vf"])):
        for l, (w, b) in enumerate(layers):
            assert eq(got["%s%d" % (br, l)][0], w) and eq(got["%s%d" % (br, l)][1], b)
    assert eq(got["log_std"], net["log_std"]) and eq(got["pe"], pe.numpy().reshape(-1))
    for i, blk in enumerate(net["blocks"]):
        for piece in lma_ref.BLOCK_PIECES:
            if piece.startswith("ln"):
                assert eq(got["blocks.%d.%s.w" % (i, piece)], blk[piece][0]) and eq(got["blocks.%d.%s.b" % (i, piece)], blk[piece][1])
            else:
                assert eq(got["blocks.%d.%s" % (i, piece)][0], blk[piece][0]) and eq(got["blocks.%d.%s" % (i, piece)][1], blk[piece][1])
    # and the product's own inverse
    ext, pe2, pi, vf, ah, vh, ls = unpack_lma_blob(desc, lma, torch.from_numpy(blob))
    assert torch.equal(pe2, pe) and eq(ext["embed2"][0].numpy(), net["embed2"][0]) and eq(vf[0][0].numpy(), net["vf"][0][0])


def test_state_dict_names_prefixes_and_bias():
    from f16_jsb_amd.lma_policy import DeviceLMAPolicy, extractor_from_state_dict
    k = 10
    net = lma_ref.random_net("R")
    sd = _state_dict(net)
    assert "features_extractor.lma_extractor.lma_blocks.1.mlp.c_proj.weight" in sd
    assert "vf_features_extractor.lma_extractor.initial_transform.embed_layer_2.bias" in sd
    pol = DeviceLMAPolicy.from_state_dict(sd, stack_k=k, device="cpu")
    assert (pol.lma.n_layers, pol.lma.ff_hidden, pol.lma.embed_dim, pol.lma.L_new, pol.features_dim) == (2, 128, 64, 5, 160)
    back = pol.state_dict()
    assert set(back) == set(sd)
    for key, v in sd.items():
        assert torch.equal(back[key], v), key
    pol2 = DeviceLMAPolicy.from_state_dict({k_: v for k_, v in sd.items() if not k_.startswith(("pi_f", "vf_f"))},
                                           stack_k=k, device="cpu")
    assert torch.equal(pol2.blob, pol.blob)
    pol2.blob.zero_()
    pol2.load_state_dict(sd)
    assert torch.equal(pol2.blob, pol.blob)
    # a differing alias: a non-shared extractor is refused
    bad = dict(sd)
    bad["pi_features_extractor.lma_extractor.lma_blocks.0.ln_1.weight"] = bad[
        "pi_features_extractor.lma_extractor.lma_blocks.0.ln_1.weight"] + 1.0
    with pytest.raises(ValueError, match="non-shared extractor"):
        DeviceLMAPolicy.from_state_dict(bad, stack_k=k, device="cpu")
    # lma_bias=False: no bias keys under the extractor; they pack as zeros
    nob = _state_dict(net, bias=False)
    assert not any(k_.endswith(".bias") and "lma_extractor" in k_ for k_ in nob)
    pol3 = DeviceLMAPolicy.from_state_dict(nob, stack_k=k, device="cpu")
    got = lma_ref.unpack_blob(k, 2, 128, [64, 64], [128, 64], pol3.blob.numpy())
    for name in ("embed", "embed2", "blocks.0.attn.c_attn", "blocks.1.mlp.c_proj"):
        assert np.all(got[name][1] == 0) and np.array_equal(got[name][0], lma_ref.unpack_blob(
            k, 2, 128, [64, 64], [128, 64], pol.blob.numpy())[name][0])
    assert np.all(got["blocks.0.ln_1.b"] == 0) and np.array_equal(got["blocks.0.ln_1.w"], net["blocks"][0]["ln_1"][0])
    with pytest.raises(KeyError, match="input_embedding"):
        extractor_from_state_dict({k_: v for k_, v in sd.items() if "features_extractor" not in k_})


# ---------------------------------------------------------------------------------------------
def test_abi_additions_agree(tmp_path):
    """f16_lma_desc as the C compiler lays the header out against abi.LmaDesc, the two prototypes
    against the signature table, every F16_LMA_* constant, and the version, still 7."""
    from f16_jsb_amd import _lib, abi
    from test_abi_cpu import parse_header
    src = tmp_path / "lma_layout.c"
    lines = ['#include <stdio.h>', '#include "f16env.h"', "int main(void) {",
             'printf("sizeof %zu 0\\n", sizeof(f16_lma_desc));']
    lines += ['printf("%s %%zu %%zu\\n", offsetof(f16_lma_desc, %s), sizeof(((f16_lma_desc*)0)->%s));' % (f, f, f)
              for f, _ in abi.LmaDesc._fields_]
    src.write_text("\n".join(lines + ["return 0; }"]) + "\n")
    exe = tmp_path / "lma_layout"
    subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    rows = [ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert rows[0] == ["sizeof", str(ctypes.sizeof(abi.LmaDesc)), "0"] and ctypes.sizeof(abi.LmaDesc) == 64
    assert len(rows) - 1 == len(abi.LmaDesc._fields_) == 11
    for (name, off, size), (f, _) in zip(rows[1:], abi.LmaDesc._fields_):
        d = getattr(abi.LmaDesc, f)
        assert (name, int(off), int(size)) == (f, d.offset, d.size)
    header = parse_header()
    assert header["constants"]["F16ENV_ABI_VERSION"] == abi.F16ENV_ABI_VERSION == 7
    lma_consts = {n: v for n, v in header["constants"].items() if n.startswith("F16_LMA_")}
    assert len(lma_consts) == 20 and all(getattr(abi, n) == v for n, v in lma_consts.items())
    assert abi.F16_LMA_OFF_BLOCK0 + abi.F16_LMA_BLOCK_SLOTS * abi.LMA_MAX_LAYERS == abi.F16_LMA_N_OFFSETS
    for fn, n_params in (("f16env_policy_lma_blob_layout", 4), ("f16env_policy_lma_forward", 17)):
        assert len(header["functions"][fn][1]) == n_params == len(_lib.SIGNATURES[fn][1])
    assert header["functions"]["f16env_policy_lma_forward"][1][:4] == ["void*", "f16_policy_desc*", "int32_t*", "float*"]


@pytest.fixture(scope="module")
def so_lib():
    from f16_jsb_amd.build import build
    build()
    from f16_jsb_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", list(MATRIX))
def test_layout_twin_equals_the_library(so_lib, name):
    from f16_jsb_amd.abi import F16_LMA_N_OFFSETS, lma_blob_layout, lma_desc, policy_desc
    k, d, nl, ff, pi_w, vf_w, act, hs, _ = MATRIX[name]
    desc, lma = policy_desc(k, d, pi_w, vf_w, act), lma_desc(k, d, heads_stacking=hs, ff_hidden=ff, n_layers=nl)
    off = (ctypes.c_int64 * F16_LMA_N_OFFSETS)()
    total = ctypes.c_int64(0)
    assert so_lib.f16env_policy_lma_blob_layout(ctypes.byref(desc), ctypes.byref(lma), off, ctypes.byref(total)) == 0
    assert (list(off), total.value) == lma_blob_layout(desc, lma)
    assert all(o % 4 == 0 for o in off if o >= 0)


def test_bad_descriptors_are_refused_by_name(so_lib):
    from f16_jsb_amd.abi import F16_LMA_N_OFFSETS, lma_desc, policy_desc
    desc = policy_desc(10, 15, [64, 64], [128, 64])
    off, total = (ctypes.c_int64 * F16_LMA_N_OFFSETS)(), ctypes.c_int64(0)

    def c_status(m):
        return so_lib.f16env_policy_lma_blob_layout(ctypes.byref(desc), ctypes.byref(m), off, ctypes.byref(total))
    assert c_status(lma_desc(10, 15)) == 0
    for field, value in (("K", 9), ("D", 17), ("embed_dim", 32), ("heads_stacking", 3), ("heads_stacking", 64), ("L_new", 4),
                         ("C_new", 64), ("d_new", 64), ("heads_latent", 8), ("ff_hidden", 48), ("n_layers", 4),
                         ("n_layers", -1)):
        m = lma_desc(10, 15)
        setattr(m, field, value)
        assert c_status(m) < 0 and so_lib.f16env_last_error(), field
    m = lma_desc(10, 15)
    m.reserved[2] = 1
    assert c_status(m) < 0
    assert so_lib.f16env_policy_lma_forward(None, ctypes.byref(desc), ctypes.byref(lma_desc(10, 15)), None, -1, None, 0, 0, 0,
                                            0, 0, None, None, None, None, None, 0) < 0
    for kw, word in ((dict(embed_dim=32), "embed_dim"), (dict(heads_stacking=3), "heads_stacking"), (dict(d_new=16), "d_new"),
                     (dict(heads_latent=2), "heads_latent"), (dict(ff_hidden=48), "ff_hidden"), (dict(n_layers=4), "n_layers")):
        with pytest.raises(ValueError, match=word):
            lma_desc(10, 15, **kw)
    with pytest.raises(ValueError, match="stack_k"):
        lma_desc(11, 15)
    with pytest.raises(ValueError, match="frame_dim"):
        lma_desc(10, 16)


def test_everything_that_needs_the_backward_refuses():
    import f16_jsb_amd
    from f16_jsb_amd.lma_policy import DeviceLMAPolicy
    from f16_jsb_amd.policy import DevicePolicy
    from f16_jsb_amd.ppo import DevicePPO
    assert f16_jsb_amd.DeviceLMAPolicy is DeviceLMAPolicy and issubclass(DeviceLMAPolicy, DevicePolicy)
    pol = DeviceLMAPolicy.from_layers(*_layers(lma_ref.random_net("S")), stack_k=4, device="cpu")
    msg = "LMA backward is not built"
    with pytest.raises(NotImplementedError, match=msg):
        pol.requires_grad_()
    assert pol.requires_grad_(False) is pol
    with pytest.raises(NotImplementedError, match=msg):
        pol.backward_blob(None)
    with pytest.raises(NotImplementedError, match=msg):
        pol.reserve_backward(8)
    with pytest.raises(NotImplementedError, match=msg):
        DevicePPO(pol)
    pol.blob.requires_grad_(True)  # (someone reaching past requires_grad_)
    obs = torch.zeros(2, 4, 15)
    with pytest.raises(NotImplementedError, match=msg):
        pol.mean_and_value(obs)
    with pytest.raises(NotImplementedError, match=msg):
        pol.evaluate_actions(obs, torch.zeros(2, 4))
