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


# ---------------------------------------------------------------------------------------------
# what the GPU matrix reaches, the exact nets' guard, and the stress inputs' conditioning
def test_matrix_covers_the_lattice_the_launcher_accepts():
    """Every L_new, ff width, stacking, block count and MLP depth the host launcher accepts is in
    MATRIX, and both activations meet blocks: a later deletion of a case fails here by name."""
    by = lambda f: {f(*MATRIX[name]) for name in MATRIX}  # noqa: E731
    assert by(lambda k, *_: lma_ref.new_dims(k)[0]) == {1, 2, 3, 4, 5}
    assert by(lambda k, *_: k) == set(range(1, 11))
    assert {MATRIX[name][3] for name in MATRIX if MATRIX[name][2] > 0} == {32, 64, 96, 128}
    assert by(lambda k, d, nl, ff, pi, vf, act, hs, inst: hs) == set(lma_ref.STACKINGS) == {1, 2, 4, 8, 16, 32}
    assert by(lambda k, d, nl, *_: nl) == {0, 1, 2, 3}
    assert by(lambda k, d, nl, ff, pi, *_: len(pi)) == {1, 2, 3} == by(lambda k, d, nl, ff, pi, vf, *_: len(vf))
    assert {MATRIX[name][6] for name in MATRIX if MATRIX[name][2] > 0} == {"tanh", "relu"}
    assert by(lambda k, d, *_: d) == {15, 17}
    # the cases this coverage rests on, by name
    want = {"K2": (1, 96, 1), "K5": (2, 96, 8), "K6": (3, 96, 16), "K6r": (3, 64, 32), "K8": (4, 128, 1), "Y": (5, 128, 8)}
    assert set(lma_ref.NEW_CASES) == set(want) <= set(MATRIX)
    for name, (L, ff, hs) in want.items():
        k, d, nl, ff_, pi_w, vf_w, act, hs_, inst = MATRIX[name]
        assert (lma_ref.new_dims(k)[0], ff_, hs_) == (L, ff, hs), name
        assert lma_ref.kernel_instance(k, d, nl, ff_, pi_w, vf_w) == inst, name
    assert [name for name in MATRIX if lma_ref.new_dims(MATRIX[name][0])[0] == 3] == ["K6", "K6r"]  # K = 6 alone gives L 3
    k, d, nl, ff, pi_w, vf_w, act, hs, inst = MATRIX["Y"]   # the largest: every maximum at once
    assert (k, nl, ff, max(pi_w + vf_w), len(pi_w), len(vf_w)) == (10, 3, 128, 128, 3, 3) and inst[1] == 159872


@pytest.mark.parametrize("k", range(1, 11))
def test_exact_integer_nets_stay_exact_in_float32(k):
    """The guard of the GPU's exact-layout test for this K and every stacking, on the inputs that
    test uses (n = 33): no sum of magnitudes reaches 2^24, the outputs are not all zero, and
    another stacking is another network (so a wrong rmap / cmap cannot pass)."""
    net, pe = lma_ref.int_case(k)
    x = lma_ref.int_inputs(k, lma_ref.INT_ROWS)
    seen = []
    for hs in lma_ref.STACKINGS:
        f, mean, value, bound = lma_ref.int_forward(net, pe, x, hs)
        assert bound < 2 ** 24, (k, hs, bound)
        assert np.abs(f).max() > 0 and np.abs(mean).max() > 0 and np.abs(value).max() > 0, (k, hs)
        seen.append(f)
    if k > 1:   # (one frame: every stacking is the identity)
        assert all(not np.array_equal(seen[i], seen[j]) for i in range(6) for j in range(i)), k
    else:
        assert all(np.array_equal(seen[0], s) for s in seen)


KINDS = ("features", "actions", "values", "log_probs")


@pytest.mark.parametrize("kind", lma_ref.STRESS)
def test_stress_input_is_hard_and_well_conditioned(kind):
    """Each stress input (net K6, 65 rows) leaves the easy regime in the way it claims, torch's
    float32 restatement stays finite on it, and a float32 restatement that only sums every linear
    in the other order stays within 2 x max(torch's error, floor) of fp64 -- half the GPU rule's
    budget of 4. That is a condition on the input, not on the kernel: if a seed change breaks it,
    choose another input; the 4 does not move."""
    net, x, eps, rows = lma_ref.stress_case(kind)
    act, hs = MATRIX[lma_ref.STRESS_CASE][6:8]
    ref, t32, probe = lma_ref.stress_refs(kind)
    assert x.shape == (65, 6, 15) and all(np.all(np.isfinite(a)) for a in t32)
    ln_mean, ln_spread = np.stack(probe["ln_mean"]), np.stack(probe["ln_spread"])   # (4 LayerNorms, 65 x 3 tokens)
    print("%s: max |score| %.1f, LayerNorm input mean %.2f..%.2f spread %.2f..%.2f, max GELU argument %.1f, tanh %.1f" % (
        kind, probe["max_score"], ln_mean.min(), ln_mean.max(), ln_spread.min(), ln_spread.max(),
        probe["gelu_arg"].max(), probe["act_arg"].max()))
    if kind == "sharp":        # past float32 exp's overflow at 88.7: the max subtraction is what keeps it finite
        assert probe["max_score"] > 100.0
    elif kind == "offset":     # E[x^2] ~ 1e4 against a variance of ~ 1..16: a one-pass variance loses 3 digits
        assert np.all(np.abs(ln_mean - lma_ref.LN_OFFSET) < 2.0) and 0.5 < ln_spread.min() and ln_spread.max() < 8.0
    elif kind == "degenerate":
        feats = lma_ref.frame_features(torch.from_numpy(x[rows].astype(np.float64))).numpy()
        assert np.all(feats[0] == feats[0][0]) and np.all(feats[1] == feats[1][0])   # K equal frames in both rows
        assert np.all(feats[0][:, 0] == 1.0) and np.all(feats[0][:, 15] == 1.0) and np.all(feats[0][:, 16] == 0.0)  # dist 0, rel 0
        # the positional table still tells the frames apart: the tokens of z differ and no LayerNorm row is constant
        z = lma_ref.extract(dict(net, blocks=[]), x[rows], torch.float64, hs).numpy().reshape(2, 3, 32)
        assert np.abs(z[:, 1:] - z[:, :1]).max(-1).min() > 0.1
        per_row = ln_spread.reshape(4, 65, 3)[:, rows]
        assert per_row.min() > 0.1
    else:                      # the MLPs' tanh is deep in its tail on that row; LayerNorm keeps GELU's argument moderate
        assert probe["act_arg"][lma_ref.HUGE_ROW] > 88.0 and np.abs(x[lma_ref.HUGE_ROW]).min() == lma_ref.HUGE
        assert np.abs(ref[0][lma_ref.HUGE_ROW]).max() > 1e3
    flipped = lma_ref.forward(net, x, eps, torch.float32, act, hs, flip=True)
    assert not np.array_equal(flipped[0], t32[0])   # (the other order is another rounding)
    for name, (e_f, floor), (e_t, _) in zip(KINDS, lma_ref.errors(flipped[:4], ref[:4], rows), lma_ref.errors(t32[:4], ref[:4], rows)):
        print("%s %s: reordered %.3e torch %.3e floor %.3e ratio %.2f" % (kind, name, e_f, e_t, floor, e_f / max(e_t, floor)))
        assert e_f <= 2.0 * max(e_t, floor), (kind, name)


def test_planted_defects_fail_the_gpu_rule():
    """The two float32 defects the stress inputs are there for: softmax without its max
    subtraction is non-finite on the sharp net, and a one-pass variance exceeds the GPU rule's
    4 x max(torch, floor) on the offset net's features. Both pass on the matrix's easy inputs."""
    act, hs = MATRIX[lma_ref.STRESS_CASE][6:8]
    net, x, eps, _ = lma_ref.stress_case("sharp")
    naive = lma_ref.forward(net, x, eps, torch.float32, act, hs, wrong="naive_softmax")
    bad = [int(np.sum(~np.isfinite(a))) for a in naive[:3]]
    print("naive softmax on the sharp net: non-finite features %d, actions %d, values %d" % tuple(bad))
    assert all(b > 0 for b in bad)
    net, x, eps, _ = lma_ref.stress_case("offset")
    ref, t32, _ = lma_ref.stress_refs("offset")
    one_pass = lma_ref.forward(net, x, eps, torch.float32, act, hs, wrong="one_pass_var")
    ratios = {}
    for name, (e_w, floor), (e_t, _) in zip(KINDS, lma_ref.errors(one_pass[:4], ref[:4]), lma_ref.errors(t32[:4], ref[:4])):
        ratios[name] = e_w / max(e_t, floor)
        print("one-pass variance on the offset net, %s: %.3e against torch %.3e floor %.3e: %.1f x" % (name, e_w, e_t, floor, ratios[name]))
    assert ratios["features"] > 4.0   # (measured 56 x; actions 10 x and values 19 x are printed above)
    # and on the matrix's own inputs neither defect shows: the easy regime cannot see them
    net, (xs, es) = lma_ref.random_net(lma_ref.STRESS_CASE), lma_ref.shared_inputs(lma_ref.STRESS_CASE)
    ref = lma_ref.forward(net, xs[:65], es[:65], torch.float64, act, hs)
    t32 = lma_ref.forward(net, xs[:65], es[:65], torch.float32, act, hs)
    for wrong in ("naive_softmax", "one_pass_var"):
        got = lma_ref.forward(net, xs[:65], es[:65], torch.float32, act, hs, wrong=wrong)
        for name, (e_w, floor), (e_t, _) in zip(KINDS, lma_ref.errors(got[:4], ref[:4]), lma_ref.errors(t32[:4], ref[:4])):
            print("%s on standard-normal rows, %s: %.2f x" % (wrong, name, e_w / max(e_t, floor)))
            assert e_w <= 4.0 * max(e_t, floor), (wrong, name)


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
