"""Checker of the device LMA policy (f16env_policy_lma_forward): a plain-torch restatement of the
eval-mode forward (the per-frame feature transform, embedding + positional table, the stacking
permutation, the second embedding, the attention / MLP blocks, the two MLPs, heads, sample and
log-prob) in a chosen dtype, written from the formulas of include/f16env.h; the re-chunk rule
(new_dims), the permutation as an index map, the documented blob layout read back (unpack_blob),
the documented LDS rule (kernel_instance) and the case matrix the CPU and GPU tests share.
Nothing here imports f16_jsb_amd."""
from __future__ import annotations

import math

import numpy as np
import torch

EMBED, D_NEW, HEADS, FEATURES = 64, 32, 4, 17
WAVES_PER_BLOCK, ROWS_PER_BLOCK = 4, 32   # four waves share one tile of 32 rows
LDS_BYTES = 160 * 1024
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
BLOCK_PIECES = ("ln_1", "attn.c_attn", "attn.c_proj", "ln_2", "mlp.c_fc", "mlp.c_proj")


# ---------------------------------------------------------------------------------------------
# shapes
def new_dims(k, embed=EMBED, plus_first=False):
    """(L_new, C_new): the divisor of k * embed closest to max(k // 2, 1); at equal distance the
    one below the target wins (plus_first: the wrong order, a negative control)."""
    total, target = k * embed, max(k // 2, 1)
    for delta in range(total):
        order = (target + delta, target - delta) if plus_first else (target - delta, target + delta)
        for cand in order:
            if cand >= 1 and total % cand == 0:
                return cand, total // cand
    raise AssertionError


def flat_index(k, embed=EMBED, heads_stacking=4):
    """(k, embed) int64: where y[t][c] lands in `flat`: ((c // dk) k + t) dk + c % dk."""
    dk = embed // heads_stacking
    t, c = np.arange(k)[:, None], np.arange(embed)[None, :]
    return ((c // dk) * k + t) * dk + c % dk


def positional_table(k, embed=EMBED):
    """The sinusoidal table in float32: pe[t][2 i] = sin(t w_i), pe[t][2 i + 1] = cos(t w_i),
    w_i = exp(2 i (-ln 10000 / embed))."""
    pos = torch.arange(k, dtype=torch.float32)[:, None]
    w = torch.exp(torch.arange(0, embed, 2, dtype=torch.float32) * (-math.log(10000.0) / embed))
    pe = torch.zeros(k, embed)
    pe[:, 0::2] = torch.sin(pos * w)
    pe[:, 1::2] = torch.cos(pos * w)
    return pe


# ---------------------------------------------------------------------------------------------
# the forward
def frame_features(o):
    """(..., 15) observation frames -> (..., 17) features, in o's dtype."""
    dx, dy, dz = o[..., 12] - o[..., 0], o[..., 13] - o[..., 1], o[..., 14] - o[..., 2]
    dist = torch.sqrt(dx * dx + dy * dy)
    rel = torch.atan2(dy, dx) - o[..., 11]
    return torch.stack([1.0 / (1.0 + dist * 1e-3), dz / 15000.0, o[..., 2] / 15000.0, o[..., 3], o[..., 6], o[..., 7],
                        o[..., 8], torch.cos(o[..., 4]), torch.cos(o[..., 5]), torch.sin(o[..., 4]), torch.sin(o[..., 5]),
                        torch.cos(o[..., 9]), torch.cos(o[..., 10]), torch.sin(o[..., 9]), torch.sin(o[..., 10]),
                        torch.cos(rel), torch.sin(rel)], -1)


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _lin(x, wb, dtype):
    y = x @ _t(wb[0], dtype).T
    return y if wb[1] is None else y + _t(wb[1], dtype)


def _layernorm(z, wb, dtype, unbiased=False):
    mean = z.mean(-1, keepdim=True)
    d = z - mean
    var = (d * d).sum(-1, keepdim=True) / (z.shape[-1] - (1 if unbiased else 0))
    y = d / torch.sqrt(var + 1e-5) * _t(wb[0], dtype)
    return y if wb[1] is None else y + _t(wb[1], dtype)


def _gelu(x, tanh_form=False):
    if tanh_form:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _attention(z, blk, dtype, wrong=None):
    n, L, _ = z.shape
    qkv = _lin(z, blk["attn.c_attn"], dtype)
    q, k, v = qkv[..., :D_NEW], qkv[..., D_NEW:2 * D_NEW], qkv[..., 2 * D_NEW:]
    if wrong == "qk_swap":
        q, k = k, q

    def heads(a):  # (n, L, 32) -> (n, 4, L, 8): head hd holds dims 8 hd .. 8 hd + 7
        if wrong == "head_order":
            return a.reshape(n, L, D_NEW // HEADS, HEADS).permute(0, 3, 1, 2)
        return a.reshape(n, L, HEADS, D_NEW // HEADS).permute(0, 2, 1, 3)
    q, k, v = heads(q), heads(k), heads(v)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(D_NEW // HEADS)
    s = s - s.max(-1, keepdim=True).values
    p = torch.exp(s)
    p = p / p.sum(-1, keepdim=True)
    o = p @ v
    if wrong == "head_order":
        o = o.permute(0, 2, 3, 1).reshape(n, L, D_NEW)
    else:
        o = o.permute(0, 2, 1, 3).reshape(n, L, D_NEW)
    return _lin(o, blk["attn.c_proj"], dtype)


def extract(net, obs, dtype=torch.float64, heads_stacking=4, pe=None, wrong=None):
    """obs (n, K, 15 | 17) -> the extractor's features (n, L_new * 32) in dtype. wrong: a negative
    control (qk_swap, head_order, tanh_gelu, unbiased_var, no_pe)."""
    x = _t(obs, dtype)
    n, k, d = x.shape
    if d == 15:
        x = frame_features(x)
    y = torch.relu(_lin(x, net["embed"], dtype))
    if wrong != "no_pe":
        y = y + (positional_table(k) if pe is None else _t(pe, torch.float32)).to(dtype)
    L, C = new_dims(k)
    flat = torch.zeros((n, k * EMBED), dtype=dtype)
    flat[:, torch.as_tensor(flat_index(k, EMBED, heads_stacking).reshape(-1))] = y.reshape(n, -1)
    z = torch.relu(_lin(flat.reshape(n, L, C), net["embed2"], dtype))
    for blk in net["blocks"]:
        z = z + _attention(_layernorm(z, blk["ln_1"], dtype, wrong == "unbiased_var"), blk, dtype, wrong)
        hdn = _gelu(_lin(_layernorm(z, blk["ln_2"], dtype, wrong == "unbiased_var"), blk["mlp.c_fc"], dtype),
                    wrong == "tanh_gelu")
        z = z + _lin(hdn, blk["mlp.c_proj"], dtype)
    return z.reshape(n, -1)


def forward(net, obs, eps, dtype=torch.float64, activation="tanh", heads_stacking=4, pe=None, wrong=None):
    """(features, actions, values, log_probs, mean) as numpy arrays of dtype."""
    f = extract(net, obs, dtype, heads_stacking, pe, wrong)
    act = torch.tanh if activation == "tanh" else torch.relu

    def mlp(layers):
        h = f
        for wb in layers:
            h = act(_lin(h, wb, dtype))
        return h
    mean = _lin(mlp(net["pi"]), net["act"], dtype)
    values = _lin(mlp(net["vf"]), net["val"], dtype)[:, 0]
    e, ls = _t(eps, dtype), _t(net["log_std"], dtype)
    actions = mean + torch.exp(ls) * e
    lp = (-0.5 * e * e - ls - LOG_SQRT_2PI).sum(-1)
    return tuple(a.numpy() for a in (f, actions, values, lp, mean))


# ---------------------------------------------------------------------------------------------
# the blob and the kernel instance, restated from include/f16env.h and DESIGN.md section 4
def _pieces(k, n_layers, ff, pi_widths, vf_widths):
    """[(name, kind, rows stored, outputs used, fan_in)] in blob order; kind "w" (operand-form
    weight followed by its bias) or "v" (a plain vector of `rows` floats)."""
    L, C = new_dims(k)
    out = []
    for name, widths in (("pi", pi_widths), ("vf", vf_widths)):
        fan_in = L * D_NEW
        for l, w in enumerate(widths):
            out.append(("%s%d" % (name, l), "w", int(w), int(w), fan_in))
            fan_in = int(w)
    out += [("act", "w", 32, 4, int(pi_widths[-1])), ("val", "w", 32, 1, int(vf_widths[-1])), ("log_std", "v", 4, 4, 0),
            ("pe", "v", k * EMBED, k * EMBED, 0), ("embed", "w", EMBED, EMBED, FEATURES), ("embed2", "w", D_NEW, D_NEW, C)]
    for i in range(n_layers):
        b = "blocks.%d." % i
        out += [(b + "ln_1.w", "v", D_NEW, D_NEW, 0), (b + "ln_1.b", "v", D_NEW, D_NEW, 0),
                (b + "attn.c_attn", "w", 3 * D_NEW, 3 * D_NEW, D_NEW), (b + "attn.c_proj", "w", D_NEW, D_NEW, D_NEW),
                (b + "ln_2.w", "v", D_NEW, D_NEW, 0), (b + "ln_2.b", "v", D_NEW, D_NEW, 0),
                (b + "mlp.c_fc", "w", ff, ff, D_NEW), (b + "mlp.c_proj", "w", D_NEW, D_NEW, ff)]
    return out


def blob_floats(k, n_layers, ff, pi_widths, vf_widths):
    return sum(rows if kind == "v" else (rows // 32) * ((fan_in + 1) // 2) * 64 + rows
               for _, kind, rows, _, fan_in in _pieces(k, n_layers, ff, pi_widths, vf_widths))


def unpack_blob(k, n_layers, ff, pi_widths, vf_widths, blob):
    """The layers a blob holds by the documented element map alone: weight element W[o][i] of a
    piece with nks = ceil(fan_in / 2) k-steps at ((o // 32 * nks + i // 2) * 2 + i % 2) * 32 + o % 32
    from the piece's start, its bias after it; vectors as they are. Returns {name: (W, b) | vector,
    "zero": positions that must hold zero, "claims": how many pieces claim each float}."""
    blob = np.asarray(blob)
    claims, zero, out, p = np.zeros(blob.shape[0], np.int64), [], {}, 0
    for name, kind, rows, used, fan_in in _pieces(k, n_layers, ff, pi_widths, vf_widths):
        assert p % 4 == 0, "a piece starts on a multiple of 4 floats"
        if kind == "v":
            out[name] = blob[p:p + rows]
            claims[p:p + rows] += 1
            p += rows
            continue
        nks = (fan_in + 1) // 2
        o, i = np.arange(rows)[:, None], np.arange(2 * nks)[None, :]
        pos = p + ((o // 32 * nks + i // 2) * 2 + i % 2) * 32 + o % 32
        p += (rows // 32) * nks * 64
        bpos = p + np.arange(rows)
        p += rows
        np.add.at(claims, pos.ravel(), 1)
        np.add.at(claims, bpos, 1)
        zero += [pos[used:, :].ravel(), pos[:used, fan_in:].ravel(), bpos[used:]]
        out[name] = (blob[pos[:used, :fan_in]], blob[bpos[:used]])
    assert p == blob.shape[0] == blob_floats(k, n_layers, ff, pi_widths, vf_widths)
    out["zero"] = np.concatenate(zero)
    out["claims"] = claims
    return out


def kernel_instance(k, d, n_layers, ff, pi_widths, vf_widths):
    """(D, dynamic LDS bytes) of the f16_policy_lma_forward_kernel<D> launch a descriptor gets, by
    DESIGN section 4's budget. Per block: the residual stream L_new x 1024 floats; with blocks, k
    and v of every token (L_new x 2048); 32 floats for the value row. Per wave (four of them): the
    LayerNorm and attention-output images, 1024 each, and the widest phase of its scratch: one
    token's frame (608) and embedding (64 x 32); with blocks gelu(c_fc) (ff x 32); a branch's
    hidden image (widest layer x 32). It must fit the CU's 160 KiB (the host launcher checks)."""
    L, _ = new_dims(k)
    scratch = [608 + EMBED * 32, max(list(pi_widths) + list(vf_widths)) * 32] + ([ff * 32] if n_layers else [])
    lds = 4 * (L * 1024 + (L * 2048 if n_layers else 0) + 32 + WAVES_PER_BLOCK * (2048 + max(scratch)))
    assert lds <= LDS_BYTES
    return int(d), lds


# name: K, D, blocks, ff, pi, vf, activation, heads_stacking, (D, LDS bytes) of the instance it reaches
MATRIX = {
    "R": (10, 15, 2, 128, [64, 64], [128, 64], "tanh", 4, (15, 159872)),    # the reference's network, raw frames
    "R17": (10, 17, 2, 128, [64, 64], [128, 64], "tanh", 4, (17, 159872)),  # the feature window in place
    "S": (4, 15, 2, 128, [64, 64], [64, 64], "tanh", 4, (15, 123008)),      # the bench's K; L_new 2
    "T": (7, 17, 1, 64, [32], [32], "tanh", 4, (17, 99968)),               # C_new 224, L_new 2, ff of two tiles
    "U": (9, 15, 3, 32, [96], [128], "tanh", 4, (15, 147584)),              # C_new 144, L_new 4, three blocks
    "V": (1, 17, 2, 128, [32], [32], "tanh", 4, (17, 110720)),              # one token: softmax of one score
    "W": (3, 15, 0, 128, [64], [64], "relu", 4, (15, 79488)),              # no block; C_new 192; exact layout
    "X": (10, 15, 2, 128, [64, 64], [128, 64], "tanh", 2, (15, 159872)),    # a second permutation (dk 32)
}


def random_net(name, seed=0, matrix=None):
    """Case `name` as a random float32 net: weights N(0, 2 / fan_in), biases N(0, 0.01), LayerNorm
    weights 1 + N(0, 0.1); made from a fixed seed, numpy arrays."""
    k, d, nl, ff, pi_w, vf_w, _, _, _ = (matrix or MATRIX)[name]
    rng = np.random.default_rng(52000 + 131 * sum(map(ord, name)) + seed)
    L, C = new_dims(k)

    def lin(o, i):
        return ((rng.standard_normal((o, i)) * math.sqrt(2.0 / i)).astype(np.float32),
                (rng.standard_normal(o) * 0.1).astype(np.float32))

    def ln():
        return ((1.0 + 0.1 * rng.standard_normal(D_NEW)).astype(np.float32), (rng.standard_normal(D_NEW) * 0.1).astype(np.float32))

    def branch(widths):
        out, fan_in = [], L * D_NEW
        for w in widths:
            out.append(lin(w, fan_in))
            fan_in = w
        return out
    net = {"embed": lin(EMBED, FEATURES), "embed2": lin(D_NEW, C), "blocks": []}
    for _ in range(nl):
        net["blocks"].append({"ln_1": ln(), "attn.c_attn": lin(3 * D_NEW, D_NEW), "attn.c_proj": lin(D_NEW, D_NEW),
                              "ln_2": ln(), "mlp.c_fc": lin(ff, D_NEW), "mlp.c_proj": lin(D_NEW, ff)})
    net.update({"pi": branch(pi_w), "vf": branch(vf_w), "act": lin(4, pi_w[-1]), "val": lin(1, vf_w[-1]),
                "log_std": np.array([-0.5, 0.0, 0.25, 0.5], np.float32)})
    return net
