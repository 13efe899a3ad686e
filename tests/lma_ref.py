"""Checker of the device LMA policy (f16env_policy_lma_forward): a plain-torch restatement of the
eval-mode forward (the per-frame feature transform, embedding + positional table, the stacking
permutation, the second embedding, the attention / MLP blocks, the two MLPs, heads, sample and
log-prob) in a chosen dtype, written from the formulas of include/f16env.h; the re-chunk rule
(new_dims), the permutation as an index map, the documented blob layout read back (unpack_blob),
the documented LDS rule (kernel_instance), the case matrix the CPU and GPU tests share with its
inputs, the exact-integer nets, and the stress inputs (a saturated softmax, LayerNorm rows far from
zero, degenerate and huge rows) with the float32 restatements that show they bite: a second
summation order, and two planted defects (softmax without its max subtraction, a one-pass variance).
Nothing here imports f16_jsb_amd."""
from __future__ import annotations

import functools
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


def _lin(x, wb, dtype, flip=False):
    """flip: the same products summed in another order (both operands reversed along the reduced
    axis): what a correct kernel with another k-step order would compute."""
    w = _t(wb[0], dtype)
    y = x.flip(-1).contiguous() @ w.flip(-1).contiguous().T if flip else x @ w.T
    return y if wb[1] is None else y + _t(wb[1], dtype)


def _layernorm(z, wb, dtype, wrong=None, probe=None):
    mean = z.mean(-1, keepdim=True)
    d = z - mean
    if probe is not None:
        probe.setdefault("ln_mean", []).append(mean.to(torch.float64).reshape(-1).numpy())
        probe.setdefault("ln_spread", []).append(d.to(torch.float64).std(-1, unbiased=False).reshape(-1).numpy())
    if wrong == "one_pass_var":   # the planted defect: E[x^2] - mean^2, cancelling when |mean| >> spread
        var = (z * z).mean(-1, keepdim=True) - mean * mean
    else:
        var = (d * d).sum(-1, keepdim=True) / (z.shape[-1] - (1 if wrong == "unbiased_var" else 0))
    y = d / torch.sqrt(var + 1e-5) * _t(wb[0], dtype)
    return y if wb[1] is None else y + _t(wb[1], dtype)


def _gelu(x, tanh_form=False):
    if tanh_form:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _attention(z, blk, dtype, wrong=None, flip=False, probe=None):
    n, L, _ = z.shape
    qkv = _lin(z, blk["attn.c_attn"], dtype, flip)
    q, k, v = qkv[..., :D_NEW], qkv[..., D_NEW:2 * D_NEW], qkv[..., 2 * D_NEW:]
    if wrong == "qk_swap":
        q, k = k, q

    def heads(a):  # (n, L, 32) -> (n, 4, L, 8): head hd holds dims 8 hd .. 8 hd + 7
        if wrong == "head_order":
            return a.reshape(n, L, D_NEW // HEADS, HEADS).permute(0, 3, 1, 2)
        return a.reshape(n, L, HEADS, D_NEW // HEADS).permute(0, 2, 1, 3)
    q, k, v = heads(q), heads(k), heads(v)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(D_NEW // HEADS)
    if probe is not None:
        probe["max_score"] = max(probe.get("max_score", 0.0), float(s.abs().max()))
    if wrong != "naive_softmax":   # the planted defect: exp of the raw score
        s = s - s.max(-1, keepdim=True).values
    p = torch.exp(s)
    p = p / p.sum(-1, keepdim=True)
    o = p @ v
    if wrong == "head_order":
        o = o.permute(0, 2, 3, 1).reshape(n, L, D_NEW)
    else:
        o = o.permute(0, 2, 1, 3).reshape(n, L, D_NEW)
    return _lin(o, blk["attn.c_proj"], dtype, flip)


def extract(net, obs, dtype=torch.float64, heads_stacking=4, pe=None, wrong=None, flip=False, probe=None):
    """obs (n, K, 15 | 17) -> the extractor's features (n, L_new * 32) in dtype. wrong: a negative
    control (qk_swap, head_order, tanh_gelu, unbiased_var, no_pe) or a planted numerical defect
    (naive_softmax, one_pass_var). flip: every linear summed in the other order. probe: a dict that
    receives the largest |attention score| ("max_score"), per LayerNorm every input row's mean and
    spread ("ln_mean", "ln_spread"), and per observation row the largest |argument| of a GELU
    ("gelu_arg"; forward adds "act_arg", the same of the MLPs' activation)."""
    x = _t(obs, dtype)
    n, k, d = x.shape
    if d == 15:
        x = frame_features(x)
    y = torch.relu(_lin(x, net["embed"], dtype, flip))
    if wrong != "no_pe":
        y = y + (positional_table(k) if pe is None else _t(pe, torch.float32)).to(dtype)
    L, C = new_dims(k)
    flat = torch.zeros((n, k * EMBED), dtype=dtype)
    flat[:, torch.as_tensor(flat_index(k, EMBED, heads_stacking).reshape(-1))] = y.reshape(n, -1)
    z = torch.relu(_lin(flat.reshape(n, L, C), net["embed2"], dtype, flip))
    for blk in net["blocks"]:
        z = z + _attention(_layernorm(z, blk["ln_1"], dtype, wrong, probe), blk, dtype, wrong, flip, probe)
        pre = _lin(_layernorm(z, blk["ln_2"], dtype, wrong, probe), blk["mlp.c_fc"], dtype, flip)
        if probe is not None:
            probe["gelu_arg"] = np.maximum(probe.get("gelu_arg", 0.0), pre.abs().amax((1, 2)).to(torch.float64).numpy())
        hdn = _gelu(pre, wrong == "tanh_gelu")
        z = z + _lin(hdn, blk["mlp.c_proj"], dtype, flip)
    return z.reshape(n, -1)


def forward(net, obs, eps, dtype=torch.float64, activation="tanh", heads_stacking=4, pe=None, wrong=None, flip=False,
            probe=None):
    """(features, actions, values, log_probs, mean) as numpy arrays of dtype."""
    f = extract(net, obs, dtype, heads_stacking, pe, wrong, flip, probe)
    act = torch.tanh if activation == "tanh" else torch.relu

    def mlp(layers):
        h = f
        for wb in layers:
            h = _lin(h, wb, dtype, flip)
            if probe is not None:
                probe["act_arg"] = np.maximum(probe.get("act_arg", 0.0), h.abs().amax(1).to(torch.float64).numpy())
            h = act(h)
        return h
    mean = _lin(mlp(net["pi"]), net["act"], dtype, flip)
    values = _lin(mlp(net["vf"]), net["val"], dtype, flip)[:, 0]
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
    # the rest of the lattice the host launcher accepts (NEW_CASES)
    "K2": (2, 17, 1, 96, [32], [32], "tanh", 1, (17, 94336)),               # L 1, C 128, dk 64, lma_fc<3>, proj2 of 48 k-steps
    "K5": (5, 15, 2, 96, [64], [96], "relu", 8, (15, 106624)),              # L 2, C 160, ReLU with blocks
    "K6": (6, 15, 2, 96, [64, 64], [64], "tanh", 16, (15, 118912)),         # L 3: wave 3 idle through the blocks
    "K6r": (6, 17, 3, 64, [128, 128, 128], [32, 32, 32], "relu", 32, (17, 135296)),   # L 3, dk 2, three MLP layers
    "K8": (8, 15, 1, 128, [64], [64], "tanh", 1, (15, 147584)),             # L 4 at C 128
    "Y": (10, 15, 3, 128, [128, 128, 128], [128, 128, 128], "tanh", 8, (15, 159872)),  # the largest descriptor taken
}
NEW_CASES = ("K2", "K5", "K6", "K6r", "K8", "Y")
N_ROWS = 257


def shared_inputs(name, matrix=None):
    """257 standard-normal rows and a fixed eps for a case, from a fixed seed."""
    k, d = (matrix or MATRIX)[name][:2]
    rng = np.random.default_rng(900 + sum(map(ord, name)))
    return rng.standard_normal((N_ROWS, k, d)).astype(np.float32), rng.standard_normal((N_ROWS, 4)).astype(np.float32)


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


# ---------------------------------------------------------------------------------------------
# the exact-integer nets: every sum exact in float32, so the kernel must equal int64 bit for bit
STACKINGS = (1, 2, 4, 8, 16, 32)
INT_ROWS = 33   # one row alone in a second block


def int_case(k, keep=0.2):
    """(net, pe): integer weights in {-1, 0, 1} thinned by a keep-rate, biases and an integer PE
    table in -2..2, ReLU, no block; from a fixed seed per K. At keep 0.2 the largest sum of
    magnitudes over all K and stackings is 731 (K 9, hs 16), far below 2^24: no K needs a thinner
    W_2 (test_lma_cpu checks the guard for all 60)."""
    rng = np.random.default_rng(40 + k)
    L, C = new_dims(k)

    def sparse(o, i, keep):
        return (rng.integers(-1, 2, (o, i)) * (rng.random((o, i)) < keep)).astype(np.int64)
    net = {"embed": (sparse(64, 17, 0.5), rng.integers(-2, 3, 64)), "embed2": (sparse(32, C, keep), rng.integers(-2, 3, 32)),
           "blocks": [], "pi": [(sparse(64, L * 32, keep), rng.integers(-2, 3, 64))],
           "vf": [(sparse(64, L * 32, keep), rng.integers(-2, 3, 64))], "act": (sparse(4, 64, 0.3), rng.integers(-2, 3, 4)),
           "val": (sparse(1, 64, 0.3), rng.integers(-2, 3, 1)), "log_std": np.zeros(4)}
    pe = rng.integers(-2, 3, (k, 64))
    return net, pe


def int_inputs(k, n, d=FEATURES):
    return np.random.default_rng(n).integers(-2, 3, (n, k, d)).astype(np.int64)


def int_forward(net, pe, x, hs=4):
    """The integer network in int64: (features, mean, value, the largest sum of magnitudes any
    output met)."""
    n, k, _ = x.shape
    L, C = new_dims(k)
    bound = [0]

    def lin(h, wb):
        bound[0] = max(bound[0], int((np.abs(h) @ np.abs(wb[0]).T + np.abs(wb[1])).max()))
        return h @ wb[0].T + wb[1]
    y = np.maximum(lin(x, net["embed"]), 0) + pe
    flat = np.zeros((n, k * EMBED), np.int64)
    flat[:, flat_index(k, EMBED, hs).reshape(-1)] = y.reshape(n, -1)
    f = np.maximum(lin(flat.reshape(n, L, C), net["embed2"]), 0).reshape(n, -1)
    mean = lin(np.maximum(lin(f, net["pi"][0]), 0), net["act"])
    value = lin(np.maximum(lin(f, net["vf"][0]), 0), net["val"])[:, 0]
    return f, mean, value, bound[0]


# ---------------------------------------------------------------------------------------------
# stress inputs: net K6 (L_new 3, ff 96, dk 4, tanh) on the first 65 of its shared rows
STRESS_CASE, STRESS_ROWS = "K6", 65
STRESS = ("sharp", "offset", "degenerate", "saturated")
ZERO_ROW, REPEAT_ROW, HUGE_ROW = 3, 40, 64   # 64: alone in the third block
SHARP_FACTOR, LN_OFFSET, HUGE = 8.0, 100.0, 1e4


def sharpen(net, factor=SHARP_FACTOR):
    """The q and k rows (the first 64 outputs) of every block's c_attn.weight times `factor`: the
    scores grow by factor^2 and the softmax saturates. (4 was tried and rejected: sharp but not
    saturated, where another summation order alone moves the features by 3.6 x torch's error.)"""
    out = dict(net, blocks=[])
    for blk in net["blocks"]:
        w = blk["attn.c_attn"][0].copy()
        w[:2 * D_NEW] *= np.float32(factor)
        out["blocks"].append(dict(blk, **{"attn.c_attn": (w, blk["attn.c_attn"][1])}))
    return out


def offset_layernorm(net, offset=LN_OFFSET):
    """embed2's bias plus `offset`: every LayerNorm input row has mean about `offset` and the
    spread it had, so a variance formed as E[x^2] - mean^2 cancels."""
    return dict(net, embed2=(net["embed2"][0], (net["embed2"][1] + np.float32(offset)).astype(np.float32)))


def stress_case(kind):
    """(net, x, eps, rows): the net and the 65 input rows of a stress input, and the rows the
    4 x torch rule is asserted on (None: all of them)."""
    net = random_net(STRESS_CASE)
    xs, es = shared_inputs(STRESS_CASE)
    x, eps, rows = xs[:STRESS_ROWS].copy(), es[:STRESS_ROWS].copy(), None
    if kind == "sharp":
        net = sharpen(net)
    elif kind == "offset":
        net = offset_layernorm(net)
    elif kind == "degenerate":   # dist = 0 and atan2(0, 0) in every frame; K equal frames
        x[ZERO_ROW] = 0.0
        x[REPEAT_ROW] = x[REPEAT_ROW, 0]
        rows = np.array([ZERO_ROW, REPEAT_ROW])
    elif kind == "saturated":    # +-1e4 in every slot of one row
        x[HUGE_ROW] = np.where(x[HUGE_ROW] < 0, -HUGE, HUGE).astype(np.float32)
        rows = np.array([HUGE_ROW])
    else:
        raise KeyError(kind)
    return net, x, eps, rows


@functools.lru_cache(maxsize=None)
def stress_refs(kind):
    """(fp64 restatement, torch float32 restatement, probe of the fp64 run) of a stress input:
    computed once, shared by the CPU and GPU tests, not changed."""
    net, x, eps, _ = stress_case(kind)
    act, hs = MATRIX[STRESS_CASE][6:8]
    probe = {}
    return forward(net, x, eps, torch.float64, act, hs, probe=probe), forward(net, x, eps, torch.float32, act, hs), probe


def errors(got, ref, rows=None):
    """Per output kind max |got - ref| and the floor 2^-24 max|ref|, over `rows`."""
    out = []
    for g, r in zip(got, ref):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        if rows is not None:
            g, r = g[rows], r[rows]
        out.append((float(np.abs(g - r).max()) if np.all(np.isfinite(g)) else float("inf"), 2.0 ** -24 * float(np.abs(r).max())))
    return out
